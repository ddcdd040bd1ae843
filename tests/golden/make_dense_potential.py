"""How far the oracle-composed reference of the trapped chain (dense_potential.Composed: the CPU oracle's
step, apply_dH and overlaps with exact E passes on the compact blocks, getHessian by calcHessianRow) lands
from the state-vector reference dense_potential.dense_trajectory on every case of test_potential_gpu.py
(TEST INFRASTRUCTURE, no GPU), in the units the device test asserts in:

  F      | F_o - F |
  divT   max | divT_o - divT | / max | divT |
  fid    max | fid_o - fid |
  H      max | H_o - H | / S,  S = max|A| + max|B|
  state  the worst of | |<ref|w>| - 1 | and max | w - ref <ref|w> | over psi_t, xi_t and dH xi_t / |dH xi_t|
         (all t), and of | |xiH_t| - |dH xi_t| | / |dH xi_t|
  sens   max | s_o - s | / (dt max |<xi_t|n_k|psi_t>|),  s[t, k] = dt Re(i <xi_t|n_k|psi_t> F)

and, under "fd", the distance of the dense sum_t w_t s[t, k] (trapezoid weights) from the central difference
of the dense cost in eps_k at h = 1e-4, relative to max_k | sum_t w_t s[t, k] |.

The device tests allow ten times the "cases" figures (1e-12 at the least); a case is usable only while every
figure stays below dense_reference.WELL_POSED.  collect() is also what
tests/test_dense_potential_reference.py replays.

  python tests/golden/make_dense_potential.py [--out FILE]
  ->  tests/golden/dense_potential.json
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def state_deviation(D, ref, got, shape):
    import numpy as np
    worst = 0.0
    for t in range(len(ref["divT"])):
        for key in ("psi", "xi"):
            worst = max(worst, *D.deviation(ref[key][t], D.dense_of(got[key][t])))
        w = D.dense_of(got["xiH"][t])
        n = np.linalg.norm(w)
        xh = D.dense_apply_dH(ref["xi"][t], shape)
        worst = max(worst, abs(n - ref["xiH_norm"][t]) / ref["xiH_norm"][t],
                    *D.deviation(xh / ref["xiH_norm"][t], w / n))
    return float(worst)


def measure(D, T, P, O, name):
    import numpy as np
    traj = P.traj_of(name)
    shape = T.traj_shape(traj)
    (di, xi, _), (dt, xt, _) = T.traj_states(traj)
    u, ref = T.traj_controls(traj), P.pot_reference(name)
    got = P.Composed(O, shape, P.potential(name)).hessian(O.MPS(*shape, di, xi), O.MPS(*shape, dt, xt), u)
    return {"F": float(abs(got["F"] - ref["F"])),
            "divT": float(np.abs(got["divT"] - ref["divT"]).max() / np.abs(ref["divT"]).max()),
            "fid": float(np.abs(got["fid"] - ref["fid"]).max()),
            "H": float(np.abs(got["H"] - ref["H"]).max() / T.hessian_scale(ref)),
            "state": state_deviation(D, ref, got, shape),
            "sens": float(np.abs(got["sens"] - ref["sens"]).max() / P.sens_scale(ref))}


def finite_difference(D, T, P, name):
    """max_k | sum_t w_t s[t, k] - dC/d eps_k | / max_k | sum_t w_t s[t, k] |"""
    import numpy as np
    traj = P.traj_of(name)
    shape = T.traj_shape(traj)
    (_, _, init), (_, _, target) = T.traj_states(traj)
    u, eps, ref = T.traj_controls(traj), P.potential(name), P.pot_reference(name)
    w = np.ones(len(u))
    w[0] = w[-1] = 0.5
    tot = w @ ref["sens"]
    fd = np.zeros(shape[0])
    for k in range(shape[0]):
        e = np.zeros(shape[0])
        e[k] = P.FD_H
        fd[k] = (P.dense_cost(init, target, shape, u, eps + e) - P.dense_cost(init, target, shape, u, eps - e)) \
            / (2 * P.FD_H)
    return float(np.abs(tot - fd).max() / np.abs(tot).max())


def collect(D, T, P, O):
    return {"cases": {name: measure(D, T, P, O, name) for name in P.POT_CASES},
            "fd": {name: finite_difference(D, T, P, name) for name in P.POT_CASES}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dense_potential.json"))
    args = ap.parse_args()
    sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
    import dense_potential as P
    import dense_reference as D
    import dense_trajectory as T
    import oracle_ffi as O
    out = collect(D, T, P, O)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in out["cases"].items():
        print(k, {a: f"{b:.2e}" for a, b in v.items()}, f"fd {out['fd'][k]:.2e}")


if __name__ == "__main__":
    sys.exit(main())
