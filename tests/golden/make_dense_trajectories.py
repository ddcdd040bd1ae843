"""How far the CPU oracle's getHessian, at the settings of test_dense_trajectory_gpu.py (cutoff 1e-14, Maxm
512: nothing binds), lands from the state-vector reference dense_trajectory.dense_trajectory on each of that
test's cases (TEST INFRASTRUCTURE, no GPU), in the units the device test asserts in:

  F      | F_o - F |
  divT   max | divT_o - divT | / max | divT |
  fid    max | fid_o - fid |
  H      max | H_o - H | / S,  S = max|A| + max|B| (the two terms of H cancel tenfold)
  state  the worst of | |<ref|w>| - 1 | and max | w - ref <ref|w> | over the oracle's stored psi_t, xi_t
         and dH xi_t / |dH xi_t| (all t), and of | |xiH_t| - |dH xi_t| | / |dH xi_t|

The device tests allow ten times these figures (1e-12 at the least); a case is usable only while every
figure stays below dense_reference.WELL_POSED.

collect() is also what tests/test_dense_trajectory_reference.py replays.

  python tests/golden/make_dense_trajectories.py [--out FILE]
  ->  tests/golden/dense_trajectories.json
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def state_deviation(D, ref, get, shape):
    """the `state` figure of the module docstring over the stored states get(which, t) -> MPS, all t"""
    import numpy as np
    worst = 0.0
    for t in range(len(ref["divT"])):
        for which, r in ((0, ref["psi"][t]), (1, ref["xi"][t])):
            worst = max(worst, *D.deviation(r, D.dense_of(get(which, t))))
        w = D.dense_of(get(2, t))
        n = np.linalg.norm(w)
        xh = D.dense_apply_dH(ref["xi"][t], shape)
        worst = max(worst, abs(n - ref["xiH_norm"][t]) / ref["xiH_norm"][t],
                    *D.deviation(xh / ref["xiH_norm"][t], w / n))
    return float(worst)


def measure(D, T, O, name):
    import numpy as np
    shape = T.traj_shape(name)
    (di, xi, _), (dt, xt, _) = T.traj_states(name)
    u, ref = T.traj_controls(name), T.traj_reference(name)
    oc = O.OC(O.Stepper(*shape, D.J, D.DT, D.CUTOFF, D.MAXM), O.MPS(*shape, dt, xt), O.MPS(*shape, di, xi),
              len(u), 0.0)
    H = oc.hessian(u, 4)    # the row workers: the same numbers bit for bit
    divT, F = oc.divT_F()
    return {"F": float(abs(F - ref["F"])),
            "divT": float(np.abs(divT - ref["divT"]).max() / np.abs(ref["divT"]).max()),
            "fid": float(np.abs(oc.fidelities(u) - ref["fid"]).max()),
            "H": float(np.abs(H - ref["H"]).max() / T.hessian_scale(ref)),
            "state": state_deviation(D, ref, oc.state, shape)}


def collect(D, T, O):
    return {name: measure(D, T, O, name) for name in T.TRAJ_CASES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dense_trajectories.json"))
    args = ap.parse_args()
    sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
    import dense_reference as D
    import dense_trajectory as T
    import oracle_ffi as O
    out = collect(D, T, O)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in out.items())
                + "\n}\n")
    for k, v in out.items():
        print(k, {a: f"{b:.2e}" for a, b in v.items()})


if __name__ == "__main__":
    sys.exit(main())
