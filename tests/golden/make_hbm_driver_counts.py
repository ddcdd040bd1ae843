"""Launch / step counters of the HBM engine's host drivers (TEST INFRASTRUCTURE):
what every driver of csrc/hbm.hip (hbm_propagate, hbm_gradient_mid,
hbm_gradient_multi, hbm_xi_dH, hbm_hessian_rows, hbm_hessian_ckpt,
hbm_hessian_pipe) launches on config 1's chain (L=5 p=5, 5 particles, dt 0.01,
cutoff 1e-8, Maxm 80, the states of states.npz), read back through
Engine.stats(k) (kinds 0-5: launches, sweep_steps; kind 7, the GEMM kernel:
launches, alg_bytes, alg_flops) and Engine.path_stats().  All are exact
integers; they change when a batch is split or merged or a step is added or
dropped, so the recorded values pin the batches a driver issues.

collect() is also what tests/test_hbm_driver_counts.py replays.

Run on an MI355X with the library to record:
  python tests/golden/make_hbm_driver_counts.py [--out FILE]
  ->  tests/golden/hbm_driver_counts.json
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
L, P, Q, J, DT, CUT, MAXM = 5, 5, 5, 1.0, 0.01, 1e-8, 80
NT = 21
ROWS_ALL = list(range(1, NT - 1))
ROWS_SUB = [3, 4, 11, 17]
# the pipeline's H thread joins the rows that are ready when it looks, so the
# number of GEMM launches (not their total traffic) depends on thread timing
PIPE_SKIP = {"7/launches"}


def _exact(v):
    assert float(v) == int(v), v   # doubles holding exact integers
    return int(v)


def counters(eng, skip=()):
    out = {}
    for k in range(6):
        s = eng.stats(k)
        out[f"{k}/launches"] = _exact(s["launches"])
        out[f"{k}/sweep_steps"] = _exact(s["sweep_steps"])
    s = eng.stats(7)
    for f in ("launches", "alg_bytes", "alg_flops"):
        out[f"7/{f}"] = _exact(s[f])
    for k, v in eng.path_stats().items():
        out[f"path/{k}"] = _exact(v)
    return {k: v for k, v in out.items() if k not in skip}


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            del os.environ[k]


def collect(states):
    """{case name: {counter: int}} of every driver call, each after reset_stats()"""
    from optimalcontrolmps_amd.native import MPS, Engine

    def st(U):
        k = f"L{L}_p{P}_N{Q}_J{J:g}_U{U:g}"
        return MPS(L, P, Q, states[k + "/dims"], states[k + "/data"])

    def engine():
        eng = Engine(L, P, Q, J, DT, CUT, MAXM, engine="hbm")
        eng.set_states(st(50.0), st(2.5))
        return eng

    def ctl(n, seed=31):
        return np.random.default_rng(seed).uniform(2, 10, n)

    out = {}

    def case(name, eng, call, skip=()):
        eng.reset_stats()
        call()
        out[name] = counters(eng, skip)

    u = ctl(NT)
    eng = engine()
    for which in (1, 2, 3):
        case(f"propagate/which{which}", eng, lambda: eng.propagate(u, which))
    eng.close()

    eng = engine()
    for n in (2, 3, 20, 21):
        for mid in ("0", "1"):
            with _env(OCG_HBM_MID=mid):
                case(f"gradient/mid{mid}/N{n}", eng, lambda: eng.gradient(ctl(n, 40 + n)))
    case("gradient_multi/K3", eng, lambda: eng.gradient_multi(np.stack([ctl(NT, 50 + k) for k in range(3)])))
    eng.close()

    eng = engine()
    eng.propagate(u, 3)
    divT, F = eng.div_t(), eng.overlap_factor()
    case("xi_dH", eng, eng.xi_dH)
    case("hessian_rows/all", eng, lambda: eng.hessian_rows(u, ROWS_ALL, F, divT))
    case("xi_dH/again", eng, eng.xi_dH)
    case("hessian_rows/sub", eng, lambda: eng.hessian_rows(u, ROWS_SUB, F, divT))
    eng.close()

    eng = engine()
    for mid in ("1", "0"):
        for K in (1, 3, 8):
            for tag, rows in (("all", ROWS_ALL), ("sub", ROWS_SUB)):
                with _env(OCG_HBM_CKPT=str(K), OCG_HBM_CKPT_MID=mid):
                    case(f"hessian_ckpt/mid{mid}/K{K}/{tag}", eng, lambda: eng.hessian(u, rows))
    eng.close()

    eng = engine()
    with _env(OCG_HBM_PIPE="1"):
        case("hessian_pipe/all", eng, lambda: eng.hessian(u, ROWS_ALL), PIPE_SKIP)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "hbm_driver_counts.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    states = dict(np.load(os.path.join(HERE, "states.npz"), allow_pickle=False))
    out = collect(states)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases, {sum(len(v) for v in out.values())} counters -> {args.out}")


if __name__ == "__main__":
    sys.exit(main())
