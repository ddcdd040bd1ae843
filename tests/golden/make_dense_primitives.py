"""How far the CPU oracle, at the settings of test_dense_primitives_gpu.py (cutoff 1e-14, Maxm 512: nothing
binds), lands from the dense state vector on each of that test's cases (TEST INFRASTRUCTURE, no GPU): per
step case and direction the residual max |w - ref <ref|w>| of the oracle's result w against
ed.exact_step's ref after the case's steps, and per dH case max |w - dH psi| / |dH psi| of the oracle's
zip-up.  The device tests allow ten times these figures (1e-12 at the least); a case is usable only while
its figure stays below dense_reference.WELL_POSED.

collect() is also what tests/test_dense_reference.py replays.

  python tests/golden/make_dense_primitives.py [--out FILE]
  ->  tests/golden/dense_primitives.json
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def collect(D, O):
    import numpy as np
    out = {}
    for name in D.STEP_CASES:
        shape = D.case_shape(name)
        _, dims, data, dense = D.case_state(name)
        st = O.Stepper(*shape, D.J, D.DT, D.CUTOFF, D.MAXM)
        m, u = O.MPS(*shape, dims, data), D.case_controls(name)
        rec = {}
        for key, fwd in (("forward", True), ("backward", False)):
            w = D.dense_of(st.steps(m, u, fwd))
            rec[key] = D.deviation(D.dense_steps(dense, shape, u, fwd), w)[1]
        if name in D.APPLY_CASES:
            ref = D.dense_apply_dH(dense, shape)
            rec["apply_dH"] = float(np.abs(D.dense_of(st.apply_dH(m)) - ref).max() / np.linalg.norm(ref))
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dense_primitives.json"))
    args = ap.parse_args()
    sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
    import dense_reference as D
    import oracle_ffi as O
    out = collect(D, O)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in out.items())
                + "\n}\n")
    for k, v in out.items():
        print(k, {a: f"{b:.2e}" for a, b in v.items()})


if __name__ == "__main__":
    sys.exit(main())
