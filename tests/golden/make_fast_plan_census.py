"""Census of the one-wave padded chain's plan builder (TEST INFRASTRUCTURE): for every chain shape of
L = 2..8, p = 2..7, Q = 1..8 with Q <= L (p - 1), whether build_fast_plan (csrc/fast_plan.hpp) accepts it,
its why_not text if not, and for an accepted shape the sizes of its plan: padded MPS elements np, step
operations nops, the maxima over the operations of nth (matricisation elements), T (eigenvalues), ngrp
(Jacobi groups), maxr (Jacobi rounds per sweep: 0, 1 for order 2, 3 for orders 3 and 4), dot (Gram dot
length), nf (factor elements), ns (gauge-product elements), and ovl (the padded overlap's plan is in use).
Read through the CPU emulator's export (tests/emu, emu_fast_census), i.e. from this repository's own
builder; no GPU.  A change of eligibility or of a plan's size changes the file, and shows in review.

collect() is also what tests/test_fast_shapes_cpu.py replays.

  python tests/golden/make_fast_plan_census.py [--out FILE]
  ->  tests/golden/fast_plan_census.json
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
EMU = os.path.join(TESTS, "emu")


def key(shape):
    return "%d,%d,%d" % tuple(shape)


def collect(emu_ffi, shapes):
    out = {}
    for s in shapes:
        ok, why, sizes = emu_ffi.fast_census(*s)
        out[key(s)] = dict(accepted=ok, why_not=why, **(sizes or {}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "fast_plan_census.json"))
    args = ap.parse_args()
    sys.path[:0] = [EMU, TESTS, os.path.dirname(TESTS)]
    subprocess.check_call(["make", "-s", "-C", EMU], stdout=subprocess.DEVNULL)
    import emu_ffi
    from fast_shapes import CENSUS_RANGE
    out = collect(emu_ffi, CENSUS_RANGE)
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in out.items())
                + "\n}\n")
    print(f"{len(out)} shapes, {sum(v['accepted'] for v in out.values())} accepted -> {args.out}")


if __name__ == "__main__":
    sys.exit(main())
