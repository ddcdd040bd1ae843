"""The one-wave padded chain over every class of chain shape its plan accepts (fast_shapes.py), on the CPU
emulator (tests/emu), no GPU:

* the census of build_fast_plan over L = 2..8, p = 2..7, Q = 1..8 equals tests/golden/fast_plan_census.json
  (make_fast_plan_census.py), and the class labels of the shape table hold in it;
* the precondition of test_fast_shapes_gpu.py: for every (shape, setting, direction) of the table the
  emulated one-wave chain, the emulated general chain and the oracle give equal bond dimensions and
  |<ref|x>| within 1e-12 of 1 -- the inputs are well posed (no truncation through a tie), so the same
  assertion on the device tests the device code and nothing else;
* the padded overlap <x|y>, <x|dH|y> (csrc/fast_overlap.hpp) of every accepted shape against the oracle to
  1e-12 (relative to max(1, |value|) for dH, as test_emu.py)."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

import fast_shapes as FS
import oracle_ffi as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")

with open(os.path.join(HERE, "golden", "fast_plan_census.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def E():
    subprocess.check_call(["make", "-s", "-C", EMU], stdout=subprocess.DEVNULL)
    sys.path.insert(0, EMU)
    import emu_ffi
    return emu_ffi


@pytest.fixture(scope="module")
def census(E):
    spec = importlib.util.spec_from_file_location("make_fast_plan_census",
                                                  os.path.join(HERE, "golden", "make_fast_plan_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(E, FS.CENSUS_RANGE)


def _key(s):
    return "%d,%d,%d" % tuple(s)


def test_census_equals_fixture(census):
    assert len(FS.CENSUS_RANGE) == 307 and sorted(census) == sorted(GOLDEN)
    differ = {k: (census[k], GOLDEN[k]) for k in GOLDEN if census[k] != GOLDEN[k]}
    assert not differ, differ
    assert sum(v["accepted"] for v in GOLDEN.values()) == 170
    assert all(v["ovl"] for v in GOLDEN.values() if v["accepted"])  # every one-wave context has the padded overlap


def test_table_labels():
    """the class a shape stands for is what its plan shows, and each rejected neighbour is rejected for the
    reason the table gives, between accepted shapes where it marks a ragged edge"""
    for s, (label, want, _) in FS.ACCEPTED.items():
        c = GOLDEN[_key(s)]
        assert c["accepted"], (s, label, c["why_not"])
        assert {k: c[k] for k in want} == want, (s, label, c)
    for s, why in FS.REJECTED.items():
        assert not GOLDEN[_key(s)]["accepted"] and GOLDEN[_key(s)]["why_not"] == why, (s, GOLDEN[_key(s)])
    for a, r, b in (((4, 4, 5), (4, 4, 6), (4, 4, 7)), ((8, 2, 3), (8, 2, 4), (8, 2, 5))):
        assert GOLDEN[_key(a)]["accepted"] and not GOLDEN[_key(r)]["accepted"] and GOLDEN[_key(b)]["accepted"]
    assert sum(1 for v in GOLDEN.values() if v.get("maxr") == 1) == 18
    assert max(v["nops"] for v in GOLDEN.values() if v["accepted"]) == 13  # of kMaxOps = 16


@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("setting", FS.SETTINGS, ids=lambda s: "m%d_c%g" % s)
@pytest.mark.parametrize("shape", list(FS.ACCEPTED) + list(FS.REJECTED), ids=FS.shape_id)
def test_inputs_well_posed(E, shape, setting, fwd):
    (L, p, Q), (maxm, cut) = shape, setting
    d, x = FS.tilted_state(L, p, Q)
    u = FS.controls(L, p, Q)
    st = O.Stepper(L, p, Q, FS.J, FS.DT, cut, maxm)
    ref = st.steps(O.MPS(L, p, Q, d, x), u, fwd)
    for fast in ([False, True] if shape in FS.ACCEPTED else [False]):  # a rejected neighbour: the general chain
        got = O.MPS(L, p, Q, *E.Emu(L, p, Q, FS.J, FS.DT, cut, maxm, fast).steps(d, x, u, fwd))
        dev = abs(abs(st.overlap(ref, got)) - 1.0)
        print(f"  {FS.shape_id(shape)} {'one-wave' if fast else 'general'}: | |<ref|x>| - 1 | = {dev:.2e}, "
              f"bonds {list(map(int, ref.bond_dims()))}")
        assert list(got.bond_dims()) == list(ref.bond_dims())
        assert dev <= 1e-12


@pytest.mark.parametrize("shape", list(FS.ACCEPTED), ids=FS.shape_id)
def test_padded_overlaps(E, shape):
    L, p, Q = shape
    maxm, cut = FS.STEPPED
    e = E.Emu(L, p, Q, FS.J, FS.DT, cut, maxm, True)
    st = O.Stepper(L, p, Q, FS.J, FS.DT, cut, maxm)
    pairs = FS.overlap_pairs(shape, lambda s, u: e.steps(s[0], s[1], u, True))
    if max(O.MPS(L, p, Q, *pairs[0][0]).bond_dims()) > 2:  # Maxm 2 cut: the stepped state sits below the bounds
        assert FS.ed.nelem(pairs[2][0][0], L, p, Q) < GOLDEN[_key(shape)]["np"]
    for (dx, x), (dy, y) in pairs:
        X, Y = O.MPS(L, p, Q, dx, x), O.MPS(L, p, Q, dy, y)
        ref, ref_dH = st.overlap(X, Y), st.overlap_dH(X, Y)
        assert abs(e.overlap_pad(dx, x, dy, y) - ref) <= 1e-12
        assert abs(e.overlap_pad(dx, x, dy, y, True) - ref_dH) <= 1e-12 * max(1.0, abs(ref_dH))
