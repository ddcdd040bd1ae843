"""The inputs of test_dense_primitives_gpu.py, pinned on the CPU (dense_reference.py; no GPU):

* canonical_state returns the ranks it drew, and its MPS and its dense vector are one state to 1e-14;
* the census condition over the union of the HBM cases: the Theta products of their first gates have m and
  n in every class around the 16- and 32-edges of k_gemm's tiles and k at 1, off a multiple of 4, 16, 17,
  32 and 33;
* well-posedness: on every step case the CPU oracle at the device test's settings stays within 1e-11 of
  the dense result (max |w - ref <ref|w>|), and the dense result has no Schmidt weight between 1e-20 and
  1e-11, so its ranks above 1e-12 are the bond dimensions of any correct step;
* the recorded oracle-to-dense deviations (tests/golden/dense_primitives.json, make_dense_primitives.py),
  from which the device test takes its bounds, are what the oracle gives now."""
import importlib.util
import json
import os

import numpy as np
import pytest

import dense_reference as D
import oracle_ffi as O
from optimalcontrolmps_amd import ed

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "dense_primitives.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def measured():
    spec = importlib.util.spec_from_file_location("make_dense_primitives",
                                                  os.path.join(HERE, "golden", "make_dense_primitives.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(D, O)


def test_md_is_the_rank_bound():
    """md_of against a count of configurations by enumeration"""
    for L, p, Q in [(5, 5, 5), (4, 3, 6), (6, 2, 3)]:
        md = D.md_of(L, p, Q)
        for b in range(L + 1):
            left, right = ed.counts(b, p), ed.counts(L - b, p)
            for q in range(Q + 1):
                assert md[b, q] == min((left == q).sum(), (right == Q - q).sum())


@pytest.mark.parametrize("name", list(D.STEP_CASES))
def test_state_has_the_drawn_ranks(name):
    L, p, Q, lo, hi = D.STEP_CASES[name][:5]
    drawn, dims, data, dense = D.case_state(name)
    md = D.md_of(L, p, Q)
    assert np.array_equal(dims, drawn) and (drawn <= np.minimum(md, hi)).all()
    if name in D.FULL_CASES:
        assert np.array_equal(drawn, md)
    assert abs(np.linalg.norm(dense) - 1.0) <= 1e-14
    # the round trip: the MPS of the dense vector is the same state again
    d2, x2 = ed.mps_from_full(dense, L, p, Q, rel_cut=1e-30)
    assert np.array_equal(d2, dims)
    assert np.abs(ed.full_from_mps(d2, x2, L, p, Q) - dense).max() <= 1e-14
    # right-canonical with the centre at site 1: orthonormal block rows from site 2 on
    for k, q, n, blk in ed.mps_blocks(dims, data, L, p, Q):
        assert np.abs(blk).max() > 0        # every block the ranks allow is populated
    rows = {}
    for k, q, n, blk in ed.mps_blocks(dims, data, L, p, Q):
        rows[(k, q)] = rows.get((k, q), 0) + blk @ blk.conj().T
    for (k, q), g in rows.items():
        if k > 1:
            assert np.abs(g - np.eye(len(g))).max() <= 1e-13


def test_census_condition():
    census = []
    for name in D.HBM_CASES:
        census += D.theta_census(D.case_state(name)[1], *D.case_shape(name))
    assert D.census_gaps(census) == []
    # what each case is in the list for
    of = lambda name, col: {c[col] for c in D.theta_census(D.case_state(name)[1], *D.case_shape(name))}
    assert 32 in of("L8p4Q8_r15_17", 0) and 17 in of("L8p4Q8_r15_17", 1)
    assert 16 in of("L11p3Q11_r31_33", 0) and max(of("L11p3Q11_r31_33", 0)) > 64    # more than two tiles
    assert {16, 32, 33} <= of("L11p3Q11_r31_33", 1) and {16, 32, 33} <= of("L11p3Q11_r31_33", 2)
    assert {15, 16, 17} <= of("L9p3Q9_r15_17", 2)


def test_census_gaps_sees_a_gap():
    assert D.census_gaps([(1, 1, 1)]) != []
    full = [(v, v, k) for v, k in zip((1, 7, 16, 20, 32, 40), (1, 6, 16, 17, 32, 33))]
    assert D.census_gaps(full) == []
    assert D.census_gaps([c for c in full if c[0] != 32]) == ["m in 32..32", "n in 32..32", "k = 32"]


@pytest.mark.parametrize("name", list(D.STEP_CASES))
def test_well_posed(measured, name):
    """the oracle at the device test's settings lands on the dense result, and the dense result's ranks
    are beyond argument"""
    shape, (_, dims, _, dense), u = D.case_shape(name), D.case_state(name), D.case_controls(name)
    for key, fwd in (("forward", True), ("backward", False)):
        print(f"FIG {name} oracle_vs_dense_{key} {measured[name][key]:.3e}")
        assert measured[name][key] <= D.WELL_POSED
        ranks, above, below = D.schmidt_ranks(D.dense_steps(dense, shape, u, fwd), shape)
        print(f"FIG {name} smallest_weight_{key} {above:.3e} largest_below {below:.3e}")
        assert above >= D.RANK_ABOVE and below <= D.RANK_BELOW
        assert (ranks >= dims).all() and (ranks <= D.md_of(*shape)).all()
    if name in D.APPLY_CASES:
        assert measured[name]["apply_dH"] <= D.WELL_POSED


def test_recorded_deviations(measured):
    """the fixture is what the oracle gives: rounding-level figures move with the BLAS underneath, so equal
    within a factor of 4 or both below 1e-13 (where the device test's bound is its floor of 1e-12)"""
    assert sorted(measured) == sorted(GOLDEN)
    for name, rec in GOLDEN.items():
        assert sorted(rec) == sorted(measured[name])
        for key, v in rec.items():
            w = measured[name][key]
            assert max(v, w) <= max(4 * min(v, w), 1e-13), (name, key, v, w)


def test_dense_references_agree_with_the_oracle():
    """np.vdot with dH_full is the overlap the oracle contracts"""
    name = "L9p3Q9_r15_17"
    shape, (_, dims, data, dense) = D.case_shape(name), D.case_state(name)
    yd, yx = D.clipped_random_mps(np.random.default_rng(9), *shape, 3, 5)
    y = ed.full_from_mps(yd, yx, *shape)
    st = O.Stepper(*shape, D.J, D.DT, D.CUTOFF, D.MAXM)
    X, Y = O.MPS(*shape, dims, data), O.MPS(*shape, yd, yx)
    scale = np.linalg.norm(y)
    assert abs(st.overlap(X, Y) - D.dense_overlap(dense, y, shape)) <= 1e-13 * scale
    assert abs(st.overlap_dH(X, Y) - D.dense_overlap(dense, y, shape, True)) <= 1e-13 * scale * ed.dH_full(*shape[:2]).max()
