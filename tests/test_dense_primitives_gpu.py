"""The caller-facing primitives of both engines (ocg_steps, ocg_step_batch, ocg_overlap, ocg_apply_dH)
against dense state vectors, on complex full-rank inputs of drawn sector ranks (dense_reference.py; the
inputs are pinned on the CPU by test_dense_reference.py), and the rejection of malformed dims before
anything reaches the device.

The HBM cases are chosen by the (m, n, k) of the products their gates perform: together they put m and n
on both sides of the 16- and 32-edges of k_gemm's tiles and k at 1, off a multiple of 4, 16, 17, 32, 33
(test_dense_reference.test_census_condition).

Tolerances.  Steps (cutoff 1e-14, Maxm 512: nothing binds): | |<ref|w>| - 1 | and max |w - ref <ref|w>|
against ed.exact_step, each at most max(1e-12, 10 x the CPU oracle's own deviation from dense on that case
and direction, tests/golden/dense_primitives.json); the factor 10 allows another eigensolver to place
rounding-level eigenvalues on the other side of the cutoff.  Bond dimensions: the dense result's Schmidt
ranks above 1e-12.  apply_dH: norm and state (unnormalised) to the same anchor.  Overlaps:
1e-12 |x| |y| (times max dH with dH) against np.vdot.  A ragged step_batch: bitwise equal to the single
steps.  Maxm binding: equal bond dimensions and |<o|g>| within 1e-12 of 1 against the live oracle.
Every test prints the deviations it asserts ("FIG ..." lines).

Worst figures observed on an MI355X next to their bounds: see DESIGN.md section 14."""
import functools
import json
import os

import numpy as np
import pytest

import dense_reference as D
import oracle_ffi as O
from optimalcontrolmps_amd import ed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "dense_primitives.json")) as _f:
    GOLDEN = json.load(_f)

# which contexts step which case: the HBM engine, the LDS engine's one-wave chain and its general chain
LDS_SHAPES = [(5, 5, 5), (5, 6, 5)]
KINDS = ("hbm", "onewave", "general")


def _kinds(name):
    return KINDS if D.case_shape(name) in LDS_SHAPES else ("hbm",)


def _engine(monkeypatch, shape, kind, maxm=D.MAXM):
    from optimalcontrolmps_amd.native import Engine
    for var, on in (("OCG_NO_FAST", kind == "general"), ("OCG_NO_FAST_OVL", kind == "general_overlap")):
        if on:
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)
    e = Engine(*shape, D.J, D.DT, D.CUTOFF, maxm, engine="hbm" if kind == "hbm" else "lds")
    assert e.info.fast_chain == (1 if kind in ("onewave", "general_overlap") else 0)
    return e


def _mps(shape, dims, data):
    from optimalcontrolmps_amd.native import MPS
    return MPS(*shape, dims, data)


def _case(name):
    _, dims, data, dense = D.case_state(name)
    return _mps(D.case_shape(name), dims, data), dense


def _fig(case, what, value):
    print(f"FIG {case} {what} {value:.3e}")
    return value


def _bound(name, key):
    return max(1e-12, 10.0 * GOLDEN[name][key])


@functools.lru_cache(maxsize=None)
def _dense_step(name, fwd, nsteps=None):
    """(ref, ranks) of the case's steps (or its first nsteps), computed once per session"""
    u = D.case_controls(name)
    u = u if nsteps is None else u[:nsteps + 1]
    ref = D.dense_steps(D.case_state(name)[3], D.case_shape(name), u, fwd)
    return ref, D.schmidt_ranks(ref, D.case_shape(name))[0].reshape(-1)


def _check_step(name, tag, key, got, ref, ranks):
    a, b = D.deviation(ref, D.dense_of(got))
    bound = _bound(name, key)
    _fig(name, f"{tag}_{key}_bound", bound)
    assert _fig(name, f"{tag}_{key}_overlap", a) <= bound
    assert _fig(name, f"{tag}_{key}_residual", b) <= bound
    assert np.array_equal(got.dims, ranks)


CASE_KINDS = [(n, k) for n in D.STEP_CASES for k in _kinds(n)]


@pytest.mark.parametrize("name,kind", CASE_KINDS, ids=["%s-%s" % ck for ck in CASE_KINDS])
def test_steps(monkeypatch, name, kind):
    psi, _ = _case(name)
    u = D.case_controls(name)
    e = _engine(monkeypatch, D.case_shape(name), kind)
    for key, fwd in (("forward", True), ("backward", False)):
        _check_step(name, kind, key, e.steps(psi, u, fwd), *_dense_step(name, fwd))
    e.close()


BATCH_KINDS = [("L9p3Q9", "hbm")] + [("L5p5Q5", k) for k in KINDS]


@pytest.mark.parametrize("batch,kind", BATCH_KINDS, ids=["%s-%s" % bk for bk in BATCH_KINDS])
def test_ragged_batch(monkeypatch, batch, kind):
    """narrow, mid and wide states of one chain in a single step_batch: bitwise the three single steps, and
    each the dense step"""
    names = D.BATCHES[batch]
    shape = D.case_shape(names[0])
    states = [_case(n)[0] for n in names]
    widths = [int(s.bond_dims().max()) for s in states]
    assert widths[0] < widths[1] < widths[2]
    uf = [D.case_controls(n)[0] for n in names]
    ut = [D.case_controls(n)[1] for n in names]
    e = _engine(monkeypatch, shape, kind)
    for key, fwd in (("forward", True), ("backward", False)):
        single = [e.step(s, a, b, fwd) for s, a, b in zip(states, uf, ut)]
        for order in ([0, 1, 2], [2, 0, 1]):
            got = e.step_batch([states[i] for i in order], [uf[i] for i in order], [ut[i] for i in order], fwd)
            for g, i in zip(got, order):
                assert np.array_equal(g.dims, single[i].dims) and np.array_equal(g.data, single[i].data), names[i]
        for n, g in zip(names, got[1:] + got[:1]):
            _check_step(n, f"{kind}_batch", key, g, *_dense_step(n, fwd, 1))
    e.close()


# ------------------------------------------------------------------------------------------- overlaps
def _overlap_operands(shape):
    """[(label, dims, data)]: canonical states of two different ranks and two clipped random states (not
    canonical, not normalised)"""
    L, p, Q = shape
    if shape == (11, 3, 11):
        wide = D.case_state("L11p3Q11_r31_33")[1:3]
        narrow = D.canonical_state(np.random.default_rng(D.OVERLAP_NARROW[5]), *D.OVERLAP_NARROW[:5])[:2]
        lo, hi = (3, 9), (20, 40)
    else:
        wide, narrow = D.case_state("L5p5Q5_full")[1:3], D.case_state("L5p5Q5_r2_2")[1:3]
        lo, hi = (1, 2), (2, 4)
    rng = np.random.default_rng(31)
    return [("narrow", *narrow), ("wide", *wide), ("random_lo", *D.clipped_random_mps(rng, L, p, Q, *lo)),
            ("random_hi", *D.clipped_random_mps(rng, L, p, Q, *hi))]


OVERLAP_KINDS = [((11, 3, 11), "hbm")] + [((5, 5, 5), k) for k in KINDS + ("general_overlap",)]


@pytest.mark.parametrize("shape,kind", OVERLAP_KINDS, ids=["L%dp%dQ%d-%s" % (*s, k) for s, k in OVERLAP_KINDS])
def test_overlaps(monkeypatch, shape, kind):
    case = "L%dp%dQ%d" % shape
    ops = _overlap_operands(shape)
    dense = {lab: ed.full_from_mps(d, x, *shape) for lab, d, x in ops}
    e = _engine(monkeypatch, shape, kind)   # general_overlap: the one-wave context's general contraction
    dmax = ed.dH_full(*shape[:2]).max()
    a, b = 0.3 - 1.7j, -2.1 + 0.4j
    pairs = [("narrow", "wide"), ("wide", "narrow"), ("random_lo", "wide"), ("random_hi", "random_lo"),
             ("random_lo", "random_hi"), ("random_hi", "random_hi")]
    by = {lab: (d, x) for lab, d, x in ops}
    for with_dH in (False, True):
        tag = f"{kind}_overlap_dH" if with_dH else f"{kind}_overlap"
        for lx, ly in pairs:
            X, Y = _mps(shape, *by[lx]), _mps(shape, *by[ly])
            tol = 1e-12 * np.linalg.norm(dense[lx]) * np.linalg.norm(dense[ly]) * (dmax if with_dH else 1.0)
            ref = D.dense_overlap(dense[lx], dense[ly], shape, with_dH)
            got = e.overlap(X, Y, with_dH)
            assert _fig(case, f"{tag}_{lx}_{ly}_vs_dense", abs(got - ref) / tol * 1e-12) <= 1e-12
            assert _fig(case, f"{tag}_{lx}_{ly}_hermitian", abs(e.overlap(Y, X, with_dH) - np.conj(got)) / tol * 1e-12) <= 1e-12
            # sesquilinear: antilinear in the bra, linear in the ket
            Xa = _mps(shape, by[lx][0], D.scaled(*by[lx], shape, a))
            Yb = _mps(shape, by[ly][0], D.scaled(*by[ly], shape, b))
            tab = tol * abs(a) * abs(b)
            assert _fig(case, f"{tag}_{lx}_{ly}_sesquilinear",
                        abs(e.overlap(Xa, Yb, with_dH) - np.conj(a) * b * got) / tab * 1e-12) <= 1e-12
    e.close()


# ------------------------------------------------------------------------------------------- apply_dH
APPLY_KINDS = [(n, k) for n in D.APPLY_CASES for k in _kinds(n)]


@pytest.mark.parametrize("name,kind", APPLY_KINDS, ids=["%s-%s" % nk for nk in APPLY_KINDS])
def test_apply_dH(monkeypatch, name, kind):
    shape = D.case_shape(name)
    psi, dense = _case(name)
    ref = D.dense_apply_dH(dense, shape)
    nref = np.linalg.norm(ref)
    e = _engine(monkeypatch, shape, kind)
    g, nrm = e.apply_dH(psi)
    e.close()
    bound = _fig(name, f"{kind}_apply_dH_bound", _bound(name, "apply_dH"))
    assert _fig(name, f"{kind}_apply_dH_norm", abs(nrm - nref) / nref) <= bound
    assert _fig(name, f"{kind}_apply_dH_state", np.abs(D.dense_of(g) - ref).max() / nref) <= bound


# ---------------------------------------------------------------------------------------- Maxm binding
@pytest.mark.parametrize("name,maxm", [("L8p4Q8_r15_17", 24), ("L11p3Q11_r31_33", 64)])
def test_maxm_binding(monkeypatch, name, maxm):
    """one step with Maxm below the input's bond dimensions, against the live oracle: random spectra have
    no symmetry ties, so the kept set is unique"""
    shape = D.case_shape(name)
    psi, _ = _case(name)
    assert psi.bond_dims().max() > maxm
    u = D.case_controls(name)[:2]
    st = O.Stepper(*shape, D.J, D.DT, D.CUTOFF, maxm)
    e = _engine(monkeypatch, shape, "hbm", maxm)
    g = e.steps(psi, u, True)
    e.close()
    o = st.steps(O.MPS(*shape, psi.dims, psi.data), u, True)
    assert o.bond_dims().max() == maxm
    assert list(g.bond_dims()) == list(o.bond_dims()) and np.array_equal(g.dims, o.dims)
    assert _fig(name, f"maxm{maxm}_vs_oracle", abs(abs(st.overlap(o, O.MPS(*shape, g.dims, g.data))) - 1.0)) <= 1e-12


# ------------------------------------------------------------------------- malformed dims are rejected
BAD_SHAPE = (5, 5, 5)


def _bad_dims(what):
    """(dims, code): the full-rank (5,5,5) dims with one defect"""
    L, p, Q = BAD_SHAPE
    d = D.md_of(L, p, Q).astype(np.int32)
    if what == "negative":
        d[2, 1] = -1
    elif what == "bond0":
        d[0, 0], d[0, 1] = 0, 1
    elif what == "bond0_two_states":
        d[0, 0] = 2
    elif what == "bondL":
        d[L, Q], d[L, Q - 1] = 0, 1
    elif what == "above_md":
        d[2, 2] += 1        # the total still fits a state slot: only the per-sector bound can reject it
    else:
        raise KeyError(what)
    return d.reshape(-1), "ECAP" if what == "above_md" else "EINVAL"


BAD = ["negative", "bond0", "bond0_two_states", "bondL", "above_md"]
CALLS = ["steps", "step_batch_second", "overlap_bra", "overlap_ket", "apply_dH", "set_states_target",
         "set_states_init", "imag_steps", "ground_state"]


def _counters(e):
    return [e.stats(k)["launches"] for k in range(10)] + [e.stats(k)["sweep_steps"] for k in range(10)], \
        e.path_stats()


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("what", BAD)
def test_malformed_dims_are_rejected(monkeypatch, engine, what):
    """every entry point that loads a chain from caller-supplied dims returns EINVAL / ECAP for a malformed
    state before anything reaches the device, and the context is as good as new afterwards"""
    from optimalcontrolmps_amd.native import Engine, OcgError
    monkeypatch.delenv("OCG_NO_FAST", raising=False)
    monkeypatch.delenv("OCG_NO_FAST_OVL", raising=False)
    shape = BAD_SHAPE
    good, _ = _case("L5p5Q5_full")
    other, _ = _case("L5p5Q5_r2_2")
    dims, code = _bad_dims(what)
    bad = _mps(shape, dims, np.zeros(good.data.size + 4096, np.complex128))
    u = D.case_controls("L5p5Q5_full")
    e = Engine(*shape, D.J, D.DT, D.CUTOFF, D.MAXM, engine=engine)
    calls = {
        "steps": lambda: e.steps(bad, u),
        "step_batch_second": lambda: e.step_batch([good, bad, other], [2.0] * 3, [3.0] * 3),
        "overlap_bra": lambda: e.overlap(bad, good),
        "overlap_ket": lambda: e.overlap(good, bad, True),
        "apply_dH": lambda: e.apply_dH(bad),
        "set_states_target": lambda: e.set_states(bad, good),
        "set_states_init": lambda: e.set_states(good, bad),
        "imag_steps": lambda: e.imag_steps(bad, 3.0, 0.05, 2),
        "ground_state": lambda: e.ground_state(bad, 3.0, [0.1, 0.05], block=2, max_steps=4),
    }
    assert sorted(calls) == sorted(CALLS)
    before = _counters(e)
    for name in CALLS:
        with pytest.raises(OcgError, match=r"\(%s\)" % code):
            calls[name]()
        assert _counters(e) == before, name
    with pytest.raises(OcgError, match="ocg_set_states first"):
        e.propagate(u, 3)       # neither rejected set_states left states behind
    # the context afterwards against a fresh one, bit for bit
    f = Engine(*shape, D.J, D.DT, D.CUTOFF, D.MAXM, engine=engine)
    for ctx in (e, f):
        ctx.set_states(good, other)
    uh = np.array([2.0, 3.5, 5.0, 4.0])
    ra, rb = [(c.steps(good, u), c.step_batch([good, other], [2.0, 4.0], [3.0, 5.0]), c.overlap(other, good, True),
               c.apply_dH(other), c.hessian(uh)) for c in (e, f)]
    e.close()
    f.close()
    same = lambda x, y: np.array_equal(x.dims, y.dims) and np.array_equal(x.data, y.data)
    assert same(ra[0], rb[0]) and all(same(x, y) for x, y in zip(ra[1], rb[1]))
    assert ra[2] == rb[2] and same(ra[3][0], rb[3][0]) and ra[3][1] == rb[3][1]
    assert np.array_equal(ra[4][0], rb[4][0]) and np.array_equal(ra[4][1], rb[4][1]) and ra[4][2] == rb[4][2]
