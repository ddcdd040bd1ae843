"""The HBM engine's decomposition path (Engine::decompose_eig /
decompose_factors through ocg_denmat_decomp) at the edges of its host
dispatch, against numpy's SVD of the block itself (decomp_reference.py;
test_decomp_reference.py shows on the CPU that numpy's own factors pass every
check used here and that every input is well posed).

* order sweep: Gram orders at threshold +- 1 of every kernel choice (LDS body
  < 16, register grids <= 32 / 64 / 128 / 192 / 208, k_heev_vals_small <= 64,
  Gram in LDS <= 88, split multisection >= 96, coop / blocked >= 209) and the
  orders 1, 2, 3, with column counts that end GEMM tiles (32) and K chunks
  (16) mid-tile;
* kept-count sweep: Maxm across vecs_fast's k <= 64 and k_heev_bt's 16-column
  blocks;
* structured blocks: Gram exactly 0.49 I, diagonal, reducible with every
  eigenvalue double, rank 1, zero, real-only, imaginary-only;
* scale invariance over 1e+-30 (absolute constants in the eigensolver);
* launch independence: the same block gives the same bits alone, among other
  orders, and in a launch large enough to cross every launch-size heuristic.
"""
import functools
import subprocess
import sys

import numpy as np
import pytest

import decomp_reference as D

pytestmark = pytest.mark.gpu

L, p, NPART = 20, 7, 20   # an HBM-engine context (the chain shape does not enter)


@pytest.fixture(scope="module")
def eng():
    from optimalcontrolmps_amd.native import Engine
    e = Engine(L, p, NPART, 1.0, 0.005, 1e-8, 512, engine="hbm")
    yield e
    e.close()


def _each(items, fn):
    """fn(item) for every item; all failures reported together, by label"""
    bad = []
    for label, item in items:
        try:
            fn(item)
        except AssertionError as e:
            bad.append(f"{label}: {str(e).splitlines()[0] if str(e) else 'assert'}")
    assert not bad, "\n".join(bad)


def _decomp(eng, Ms, cutoff, maxm):
    """the margin condition on every input first, then one batched call"""
    for M in Ms:
        D.well_posed(M, cutoff, maxm)
    return eng.denmat_decomp(Ms, cutoff, maxm)


@pytest.mark.parametrize("name", list(D.SWEEP_PASSES))
@pytest.mark.parametrize("extra", D.COL_EXTRA)
def test_order_sweep(eng, name, extra):
    """every threshold order and its neighbours in one batch per column variant
    (c = n, n + 1, n + 37); geometric spectrum under the cutoff, and 1 / (1 + i)
    with cutoff 0 (k = n: every eigenvalue resolved, A a full unitary)"""
    _, cutoff, maxm = D.SWEEP_PASSES[name]
    Ms = D.sweep_blocks(name, extra)
    res = _decomp(eng, Ms, cutoff, maxm)

    def one(mr):
        M, r = mr
        D.check(M, r, cutoff, maxm)
        if cutoff == 0.0:
            assert r[0] == M.shape[0], (M.shape, r[0])

    _each([(M.shape, (M, r)) for M, r in zip(Ms, res)], one)


_kept_blocks = functools.lru_cache(maxsize=None)(D.kept_blocks)


@pytest.mark.parametrize("maxm", D.kept_maxms())
def test_kept_count_sweep(eng, maxm):
    """cutoff 0 and a slow spectrum: Maxm alone sets k, across k = 64 | 65
    (eigenvectors in-kernel or by k_heev_bt) and the 16-column blocks' ends"""
    Ms = _kept_blocks()
    res = _decomp(eng, Ms, 0.0, maxm)

    def one(mr):
        M, r = mr
        assert r[0] == min(maxm, M.shape[0]), (M.shape, r[0])
        D.check(M, r, 0.0, maxm)

    _each([(M.shape, (M, r)) for M, r in zip(Ms, res)], one)


@pytest.mark.parametrize("n", D.STRUCT_ORDERS)
def test_structured_blocks(eng, n):
    """one order per kernel class; the non-unique ones through check_gauge_free"""
    blocks = D.structured_blocks(n)
    calls = sorted({m for _, _, maxms, _ in blocks.values() for m in maxms}, reverse=True)
    items = []
    for maxm in calls:
        names = [k for k, v in blocks.items() if maxm in v[2]]
        res = _decomp(eng, [blocks[k][0] for k in names], 1e-8, maxm)
        items += [(f"{k} Maxm {maxm}", (blocks[k], r, maxm)) for k, r in zip(names, res)]

    def one(it):
        (M, cutoff, _, checker), r, maxm = it
        checker(M, r, cutoff, maxm)

    _each(items, one)


def test_scale_invariance(eng):
    """M, 1e30 M and 1e-30 M: same kept counts, w / scale^2 = numpy's spectrum
    of M (1e-12 of the largest), A B / scale = the unscaled A B (2e-9 ||M||_F:
    both are within check()'s 1e-9 of the same M_k)"""
    Ms = D.scale_blocks()
    ref = _decomp(eng, Ms, 1e-8, 512)
    _each([(M.shape, (M, r)) for M, r in zip(Ms, ref)], lambda mr: D.check(mr[0], mr[1], 1e-8, 512))
    for sc in D.SCALES:
        res = _decomp(eng, [sc * M for M in Ms], 1e-8, 512)

        def one(t):
            M, r, r0 = t
            lam = np.linalg.svd(M, compute_uv=False) ** 2
            k = r0[0]
            assert r[0] == k, (M.shape, sc, r[0], k)
            wd = np.sort(r[1])[::-1] / sc ** 2
            assert np.abs(wd[:k] - lam[:k]).max() <= 1e-12 * lam[0], (M.shape, sc)
            assert np.abs(r[2].conj().T @ r[2] - np.eye(k)).max() <= 1e-11, (M.shape, sc)
            assert np.linalg.norm(r[2] @ r[3] / sc - r0[2] @ r0[3]) <= 2e-9 * np.linalg.norm(M), (M.shape, sc)

        _each([((M.shape, sc), (M, r, r0)) for M, r, r0 in zip(Ms, res, ref)], one)


def _cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a
    child process: torch brings its own HIP runtime, which finds no device in a
    process where the library has already initialised the system's"""
    out = subprocess.run([sys.executable, "-c", "import torch; "
                          "print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


def test_launch_independence_bitwise(eng):
    """a block's kept count, eigenvalues and factors do not depend on what else
    is in its launch: each probe (one per kernel class) alone, all probes in one
    call, and all probes among enough order-208 fillers that the launch's split
    workgroups exceed two per CU.  Pipelined == stored, checkpointed == stored
    and sharded == full rest on this."""
    n_cu = _cu_count()
    Ms, filler = D.probe_blocks()
    F = D.filler_count(n_cu)
    assert 13 * F + sum(D.split_workgroups(n) for n in D.PROBE_ORDERS) > D.SPLIT_WG_PER_CU * n_cu
    alone = [_decomp(eng, [M], 1e-8, 512)[0] for M in Ms]
    together = _decomp(eng, Ms, 1e-8, 512)
    D.well_posed(filler, 1e-8, 512)
    crowded = eng.denmat_decomp(Ms + [filler] * F, 1e-8, 512)
    assert eng.path_stats()["coop_fallbacks"] == 0   # (a fallback re-runs a block on another kernel)
    _each([(M.shape, (M, r)) for M, r in zip(Ms, alone)], lambda mr: D.check(mr[0], mr[1], 1e-8, 512))

    def same(t):
        r0, r = t
        assert r[0] == r0[0], ("kept", r[0], r0[0])
        for what, a, b in zip(("w", "A", "B"), r[1:], r0[1:]):
            assert np.array_equal(a, b), (what, float(np.abs(a - b).max()))

    _each([((f"order {n}", mix), (r0, r)) for mix, rs in (("all probes", together), ("probes + fillers", crowded))
           for n, r0, r in zip(D.PROBE_ORDERS, alone, rs)], same)
    # the fillers are copies: the same bits as one another
    _each([(f"filler {i}", (crowded[len(Ms)], r)) for i, r in enumerate(crowded[len(Ms) + 1:])], same)
