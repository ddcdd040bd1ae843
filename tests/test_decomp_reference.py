"""decomp_reference.py on the CPU: numpy's own SVD factors of every input
test_decomp_edges_gpu.py decomposes pass check() / check_gauge_free(), and
every (order, spectrum, cutoff, Maxm) combination used there is well posed
(rule_margin >= 1e-3: the kept count does not hinge on eigenvalues the
eigensolver may leave unresolved).  So a failure of the GPU tests is the
kernels', not the reference's or the inputs'."""
import functools

import numpy as np
import pytest

import decomp_reference as D


def _own(M, cutoff, maxm, checker):
    D.well_posed(M, cutoff, maxm)
    checker(M, D.numpy_factors(M, cutoff, maxm), cutoff, maxm)


def test_rule_margin_cases():
    lam = np.array([1.0, 1e-3, 1e-6, 1e-9])
    # cutoff 1e-5: discards 1e-9 and 1e-6 (tail 1.001e-6 < 1.001001e-5), keeps 1e-3
    k, m = D.rule_margin(lam, 1e-5, 512)
    ct = 1e-5 * lam.sum()
    assert k == 2
    assert m == pytest.approx(min((ct - lam[2:].sum()) / ct, (lam[1:].sum() - ct) / ct))
    # Maxm alone decides, the cutoff discards nothing more: only the stopping sum applies
    k, m = D.rule_margin(lam, 1e-5, 2)
    assert k == 2 and m == pytest.approx((lam[1:].sum() - ct) / ct)
    # cutoff 0, zero spectrum, one kept state: cannot bind
    assert D.rule_margin(lam, 0.0, 3) == (3, np.inf)
    assert D.rule_margin(np.zeros(5), 1e-8, 512) == (1, np.inf)
    assert D.rule_margin(lam, 1e-8, 1) == (1, np.inf)
    # a tail sum right at the cutoff is flagged
    lam2 = np.array([1.0, 1e-8 * (1 + 1e-5), 0.0])
    assert D.rule_margin(lam2, 1e-8, 512)[1] < D.MARGIN_MIN


def test_checks_reject_wrong_factors():
    """the checks are not vacuous: a rotated A (orthonormal, wrong subspace), a
    B that is not A^H M and an eigenvalue off by 1e-11 are all caught"""
    rng = np.random.default_rng(1)
    M = D.block(rng, 80, 85, np.exp(-np.arange(80) / 5.0))
    k, lam, A, B = D.numpy_factors(M, 1e-8, 512)
    D.check(M, (k, lam, A, B), 1e-8, 512)
    U = np.linalg.svd(M)[0]
    A2 = A.copy()
    A2[:, 0] = np.cos(1e-4) * U[:, 0] + np.sin(1e-4) * U[:, k]
    for chk in (D.check, D.check_gauge_free):
        with pytest.raises(AssertionError):
            chk(M, (k, lam, A2, A2.conj().T @ M), 1e-8, 512)
        with pytest.raises(AssertionError):
            chk(M, (k, lam * (1 + 1e-11), A, B), 1e-8, 512)
        with pytest.raises(AssertionError):
            chk(M, (k - 1, lam, A[:, :k - 1], B[:k - 1]), 1e-8, 512)
    with pytest.raises(AssertionError):
        D.check_gauge_free(M, (k, lam, A, B * (1 + 1e-12)), 1e-8, 512)
    Z = np.zeros((6, 8), complex)
    e0 = np.eye(6, 1, dtype=complex)
    D.check_gauge_free(Z, (1, np.zeros(6), e0, np.zeros((1, 8), complex)), 1e-8, 512)
    with pytest.raises(AssertionError):
        D.check_gauge_free(Z, (1, np.zeros(6), 0 * e0, np.zeros((1, 8), complex)), 1e-8, 512)


@pytest.mark.parametrize("name", list(D.SWEEP_PASSES))
@pytest.mark.parametrize("extra", D.COL_EXTRA)
def test_order_sweep_inputs(name, extra):
    _, cutoff, maxm = D.SWEEP_PASSES[name]
    for M in D.sweep_blocks(name, extra):
        _own(M, cutoff, maxm, D.check)
        if cutoff == 0.0:
            # every eigenvalue kept: the Gram route resolves directions to ~eps cond^2, so cond <= 512
            s = np.linalg.svd(M, compute_uv=False)
            assert D.numpy_factors(M, cutoff, maxm)[0] == M.shape[0] and s[0] / s[-1] <= 512 * (1 + 1e-9)


_kept_blocks = functools.lru_cache(maxsize=None)(D.kept_blocks)


@pytest.mark.parametrize("maxm", D.kept_maxms())
def test_kept_sweep_inputs(maxm):
    assert D.kept_maxms() == [1, 2, 15, 16, 17, 63, 64, 65, 129, 130, 207, 208, 511, 512]
    for M in _kept_blocks():
        _own(M, 0.0, maxm, D.check)
        assert D.numpy_factors(M, 0.0, maxm)[0] == min(maxm, M.shape[0])


@pytest.mark.parametrize("n", D.STRUCT_ORDERS)
def test_structured_inputs(n):
    blocks = D.structured_blocks(n)
    for name, (M, cutoff, maxms, checker) in blocks.items():
        assert M.shape[0] == n and M.shape[0] <= M.shape[1], name
        for maxm in maxms:
            _own(M, cutoff, maxm, checker)
    # the structure each input claims
    M = blocks["identity_gram"][0]
    assert np.abs(M @ M.conj().T - 0.49 * np.eye(n)).max() <= 1e-14
    assert D.numpy_factors(M, 1e-8, 512)[0] == n and D.numpy_factors(M, 1e-8, n // 2)[0] == n // 2
    for name in ("diagonal_gram", "permuted_diagonal_gram"):
        G = blocks[name][0] @ blocks[name][0].conj().T
        assert np.abs(G - np.diag(np.diag(G))).max() <= 1e-15
    s = np.linalg.svd(blocks["doubled"][0], compute_uv=False)
    assert np.abs(s[0::2] - s[1::2]).max() <= 1e-15
    assert np.linalg.matrix_rank(blocks["rank_one"][0]) == 1
    assert not blocks["real"][0].imag.any() and not blocks["imaginary"][0].real.any()


def test_scale_inputs():
    for M in D.scale_blocks():
        k0 = D.numpy_factors(M, 1e-8, 512)[0]
        _own(M, 1e-8, 512, D.check)
        for sc in D.SCALES:
            _own(sc * M, 1e-8, 512, D.check)
            assert D.numpy_factors(sc * M, 1e-8, 512)[0] == k0
            # squares of Gram entries stay inside the fp64 range
            g = np.abs(sc * M).max() ** 2 * M.shape[1]
            assert 1e-150 < g ** 2 < 1e150


def test_probe_inputs():
    Ms, filler = D.probe_blocks()
    for M in Ms + [filler]:
        _own(M, 1e-8, 512, D.check)
    # on 256 CUs: 30 probe workgroups + 13 F > 512 first at F = 38; the call stays under ~90 blocks
    assert sum(D.split_workgroups(n) for n in D.PROBE_ORDERS) == 30
    assert D.filler_count(256) == 38
    for n_cu in (64, 256, 304):
        F = D.filler_count(n_cu)
        assert 13 * F + 30 > 2 * n_cu >= 13 * (F - 1) + 30
    assert len(Ms) + D.filler_count(256) <= 90
