"""Inputs and checks of the decomposition tests (test_eigensolver_gpu.py,
test_decomp_edges_gpu.py), and test_decomp_reference.py's CPU check that
numpy's own SVD factors satisfy every one of them.

The reference is numpy's SVD of the block M itself (LAPACK on M, not on its
Gram M M^H: more accurate than the route under test).  Every check is on
gauge-invariant quantities.
"""
import numpy as np

import oracle_ffi as O

EPS = np.finfo(np.float64).eps


def block(rng, n, c, spec, rank=None):
    """n x c complex with singular values spec (length min(n, c) or rank)"""
    r = len(spec) if rank is None else rank
    U, _ = np.linalg.qr(rng.normal(size=(n, r)) + 1j * rng.normal(size=(n, r)))
    V, _ = np.linalg.qr(rng.normal(size=(c, r)) + 1j * rng.normal(size=(c, r)))
    return (U * np.asarray(spec[:r])) @ V.conj().T


def check(M, res, cutoff, maxm):
    k, w, A, B = res
    s = np.linalg.svd(M, compute_uv=False)
    lam = s ** 2
    k_ref = O.truncate(lam, cutoff, maxm)
    assert k == k_ref, (M.shape, k, k_ref)
    # resolved eigenvalues (the kept ones and every one above the unresolved threshold)
    wd = np.sort(w)[::-1]
    assert np.abs(wd[:k] - lam[:k]).max() <= 1e-12 * lam[0], M.shape
    assert np.abs(A.conj().T @ A - np.eye(k)).max() <= 1e-11, M.shape
    U, s2, Vh = np.linalg.svd(M, full_matrices=False)
    Mk = (U[:, :k] * s2[:k]) @ Vh[:k]
    assert np.linalg.norm(A @ B - Mk) <= 1e-9 * np.linalg.norm(M), M.shape


def rule_margin(lam, cutoff, maxm):
    """(k_ref, margin): the truncation rule's kept count on the descending
    spectrum lam (oracle truncate_count, minm 1) and the relative distance
    from cutoff * total of the tail sums that decided it:
    * sum(lam[k_ref:]) < cutoff * total let the rule discard down to k_ref
      (applies when the cutoff discarded anything: k_ref < min(Maxm, n));
    * sum(lam[k_ref - 1:]) >= cutoff * total stopped it (applies when
      k_ref > 1: below that the rule stops at minm whatever the sum).
    inf when the cutoff cannot bind (cutoff * total = 0, or neither applies).

    The eigensolver may leave eigenvalues below ~1e-3 cutoff / n of the trace
    unresolved (set to their mean), which moves a tail sum by up to
    1e-3 cutoff total: inputs with margin >= 1e-3 have one right kept count."""
    lam = np.asarray(lam, dtype=np.float64)
    n = len(lam)
    k_ref = O.truncate(lam, cutoff, maxm)
    ct = cutoff * float(np.clip(lam, 0.0, None).sum())
    margin = np.inf
    if ct > 0:
        if k_ref < min(maxm, n):
            margin = min(margin, abs(ct - lam[k_ref:].sum()) / ct)
        if k_ref > 1:
            margin = min(margin, abs(lam[k_ref - 1:].sum() - ct) / ct)
    return k_ref, margin


MARGIN_MIN = 1e-3


def well_posed(M, cutoff, maxm):
    """the input condition of every new decomposition test: the rule's margin
    on numpy's spectrum (asserted before the GPU is called); returns k_ref"""
    lam = np.linalg.svd(M, compute_uv=False) ** 2
    k_ref, margin = rule_margin(lam, cutoff, maxm)
    assert margin >= MARGIN_MIN, (M.shape, cutoff, maxm, k_ref, margin)
    return k_ref


def check_gauge_free(M, res, cutoff, maxm):
    """check() for inputs whose best rank-k approximation is not unique
    (repeated singular values across the cut): same kept count, eigenvalues
    and orthonormality; ||A B - M_k|| is replaced by
    * B = A^H M to the rounding of a length-n complex dot product per entry,
      ||B - A^H M||_F <= 4 n eps sqrt(k) ||M||_F;
    * ||M - A B||_F <= sqrt(sum(lam[k:])) + 1e-9 ||M||_F: the optimal residual
      plus check()'s 1e-9 (triangle inequality on ||A B - M_k||).
    The zero block: total 0, one kept state (minm 1), A a unit vector, B = 0."""
    k, w, A, B = res
    n = M.shape[0]
    s = np.linalg.svd(M, compute_uv=False)
    lam = s ** 2
    k_ref = O.truncate(lam, cutoff, maxm)
    assert k == k_ref, (M.shape, k, k_ref)
    if not M.any():
        total = float(np.clip(w, 0.0, None).sum())   # (the rule clamps negative eigenvalues to zero)
        assert k == 1 and total == 0.0, (M.shape, k, total)
        assert abs(np.linalg.norm(A) - 1.0) <= 1e-11, (M.shape, "|A|", float(np.linalg.norm(A)))
        assert not B.any(), (M.shape, "B", float(np.abs(B).max()))
        return
    wd = np.sort(w)[::-1]
    assert np.abs(wd[:k] - lam[:k]).max() <= 1e-12 * lam[0], M.shape
    assert np.abs(A.conj().T @ A - np.eye(k)).max() <= 1e-11, M.shape
    nM = np.linalg.norm(M)
    assert np.linalg.norm(B - A.conj().T @ M) <= 4 * n * EPS * np.sqrt(k) * nM, M.shape
    assert np.linalg.norm(M - A @ B) <= np.sqrt(lam[k:].sum()) + 1e-9 * nM, M.shape


def numpy_factors(M, cutoff, maxm):
    """numpy's own answer in denmat_decomp's format: (k_ref, s^2, U_k, U_k^H M)"""
    U, s, _ = np.linalg.svd(M, full_matrices=False)
    lam = s ** 2
    k = O.truncate(lam, cutoff, maxm)
    A = U[:, :k]
    return k, lam, A, A.conj().T @ M


# ---------------------------------------------------------------- the inputs of test_decomp_edges_gpu.py

# neighbours of every dispatch threshold of Engine::decompose_eig / decompose_factors
ORDERS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 87, 88, 89, 95, 96, 97, 127, 128, 129, 191, 192, 193,
          207, 208, 209, 210, 511]
COL_EXTRA = [0, 1, 37]
# (spectrum, cutoff, Maxm) of the order sweep's two passes
SWEEP_PASSES = {"geometric": (lambda n: np.exp(-np.arange(n) / 5.0), 1e-8, 512),
                "harmonic": (lambda n: 1.0 / (1.0 + np.arange(n)), 0.0, 512)}


def sweep_blocks(name, extra):
    """the order sweep's batch of one pass and one column variant"""
    spec, _, _ = SWEEP_PASSES[name]
    rng = np.random.default_rng([len(name), extra])
    return [block(rng, n, n + extra, spec(n)) for n in ORDERS]


KEPT_SHAPES = [(65, 70), (130, 130), (208, 230), (512, 512)]


def kept_maxms():
    """Maxm values of the kept-count sweep (n - 1 and n of every block)"""
    ms = {1, 2, 15, 16, 17, 63, 64, 65}
    for n, _ in KEPT_SHAPES:
        ms |= {n - 1, n}
    return sorted(ms)


def kept_blocks():
    rng = np.random.default_rng(6416)
    return [block(rng, n, c, 1.0 / (1.0 + np.arange(n))) for n, c in KEPT_SHAPES]


STRUCT_ORDERS = [12, 40, 100, 200, 300]


def _unitary(rng, c):
    Q, _ = np.linalg.qr(rng.normal(size=(c, c)) + 1j * rng.normal(size=(c, c)))
    return Q


def _real_block(rng, n, c, spec):
    U, _ = np.linalg.qr(rng.normal(size=(n, n)))
    V, _ = np.linalg.qr(rng.normal(size=(c, n)))
    return (U * spec) @ V.T


def structured_blocks(n):
    """{name: (M, cutoff, [Maxm...], checker)} of (even) order n, c = n + 5 columns"""
    c = n + 5
    rng = np.random.default_rng(7000 + n)
    Q = _unitary(rng, c)[:n]
    d = np.exp(-np.arange(n) / 7.0)
    h = n // 2
    X = block(rng, h, h + 3, np.exp(-np.arange(h) / 5.0))
    XX = np.zeros((n, n + 6), complex)   # (two blocks of h + 3 columns: one column more than the others)
    XX[:h, :h + 3] = X
    XX[h:, h + 3:] = X
    one = block(rng, n, c, np.array([1.3]), rank=1)
    gen = np.exp(-np.arange(n) / 5.0)
    G = check_gauge_free
    return {
        "identity_gram": (0.7 * Q, 1e-8, [512, n // 2], G),            # Gram 0.49 I
        "diagonal_gram": (d[:, None] * Q, 1e-8, [512], G),             # zero Householder vectors
        "permuted_diagonal_gram": (d[rng.permutation(n)][:, None] * Q, 1e-8, [512], G),
        "doubled": (XX, 1e-8, [512], G),                               # every singular value twice
        "rank_one": (one, 1e-8, [512], G),
        "zero": (np.zeros((n, c), complex), 1e-8, [512], G),
        "real": (_real_block(rng, n, c, gen).astype(complex), 1e-8, [512], check),
        "imaginary": (1j * _real_block(rng, n, c, gen), 1e-8, [512], check),
    }


SCALE_ORDERS = [12, 48, 100, 160, 208, 300]
SCALES = [1e30, 1e-30]


def scale_blocks():
    rng = np.random.default_rng(3030)
    return [block(rng, n, n + 7, np.exp(-np.arange(n) / 5.0)) for n in SCALE_ORDERS]


PROBE_ORDERS = [12, 48, 100, 160, 208, 256]   # one per kernel class
FILLER_ORDER = 208
SPLIT_SPE = 16      # eigenvalues per k_heev_bisect_split workgroup
SPLIT_RANGE = (96, 208)
SPLIT_WG_PER_CU = 2  # the launch guard OCG_HBM_SPLIT_WG stood at


def probe_blocks():
    rng = np.random.default_rng(1234)
    Ms = [block(rng, n, n + 11, np.exp(-np.arange(n) / 5.0)) for n in PROBE_ORDERS]
    filler = block(rng, FILLER_ORDER, FILLER_ORDER, np.exp(-np.arange(FILLER_ORDER) / 5.0))
    return Ms, filler


def split_workgroups(n):
    return -(-n // SPLIT_SPE) if SPLIT_RANGE[0] <= n <= SPLIT_RANGE[1] else 0


def filler_count(n_cu):
    """smallest F with the launch's split workgroups above SPLIT_WG_PER_CU per CU"""
    have = sum(split_workgroups(n) for n in PROBE_ORDERS)
    per = split_workgroups(FILLER_ORDER)
    return max(0, (SPLIT_WG_PER_CU * n_cu - have) // per + 1)
