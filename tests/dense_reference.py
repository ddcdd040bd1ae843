"""Inputs and dense references of the primitive tests (test_dense_reference.py on the CPU,
test_dense_primitives_gpu.py on the device): complex right-canonical states of drawn sector ranks, the
(m, n, k) census of the products their first gates perform, and the state-vector references of a time step,
an overlap and dH |psi> (numpy only).

Inputs.  Every other state the suite steps, overlaps or zips up descends from a real ED ground state: its
Schmidt spectra decay steeply and most of its high sectors are numerically empty.  canonical_state() draws
the rank of every bond sector and fills every block with complex numbers of one scale, so the Schmidt
spectra are flat, every sector the ranks allow is populated, and the products of a step have the drawn
shapes.

Well-posedness.  A gate on a bond whose rank is below its Hilbert-space bound md grows that rank; the new
Schmidt weights come in tiers of dt^2 (1e-4, 1e-9, 1e-14, ... at dt = 0.01).  Where the bound is reached
within the first two tiers a cutoff of 1e-14 cuts nothing and the truncated step equals the dense one to
rounding; where the third tier is populated it does not.  test_dense_reference.py measures this per case
with the CPU oracle and records it in tests/golden/dense_primitives.json (make_dense_primitives.py).
"""
import functools

import numpy as np

from optimalcontrolmps_amd import ed

J, DT = 1.0, 0.01
CUTOFF, MAXM = 1e-14, 512       # nothing binds
RANK_WEIGHT = 1e-12             # a Schmidt weight above this counts towards the dense rank
RANK_ABOVE, RANK_BELOW = 1e-11, 1e-20   # no weight of a case's dense result may lie between these
WELL_POSED = 1e-11              # oracle-to-dense deviation every step case must stay below

# HBM-engine step cases: name -> (L, p, Q, lo, hi, seed, steps).  The seeds are those of 1..12 at which
# the dense results have no Schmidt weight between RANK_BELOW and RANK_ABOVE (the third dt^2 tier of
# (11,3,11) sits near 1e-12 and straddles RANK_WEIGHT at most seeds) and the census condition holds.
# The k = 17 case is (9,3,9): at (10,3,10) ranks 15..17 leave bond 5 so far below its bound of 51 that
# the third tier is populated and a cutoff of 1e-14 cuts into it (oracle-to-dense 4e-9); at (9,3,9) the
# bound of the odd bond 5 is 19.
HBM_CASES = {
    "L8p4Q8_r15_17": (8, 4, 8, 15, 17, 7, 2),
    "L11p3Q11_r31_33": (11, 3, 11, 31, 33, 6, 1),
    "L9p3Q9_r15_17": (9, 3, 9, 15, 17, 3, 2),
}
# full-rank (ranks = md) cases of both engines, general LDS chain and one-wave chain
FULL_CASES = {
    "L5p5Q5_full": (5, 5, 5, 1 << 20, 1 << 20, 4, 2),
    "L5p6Q5_full": (5, 6, 5, 1 << 20, 1 << 20, 5, 2),
}
# the narrow and mid members of the ragged batches (one step each; the wide member is a case above)
BATCH_CASES = {
    "L9p3Q9_r7_8": (9, 3, 9, 7, 8, 11, 1),
    "L9p3Q9_r11_13": (9, 3, 9, 11, 13, 12, 1),
    "L9p3Q9_full": (9, 3, 9, 1 << 20, 1 << 20, 13, 1),
    "L5p5Q5_r2_2": (5, 5, 5, 2, 2, 14, 1),
    "L5p5Q5_r3_3": (5, 5, 5, 3, 3, 15, 1),
}
STEP_CASES = {**HBM_CASES, **FULL_CASES, **BATCH_CASES}
# narrow, mid, wide on one chain: a single step_batch call
BATCHES = {"L9p3Q9": ["L9p3Q9_r7_8", "L9p3Q9_r11_13", "L9p3Q9_full"],
           "L5p5Q5": ["L5p5Q5_r2_2", "L5p5Q5_r3_3", "L5p5Q5_full"]}
# dH |psi> cases (the zip-up truncates at the same settings)
APPLY_CASES = ["L8p4Q8_r15_17", "L9p3Q9_r15_17", "L5p5Q5_full", "L5p5Q5_r2_2"]
# overlap operand beside the (11,3,11) step case: bra and ket of different ranks make the transfer
# products rectangular (never stepped, so not a case): (L, p, Q, lo, hi, seed)
OVERLAP_NARROW = (11, 3, 11, 15, 17, 21)


def hs_count(nsites, p, q):
    """configurations of nsites sites with n < p each and q particles in all"""
    c = np.zeros(max(q, 0) + 1, dtype=object)
    c[0] = 1
    for _ in range(nsites):
        c = np.array([sum(c[max(0, j - p + 1):j + 1]) for j in range(len(c))], dtype=object)
    return int(c[q]) if q >= 0 else 0


def md_of(L, p, Q):
    """(L+1, Q+1): the Schmidt-rank bound min(HS_left(b, q), HS_right(L - b, Q - q)) of every bond sector"""
    return np.array([[min(hs_count(b, p, q), hs_count(L - b, p, Q - q)) for q in range(Q + 1)]
                     for b in range(L + 1)], dtype=np.int64)


def draw_ranks(rng, L, p, Q, lo, hi):
    """(L+1, Q+1) sector ranks min(md, U{lo..hi}), then lowered to what the neighbouring bonds can feed
    (d(b, q) <= sum_n d(b - 1, q - n) and <= sum_n d(b + 1, q + n)) so that a generic state has them"""
    md = md_of(L, p, Q)
    d = np.minimum(md, rng.integers(lo, hi + 1, size=md.shape))
    d[0], d[L] = md[0], md[L]
    changed = True
    while changed:
        changed = False
        for b in range(1, L):
            for q in range(Q + 1):
                left = sum(d[b - 1, q - n] for n in range(p) if q - n >= 0)
                right = sum(d[b + 1, q + n] for n in range(p) if q + n <= Q)
                v = min(d[b, q], left, right)
                changed |= v != d[b, q]
                d[b, q] = v
    return d.astype(np.int32)


def _gauss(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def canonical_state(rng, L, p, Q, lo, hi):
    """(dims, data, dense): a complex right-canonical state with its centre at site 1 (what BH_tDMRG::step
    assumes) of sector ranks draw_ranks(rng, ...).  Every site gets orthonormal block rows by QR, the
    normalised dense vector goes back through ed.mps_from_full, and dense is re-expanded from the returned
    MPS: the reference sees exactly the device's input."""
    d = draw_ranks(rng, L, p, Q, lo, hi)
    data = []
    for k in range(1, L + 1):
        blocks = {}
        for q in range(Q + 1):
            ns = [n for n in range(p) if q + n <= Q and d[k, q + n] > 0]
            r, c = int(d[k - 1, q]), int(sum(d[k, q + n] for n in ns))
            if r == 0 or c == 0:
                continue
            assert r <= c
            Qm, _ = np.linalg.qr(_gauss(rng, (c, r)))
            row, off = Qm.conj().T, 0
            for n in ns:
                blocks[(q, n)] = row[:, off:off + d[k, q + n]]
                off += d[k, q + n]
        for q in range(Q + 1):
            for n in range(p):
                if q + n <= Q and d[k - 1, q] > 0 and d[k, q + n] > 0:
                    data.append(np.ascontiguousarray(blocks[(q, n)]).ravel())
    full = ed.full_from_mps(d, np.concatenate(data), L, p, Q)
    dims, dat = ed.mps_from_full(full / np.linalg.norm(full), L, p, Q, rel_cut=1e-30)
    return dims, dat, ed.full_from_mps(dims, dat, L, p, Q)


@functools.lru_cache(maxsize=None)
def case_state(name):
    """(drawn ranks, dims, data, dense) of a named case, computed once and shared (do not modify)"""
    L, p, Q, lo, hi, seed, _ = STEP_CASES[name]
    drawn = draw_ranks(np.random.default_rng(seed), L, p, Q, lo, hi)
    return (drawn,) + canonical_state(np.random.default_rng(seed), L, p, Q, lo, hi)


def case_shape(name):
    return STEP_CASES[name][:3]


def case_controls(name):
    """steps + 1 controls in [2, 10]"""
    L, p, Q, _, _, seed, steps = STEP_CASES[name]
    return np.random.default_rng(1000 + seed).uniform(2.0, 10.0, steps + 1)


def theta_census(dims, L, p, Q):
    """[(m, n, k)] of the Theta = A(i1) A(i1 + 1) products of the odd-bond gates (the first pass of a step,
    whose operands are the input's own tensors): per gate (i1, i1 + 1), centre sector q and right
    occupation n2, m = sum_n d(i1 - 1, q - n), n = d(i1 + 1, q + n2), k = d(i1, q)"""
    d = np.asarray(dims).reshape(L + 1, Q + 1)
    out = []
    for i1 in range(1, L, 2):
        for q in range(Q + 1):
            k = int(d[i1, q])
            m = int(sum(d[i1 - 1, q - n] for n in range(p) if q - n >= 0))
            for n2 in range(p):
                if q + n2 <= Q and k > 0 and m > 0 and d[i1 + 1, q + n2] > 0:
                    out.append((m, int(d[i1 + 1, q + n2]), k))
    return out


MN_CLASSES = [(1, 1), (2, 15), (16, 16), (17, 31), (32, 32), (33, 1 << 30)]


def census_gaps(census):
    """what the census condition misses (empty: met): m and n each in every class of MN_CLASSES (the 16-
    and 32-edges of k_gemm's tiles), k in {1, not a multiple of 4, 16, 17, 32, 33} (its k-steps of 4 in
    chunks of 16)"""
    gaps = []
    for name, col in (("m", 0), ("n", 1)):
        vals = {c[col] for c in census}
        gaps += [f"{name} in {lo}..{hi}" for lo, hi in MN_CLASSES if not any(lo <= v <= hi for v in vals)]
    ks = {c[2] for c in census}
    gaps += [f"k = {v}" for v in (1, 16, 17, 32, 33) if v not in ks]
    if not any(v % 4 for v in ks if v > 1):
        gaps.append("k not a multiple of 4")
    return gaps


# ------------------------------------------------------------------------------------ dense references
def dense_steps(psi, shape, u, forward=True):
    L, p, _ = shape
    for s in range(len(u) - 1):
        psi = ed.exact_step(psi, L, p, J, DT, u[s], u[s + 1], forward)
    return psi


def dense_overlap(x, y, shape, with_dH=False):
    return np.vdot(x, ed.dH_full(shape[0], shape[1]) * y) if with_dH else np.vdot(x, y)


def dense_apply_dH(psi, shape):
    """dH |psi>, not normalised (the oracle's convention)"""
    return ed.dH_full(shape[0], shape[1]) * psi


def dense_of(m):
    return ed.full_from_mps(m.dims, m.data, m.L, m.p, m.Q)


def deviation(ref, w):
    """(| |<ref|w>| - 1 |, max |w - ref <ref|w>|) of two normalised vectors: the second is the residual
    after the phase is removed"""
    ov = np.vdot(ref, w)
    return abs(abs(ov) - 1.0), float(np.abs(w - ref * ov).max())


def schmidt_ranks(psi, shape, weight=RANK_WEIGHT):
    """(ranks, above, below): the (L+1, Q+1) number of Schmidt weights above `weight` (of a total of 1) per
    bond sector of a dense vector, the smallest weight counted and the largest not counted.  With
    above >= RANK_ABOVE and below <= RANK_BELOW a truncation at CUTOFF has nothing to decide: every weight
    is a thousand times above the cutoff or rounding noise, and the ranks are the bond dimensions of any
    correct step."""
    L, p, Q = shape
    r = np.zeros((L + 1, Q + 1), np.int32)
    r[0, 0] = r[L, Q] = 1
    below, above = 0.0, np.inf
    for b in range(1, L):
        M = psi.reshape(p ** b, p ** (L - b))
        ql, qr = ed.counts(b, p), ed.counts(L - b, p)
        for q in range(Q + 1):
            R, C = np.where(ql == q)[0], np.where(qr == Q - q)[0]
            if len(R) == 0 or len(C) == 0:
                continue
            s2 = np.linalg.svd(M[np.ix_(R, C)], compute_uv=False) ** 2
            r[b, q] = int((s2 > weight).sum())
            below = max(below, float(s2[r[b, q]:].max(initial=0.0)))
            above = min(above, float(s2[:r[b, q]].min(initial=np.inf)))
    return r, above, below


def scaled(dims, data, shape, a):
    """data of a |state>: site 1's blocks (the first sum_n d(1, n) elements) times the complex a"""
    L, p, Q = shape
    n1 = int(np.asarray(dims).reshape(L + 1, Q + 1)[1, :p].sum())
    out = np.array(data, dtype=np.complex128)
    out[:n1] *= a
    return out


def clipped_random_mps(rng, L, p, Q, lo, hi):
    """(dims, data): spectrum_reference.random_mps (complex Gaussian blocks, neither canonical nor
    normalised) with every sector clipped to its bound md, which the chain engines require"""
    d = np.minimum(md_of(L, p, Q), rng.integers(lo, hi + 1, size=(L + 1, Q + 1))).astype(np.int32)
    return d.reshape(-1), _gauss(rng, ed.nelem(d, L, p, Q)) / np.sqrt(2.0 * max(lo, 1) * p)
