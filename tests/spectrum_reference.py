"""Reference for ocg_observe_spectrum / ocg_observe_spectrum_states.

`spectrum_ref` restates the block formula of include/ocmps.h in numpy over the
compact U(1) blocks: with the environments of observe_reference.py
(Lenv_k[q'] = sum A^H Lenv_{k-1} A, Renv_{k-1}[q] = sum A Renv_k A^H) the
Schmidt weights of bond b in sector q are the eigenvalues of
X = S^H Renv_b[q] S, S = V diag(sqrt(max(lambda, 0))), Lenv_b[q] = V diag(lambda) V^H
(no conjugate on Renv).  `spectrum_dense` takes the same weights from the
singular values of the full p**L state vector; tests/test_spectrum_reference.py
pins the first against the second.
"""
import numpy as np

from optimalcontrolmps_amd import ed


def entropy_of(w):
    """the reference's rule: clamp at 0, p = w / sum w, S = -sum_{p > 1e-12} p ln p (0 for a zero state)"""
    w = np.maximum(np.asarray(w, float), 0.0)
    tot = w.sum()
    if tot == 0:
        return 0.0
    p = w / tot
    p = p[p > 1e-12]
    return float(-(p * np.log(p)).sum())


def envs(dims, data, L, p, Q):
    dims = np.asarray(dims).reshape(L + 1, Q + 1)
    A = {(k, q, n): b for k, q, n, b in ed.mps_blocks(dims, np.asarray(data, np.complex128), L, p, Q)}
    Lenv = [dict() for _ in range(L + 1)]
    Renv = [dict() for _ in range(L + 1)]
    Lenv[0][0] = np.ones((1, 1), complex)
    Renv[L][Q] = np.ones((1, 1), complex)
    for k in range(1, L + 1):
        for (kk, q, n), a in A.items():
            if kk == k and q in Lenv[k - 1]:
                Lenv[k][q + n] = Lenv[k].get(q + n, 0) + a.conj().T @ Lenv[k - 1][q] @ a
    for k in range(L, 0, -1):
        for (kk, q, n), a in A.items():
            if kk == k and q + n in Renv[k]:
                Renv[k - 1][q] = Renv[k - 1].get(q, 0) + a @ Renv[k][q + n] @ a.conj().T
    return dims, Lenv, Renv


def spectrum_ref(dims, data, L, p, Q, conj_renv=False):
    """dict(weights, sectors: lists over the bonds b = 1..L-1 of arrays of length bond[b], weights
    descending with ties by sector ascending; entropy (L-1,); norm2).  conj_renv=True is the wrong
    formula (the conjugated right environment), kept so that a test can show it to be wrong."""
    dims, Lenv, Renv = envs(dims, data, L, p, Q)
    weights, sectors, entropy = [], [], np.zeros(L - 1)
    for b in range(1, L):
        w, s = [], []
        for q in range(Q + 1):
            d = int(dims[b, q])
            if d == 0:
                continue
            if q in Lenv[b] and q in Renv[b]:
                lam, V = np.linalg.eigh(Lenv[b][q])
                S = V * np.sqrt(np.maximum(lam, 0.0))
                R = Renv[b][q].conj() if conj_renv else Renv[b][q]
                X = S.conj().T @ R @ S
                w.extend(np.linalg.eigvalsh(0.5 * (X + X.conj().T)))
            else:
                w.extend([0.0] * d)
            s.extend([q] * d)
        w, s = np.array(w, float), np.array(s, np.int32)
        o = np.lexsort((s, -w))
        weights.append(w[o])
        sectors.append(s[o])
        entropy[b - 1] = entropy_of(w)
    norm2 = float(np.real(Lenv[L][Q][0, 0])) if Q in Lenv[L] else 0.0
    return {"weights": weights, "sectors": sectors, "entropy": entropy, "norm2": norm2}


def spectrum_dense(psi, L, p):
    """dict(weights: per bond the squared singular values of psi.reshape(p**b, -1), descending (site 1
    is the slowest index, as ed.full_from_mps produces); entropy (L-1,); norm2)"""
    psi = np.asarray(psi, np.complex128)
    weights = [np.linalg.svd(psi.reshape(p ** b, -1), compute_uv=False) ** 2 for b in range(1, L)]
    return {"weights": weights, "entropy": np.array([entropy_of(w) for w in weights]),
            "norm2": float(np.vdot(psi, psi).real)}


def weight_dev(a, b):
    """largest deviation between two descending weight lists of one bond (the shorter padded with 0)"""
    n = max(len(a), len(b))
    x, y = np.zeros(n), np.zeros(n)
    x[:len(a)] = a
    y[:len(b)] = b
    return float(np.abs(x - y).max()) if n else 0.0


def padded(ref, wcap):
    """(schmidt (L-1, wcap), sector (L-1, wcap)) of a spectrum_ref result in ocg_observe_spectrum's layout"""
    nb = len(ref["weights"])
    w, s = np.zeros((nb, wcap)), np.full((nb, wcap), -1, np.int32)
    for b in range(nb):
        n = len(ref["weights"][b])
        w[b, :n] = ref["weights"][b]
        s[b, :n] = ref["sectors"][b]
    return w, s


def reachable(L, p, Q):
    """bool (L+1, Q+1): sector q of bond b can be reached from both ends"""
    ok = np.zeros((L + 1, Q + 1), bool)
    for b in range(L + 1):
        for q in range(Q + 1):
            ok[b, q] = q <= b * (p - 1) and Q - q <= (L - b) * (p - 1)
    return ok


def random_mps(rng, L, p, Q, lo, hi):
    """(dims, data): complex Gaussian blocks, every reachable bond sector of a size in lo..hi (the ends
    are one state); neither canonical nor normalised"""
    dims = np.zeros((L + 1, Q + 1), np.int32)
    ok = reachable(L, p, Q)
    for b in range(1, L):
        for q in range(Q + 1):
            if ok[b, q]:
                dims[b, q] = rng.integers(lo, hi + 1)
    dims[0, 0] = 1
    dims[L, Q] = 1
    n = ed.nelem(dims, L, p, Q)
    data = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0 * max(lo, 1) * p)
    return dims.reshape(-1), data


def pad_sector(dims, data, L, p, Q, b, q):
    """(dims, data) of the same state with sector q of bond b enlarged by one all-zero state"""
    dims = np.asarray(dims).reshape(L + 1, Q + 1)
    nd = dims.copy()
    nd[b, q] += 1
    out = []
    for k, qq, n, blk in ed.mps_blocks(dims, np.asarray(data, np.complex128), L, p, Q):
        if k == b and qq + n == q:
            blk = np.concatenate([blk, np.zeros((blk.shape[0], 1), complex)], axis=1)
        if k == b + 1 and qq == q:
            blk = np.concatenate([blk, np.zeros((1, blk.shape[1]), complex)], axis=0)
        out.append(blk.reshape(-1))
    # blocks that only exist because the sector is now non-empty
    full = []
    it = iter(out)
    have = {(k, qq, n) for k, qq, n, _ in ed.mps_blocks(dims, np.asarray(data, np.complex128), L, p, Q)}
    for k in range(1, L + 1):
        for qq in range(Q + 1):
            for n in range(p):
                if qq + n > Q:
                    continue
                r, c = int(nd[k - 1, qq]), int(nd[k, qq + n])
                if r == 0 or c == 0:
                    continue
                full.append(next(it) if (k, qq, n) in have else np.zeros(r * c, complex))
    return nd.reshape(-1), np.concatenate(full)
