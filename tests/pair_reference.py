"""Reference for ocg_observe_pairs / ocg_observe_pairs_states: the transition matrix
elements between a bra x and a ket y in the compact U(1) block format,

    ovl = <x|y>,   occ[k][n] = <x|P_k(n)|y>   (P_k(n) the projector on occupation n of site k),
    hop[b][0] = <x|a+_b a_{b+1}|y>,   hop[b][1] = <x|a_b a+_{b+1}|y>   (a, a+ cut at p levels).

`pairs_ref` restates the block contraction of include/ocmps.h in numpy: rectangular
left and right environments (block q is d_x[b][q] x d_y[b][q]) and, for the hopping
terms, an environment opened at site b and closed at site b + 1.  `pairs_dense` takes
the same numbers from the full state vectors and explicit site operators;
tests/test_pair_reference.py pins the first against the second.
"""
import numpy as np

import observe_reference as R
from optimalcontrolmps_amd import ed


def _blocks(dims, data, L, p, Q):
    dims = np.asarray(dims).reshape(L + 1, Q + 1)
    return {(k, q, n): b for k, q, n, b in ed.mps_blocks(dims, np.asarray(data, np.complex128), L, p, Q)}


def pairs_ref(dims_x, x, dims_y, y, L, p, Q):
    """dict(ovl complex, occ (L, p) complex, hop (L-1, 2) complex) of the pair (bra x, ket y)"""
    AX, AY = _blocks(dims_x, x, L, p, Q), _blocks(dims_y, y, L, p, Q)
    # right environments N_b[q] (d_x x d_y): N_{k-1}[q] = sum_n conj(Ax(q, n)) N_k[q + n] Ay(q, n)^T
    N = [dict() for _ in range(L + 1)]
    N[L][Q] = np.ones((1, 1), complex)
    for k in range(L, 0, -1):
        for (kk, q, n), ax in AX.items():
            ay = AY.get((kk, q, n))
            if kk != k or ay is None or q + n not in N[k]:
                continue
            N[k - 1][q] = N[k - 1].get(q, 0) + ax.conj() @ N[k][q + n] @ ay.T
    occ = np.zeros((L, p), complex)
    hop = np.zeros((max(L - 1, 0), 2), complex)
    Lenv = {0: np.ones((1, 1), complex)}
    C, G = {}, {}  # opened at the site before, by ket sector: a+ placed (bra one above), a placed (bra one below)
    for k in range(1, L + 1):
        Ln, Cn, Gn = {}, {}, {}
        for (kk, q, n), ay in AY.items():
            if kk != k:
                continue
            right = N[k].get(q + n)
            if q in Lenv:
                t = Lenv[q] @ ay
                ax = AX.get((k, q, n))
                if ax is not None:
                    Ln[q + n] = Ln.get(q + n, 0) + ax.conj().T @ t
                    if right is not None:
                        occ[k - 1, n] += np.sum(ax.conj().T @ t * right)
                up, dn = AX.get((k, q, n + 1)), AX.get((k, q, n - 1))
                if up is not None:  # <n + 1|a+|n>
                    Cn[q + n] = Cn.get(q + n, 0) + np.sqrt(n + 1.0) * up.conj().T @ t
                if dn is not None:  # <n - 1|a|n>
                    Gn[q + n] = Gn.get(q + n, 0) + np.sqrt(float(n)) * dn.conj().T @ t
            if right is None or k == 1:
                continue
            ax = AX.get((k, q + 1, n - 1))  # a here after a+ on the site before
            if q in C and ax is not None:
                hop[k - 2, 0] += np.sqrt(float(n)) * np.sum(ax.conj().T @ C[q] @ ay * right)
            ax = AX.get((k, q - 1, n + 1))  # a+ here after a on the site before
            if q in G and ax is not None:
                hop[k - 2, 1] += np.sqrt(n + 1.0) * np.sum(ax.conj().T @ G[q] @ ay * right)
        Lenv, C, G = Ln, Cn, Gn
    ovl = complex(Lenv[Q][0, 0]) if Q in Lenv else 0j
    return {"ovl": ovl, "occ": occ, "hop": hop}


def pairs_dense(vx, vy, L, p):
    """the same dict from the full state vectors (site 1 the slowest index) and explicit operators"""
    vx, vy = np.asarray(vx, np.complex128), np.asarray(vy, np.complex128)
    A, Ad = R._op(p, "A"), R._op(p, "Adag")
    occ = np.zeros((L, p), complex)
    for k in range(1, L + 1):
        for n in range(p):
            P = np.zeros((p, p))
            P[n, n] = 1.0
            occ[k - 1, n] = np.vdot(vx, R._apply(vy, P, k, L, p))
    hop = np.zeros((max(L - 1, 0), 2), complex)
    for b in range(1, L):
        hop[b - 1, 0] = np.vdot(vx, R._apply(R._apply(vy, A, b + 1, L, p), Ad, b, L, p))
        hop[b - 1, 1] = np.vdot(vx, R._apply(R._apply(vy, Ad, b + 1, L, p), A, b, L, p))
    return {"ovl": complex(np.vdot(vx, vy)), "occ": occ, "hop": hop}


def pairs_of_mps(dims_x, x, dims_y, y, L, p, Q):
    return pairs_dense(ed.full_from_mps(dims_x, x, L, p, Q), ed.full_from_mps(dims_y, y, L, p, Q), L, p)


def norm_of(dims, data, L, p, Q):
    """sqrt(<s|s>) by the block contraction"""
    return float(np.sqrt(abs(pairs_ref(dims, data, dims, data, L, p, Q)["ovl"])))


def deviation(got, ref, p, scale):
    """the largest deviation of a pair's outputs in units of their tolerance scale: scale = sqrt(<x|x><y|y>)
    times 1 for ovl and occ, p - 1 (the largest |<m|a+ a|n>|) for hop"""
    dev = max(abs(complex(got["ovl"]) - ref["ovl"]), float(np.abs(np.asarray(got["occ"]) - ref["occ"]).max()))
    if ref["hop"].size:
        dev = max(dev, float(np.abs(np.asarray(got["hop"]) - ref["hop"]).max()) / max(p - 1, 1))
    return dev / scale


def drop_sector(dims, data, L, p, Q, b, q):
    """(dims, data) of the state without sector q of bond b (its blocks removed)"""
    dims = np.asarray(dims).reshape(L + 1, Q + 1)
    nd = dims.copy()
    nd[b, q] = 0
    keep = [blk.reshape(-1) for k, qq, n, blk in ed.mps_blocks(dims, np.asarray(data, np.complex128), L, p, Q)
            if not (k == b and qq + n == q) and not (k == b + 1 and qq == q)]
    return nd.reshape(-1), np.concatenate(keep)
