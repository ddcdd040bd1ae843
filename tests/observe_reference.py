"""Reference for ocg_observe / ocg_observe_states.

`observe_ref` restates the definitions of include/ocmps.h (ocg_observe) over
the compact U(1) blocks in numpy: left / right environments, the occupation
distribution per site, and the correlation rows <a+_i a_j>, <n_i n_j> from a
start site with the bra one sector above the ket.  `observe_dense` computes the
same numbers from the full p**L state vector (operators applied site by site);
tests/test_observe_reference.py pins the first against the second.
"""
import numpy as np

from optimalcontrolmps_amd import ed


def blocks_of(dims, data, L, p, Q):
    return {(k, q, n): b for k, q, n, b in ed.mps_blocks(dims, data, L, p, Q)}


def observe_ref(dims, data, L, p, Q, rows=()):
    """dict(norm2, occ (L, p), bond (L+1,), ada (nrows, L) complex, nn (nrows, L))"""
    dims = np.asarray(dims).reshape(L + 1, Q + 1)
    A = blocks_of(dims, np.asarray(data, np.complex128), L, p, Q)
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
    norm2 = float(np.real(Lenv[L][Q][0, 0])) if Q in Lenv[L] else 0.0
    occ = np.zeros((L, p))
    for (k, q, n), a in A.items():
        if q in Lenv[k - 1] and q + n in Renv[k]:
            occ[k - 1, n] += np.real(np.trace(a.conj().T @ Lenv[k - 1][q] @ a @ Renv[k][q + n]))
    nvec = np.arange(p)
    ada = np.zeros((len(rows), L), complex)
    nn = np.zeros((len(rows), L))
    for ri, i in enumerate(rows):
        ada[ri, i - 1] = (nvec * occ[i - 1]).sum()
        nn[ri, i - 1] = (nvec ** 2 * occ[i - 1]).sum()
        C, N = {}, {}
        for (k, q, n), a in A.items():          # open at site i
            if k != i or q not in Lenv[i - 1]:
                continue
            if (i, q, n + 1) in A:
                C[q + n] = C.get(q + n, 0) + np.sqrt(n + 1) * A[(i, q, n + 1)].conj().T @ Lenv[i - 1][q] @ a
            if n:
                N[q + n] = N.get(q + n, 0) + n * a.conj().T @ Lenv[i - 1][q] @ a
        for j in range(i + 1, L + 1):
            va, vn = 0.0, 0.0
            for (k, s, n), a in A.items():      # close at site j
                if k != j or s + n not in Renv[j]:
                    continue
                if n >= 1 and s in C and (j, s + 1, n - 1) in A:
                    va += np.sqrt(n) * np.trace(A[(j, s + 1, n - 1)].conj().T @ C[s] @ a @ Renv[j][s + n])
                if n >= 1 and s in N:
                    vn += n * np.real(np.trace(a.conj().T @ N[s] @ a @ Renv[j][s + n]))
            ada[ri, j - 1] = va
            nn[ri, j - 1] = vn
            C2, N2 = {}, {}
            for (k, s, n), a in A.items():      # transfer through site j
                if k != j:
                    continue
                if s in C and (j, s + 1, n) in A:
                    C2[s + n] = C2.get(s + n, 0) + A[(j, s + 1, n)].conj().T @ C[s] @ a
                if s in N:
                    N2[s + n] = N2.get(s + n, 0) + a.conj().T @ N[s] @ a
            C, N = C2, N2
    return {"norm2": norm2, "occ": occ, "bond": dims.sum(axis=1), "ada": ada, "nn": nn}


def _op(p, name):
    O = np.zeros((p, p))
    j = np.arange(p)
    if name == "N":
        O[j, j] = j
    elif name == "A":
        O[j[:-1], j[1:]] = np.sqrt(j[1:])
    elif name == "Adag":
        O[j[1:], j[:-1]] = np.sqrt(j[1:])
    return O


def _apply(psi, O, site, L, p):
    T = psi.reshape((p,) * L)
    return np.moveaxis(np.tensordot(O, T, axes=([1], [site - 1])), 0, site - 1).reshape(-1)


def observe_dense(psi, L, p, rows=()):
    """the same dict (without bond) from the full state vector"""
    T = np.abs(psi.reshape((p,) * L)) ** 2
    occ = np.array([T.sum(axis=tuple(a for a in range(L) if a != k)) for k in range(L)])
    ada = np.zeros((len(rows), L), complex)
    nn = np.zeros((len(rows), L))
    Nop, Aop, Adop = _op(p, "N"), _op(p, "A"), _op(p, "Adag")
    for ri, i in enumerate(rows):
        for j in range(i, L + 1):
            ada[ri, j - 1] = np.vdot(psi, _apply(_apply(psi, Aop, j, L, p), Adop, i, L, p))
            nn[ri, j - 1] = np.vdot(psi, _apply(_apply(psi, Nop, j, L, p), Nop, i, L, p)).real
        ada[ri, i - 1] = ada[ri, i - 1].real
    return {"norm2": float(np.vdot(psi, psi).real), "occ": occ, "ada": ada, "nn": nn}


def dense_of(m):
    """full state vector of a native.MPS"""
    return ed.full_from_mps(m.dims, m.data, m.L, m.p, m.Q)


def max_dev(got, ref, keys=("norm2", "occ", "ada", "nn")):
    return max(float(np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max()) for k in keys
               if np.asarray(ref[k]).size)


def fock(L, p, Q, occ):
    """(dims, data) of the Fock state |occ_1 ... occ_L> (every block 1 x 1)"""
    assert sum(occ) == Q and max(occ) < p
    dims = np.zeros((L + 1, Q + 1), np.int32)
    q = 0
    dims[0, 0] = 1
    for k, n in enumerate(occ, 1):
        q += n
        dims[k, q] = 1
    return dims.reshape(-1), np.ones(L, np.complex128)
