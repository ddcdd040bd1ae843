"""Reference for ocg_observe_strings / ocg_observe_strings_states: the expectation of a product of
diagonal one-site operators, O = (x)_k F_k with F_k = sum_n f[k-1][n] P_k(n), in the compact U(1)
block format.

`strings_ref` restates the formulas of include/ocmps.h in numpy: the support [a, b] runs from the first to
the last site whose table is not exactly 1 for every n; an empty support gives norm2; otherwise

    E_{a-1}[q] = Lenv_{a-1}[q]
    E_k[q+n]  += f[k][n] A_k(q,n)^H E_{k-1}[q] A_k(q,n)       k = a..b
    out        = sum_q sum E_b[q] o Renv_b[q]^T

with the environments of spectrum_reference.envs.  `strings_dense` takes the same numbers from the full
state vector, sum over the Fock configurations of |amp|^2 prod_k f[k][n_k];
tests/test_string_reference.py pins the first against the second.
"""
import numpy as np

import spectrum_reference as S
from optimalcontrolmps_amd import ed


def support(f):
    """(a, b), 1-based and inclusive, of one table f (L, p); None when it is empty"""
    sites = [k for k in range(1, len(f) + 1) if not np.all(f[k - 1] == 1)]
    return (sites[0], sites[-1]) if sites else None


def strings_ref(dims, data, L, p, Q, f):
    """complex (nops,) = <s|O_m|s> (raw) for the tables f (nops, L, p)"""
    f = np.asarray(f, np.complex128).reshape(-1, L, p)
    dims, Lenv, Renv = S.envs(dims, data, L, p, Q)
    A = {(k, q, n): b for k, q, n, b in ed.mps_blocks(dims, np.asarray(data, np.complex128), L, p, Q)}
    out = np.zeros(len(f), complex)
    for m, fm in enumerate(f):
        sup = support(fm)
        if sup is None:
            out[m] = Lenv[L][Q][0, 0] if Q in Lenv[L] else 0.0
            continue
        a, b = sup
        E = dict(Lenv[a - 1])
        for k in range(a, b + 1):
            En = {}
            for (kk, q, n), blk in A.items():
                if kk == k and q in E:
                    En[q + n] = En.get(q + n, 0) + fm[k - 1, n] * (blk.conj().T @ E[q] @ blk)
            E = En
        out[m] = sum(np.sum(E[q] * Renv[b][q].T) for q in E if q in Renv[b])
    return out


def strings_dense(psi, L, p, f):
    """the same from the full state vector (site 1 the slowest index)"""
    f = np.asarray(f, np.complex128).reshape(-1, L, p)
    T = np.abs(np.asarray(psi).reshape((p,) * L)) ** 2
    out = np.zeros(len(f), complex)
    for m, fm in enumerate(f):
        W = T.astype(complex)
        for k in range(L):
            W = W * fm[k].reshape((1,) * k + (p,) + (1,) * (L - 1 - k))
        out[m] = W.sum()
    return out


def scale(norm2, f):
    """the tolerance scale of every operator: norm2 prod_k max_n |f[k][n]|"""
    return norm2 * np.abs(np.asarray(f)).max(axis=-1).prod(axis=-1)


def identity(L, p, nops=1):
    return np.ones((nops, L, p), np.complex128)


def parity_tables(L, p, i, nbar):
    """the L - i + 1 operators prod_{k=i..j} (-1)^(n_k - nbar), j = i..L"""
    f = identity(L, p, L - i + 1)
    sign = (-1.0) ** (np.arange(p) - nbar)
    for m in range(len(f)):
        f[m, i - 1:i + m] = sign
    return f


def counting_tables(L, p, Q, i, j):
    """the Q + 1 operators exp(i theta_r N_A), theta_r = 2 pi r / (Q + 1), A the sites i..j"""
    f = identity(L, p, Q + 1)
    theta = 2 * np.pi * np.arange(Q + 1) / (Q + 1)
    f[:, i - 1:j, :] = np.exp(1j * theta[:, None, None] * np.arange(p)[None, None, :])
    return f


def counting_from(G, norm2, Q):
    """P(m), m = 0..Q, from the generating-function values G (..., Q + 1)"""
    theta = 2 * np.pi * np.arange(Q + 1) / (Q + 1)
    return (np.asarray(G) @ np.exp(-1j * np.outer(theta, np.arange(Q + 1)))).real / (Q + 1) / norm2
