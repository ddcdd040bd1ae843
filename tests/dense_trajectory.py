"""Inputs and the dense reference of the driver tests (test_dense_trajectory_reference.py on the CPU,
test_dense_trajectory_gpu.py on the device): trajectory cases built from dense_reference.canonical_state
draws, and getHessian(u) -- psi_t, xi_t, F, divT, the fidelities, the gradient and the Hessian with its two
terms -- from state vectors alone (numpy only).  It shares no convention of conjugation, normiH or index
pairing with the kernels or with the CPU oracle.  The constants, the state construction and the one-step
references are dense_reference.py's."""
import functools

import numpy as np

from dense_reference import DT, J, canonical_state, dense_steps
from optimalcontrolmps_amd import ed

# name -> (L, p, Q, lo, hi, seed, N_t, mix).  init is the canonical_state draw of `seed`.  The target is
# correlated with init so that neither term of the Hessian drowns the other (a random target has |F| of
# 4e-3 .. 0.2 and H is almost all B): target = normalise(dense_steps(init, u') + mix * a second
# canonical_state draw), taken back through ed.mps_from_full and re-expanded, u' = traj_controls(name,
# k=TARGET_K).  mix = 0: the target is the evolved init, of grown ranks, and u' has twice the steps of the
# trajectory: with as many, xi_0 = U(u)^-1 U(u') init comes back so close to init that its smallest Schmidt
# weights (2e-13) straddle the cutoff and the zip-up of dH xi_0 cuts into them (oracle-to-dense 4e-8 on
# that one stored state, 1e-14 on every scalar).
TARGET_K = 99
TRAJ_CASES = {
    "T_L5p5Q5": (5, 5, 5, 1 << 20, 1 << 20, 4, 9, 0.5),
    "T_L5p6Q5": (5, 6, 5, 1 << 20, 1 << 20, 5, 9, 0.5),
    "T_L4p4Q7": (4, 4, 7, 1 << 20, 1 << 20, 6, 6, 0.5),
    "T_L8p4Q8": (8, 4, 8, 1 << 20, 1 << 20, 8, 6, 0.5),
    "T_L9p3Q9": (9, 3, 9, 1 << 20, 1 << 20, 13, 7, 0.5),
    "T_L8p4Q8_r15_17": (8, 4, 8, 15, 17, 7, 6, 0.0),
}
TRAJ_FULL = [n for n, c in TRAJ_CASES.items() if c[3] == 1 << 20]
TRAJ_LDS = ["T_L5p5Q5", "T_L5p6Q5", "T_L4p4Q7"]
TRAJ_HBM = ["T_L8p4Q8", "T_L9p3Q9", "T_L8p4Q8_r15_17", "T_L5p5Q5"]


def traj_shape(name):
    return TRAJ_CASES[name][:3]


def traj_controls(name, n=None, k=0):
    """the k-th control vector of a case: n (default the case's N_t) controls in [2, 10]; different k give
    distinct vectors (the members of a multi-control call, a second call on one context)"""
    seed, nt = TRAJ_CASES[name][5:7]
    return np.random.default_rng(1000 + seed + 7919 * k).uniform(2.0, 10.0, nt if n is None else n)


@functools.lru_cache(maxsize=None)
def traj_states(name):
    """((dims, data, dense) of init, (dims, data, dense) of target), computed once and shared (do not
    modify); both dense vectors are re-expanded from the MPS the device gets"""
    L, p, Q, lo, hi, seed, nt, mix = TRAJ_CASES[name]
    shape = (L, p, Q)
    init = canonical_state(np.random.default_rng(seed), L, p, Q, lo, hi)
    full = dense_steps(init[2], shape, traj_controls(name, None if mix else 2 * nt - 1, TARGET_K))
    if mix:
        full = full + mix * canonical_state(np.random.default_rng(2000 + seed), L, p, Q, lo, hi)[2]
    dims, dat = ed.mps_from_full(full / np.linalg.norm(full), L, p, Q, rel_cut=1e-30)
    return init, (dims, dat, ed.full_from_mps(dims, dat, L, p, Q))


def dense_trajectory(init, target, shape, u):
    """getHessian(u) of the GRAPE cost 0.5 (1 - |<target|psi_{N-1}>|^2) without regularisation, from state
    vectors alone: a dict of
      psi, xi   (N, dim)  psi_0 = init, psi_{i+1} = U(u_i -> u_{i+1}) psi_i;  xi_{N-1} = target,
                          xi_{i-1} = U^-1(u_i -> u_{i-1}) xi_i
      F                   <psi_{N-1}|target>
      divT      (N,)      <xi_i|dH|psi_i>
      fid       (N,)      |<target|psi_t>|^2
      grad      (N,)      dt Re(i divT_i F)
      xiH_norm  (N,)      |dH xi_t|
      A, B, H   (N, N)    H = A + B;  for 1 <= i <= j <= N-2, phi = dH psi_i (not normalised), n = |phi|:
                          A_ii = dt^2 Re(F <dH xi_i|phi>),  A_ij = A_ji = dt^2 Re(F n <dH xi_j|phi_j>) with
                          phi_j = U(u_{j-1} -> u_j) ... U(u_i -> u_{i+1}) phi / n;
                          B_ij = -dt^2 Re(divT_i conj divT_j).  Rows and columns 0 and N-1 are 0.
    ed.exact_step normalises its output, which is why n is multiplied back in."""
    L, p, _ = shape
    N = len(u)
    dH = ed.dH_full(L, p)
    psi, xi = [init], [target]
    for i in range(N - 1):
        psi.append(ed.exact_step(psi[-1], L, p, J, DT, u[i], u[i + 1], True))
    for i in range(N - 1, 0, -1):
        xi.insert(0, ed.exact_step(xi[0], L, p, J, DT, u[i], u[i - 1], False))
    psi, xi = np.array(psi), np.array(xi)
    F = np.vdot(psi[-1], target)
    divT = np.array([np.vdot(xi[i], dH * psi[i]) for i in range(N)])
    fid = np.array([abs(np.vdot(target, s)) ** 2 for s in psi])
    xiH = dH * xi
    A, B = np.zeros((N, N)), np.zeros((N, N))
    for i in range(1, N - 1):
        phi = dH * psi[i]
        n = np.linalg.norm(phi)
        A[i, i] = DT * DT * (F * np.vdot(xiH[i], phi)).real
        phi = phi / n
        for j in range(i + 1, N - 1):
            phi = ed.exact_step(phi, L, p, J, DT, u[j - 1], u[j], True)
            A[i, j] = A[j, i] = DT * DT * (F * n * np.vdot(xiH[j], phi)).real
        for j in range(1, N - 1):
            B[i, j] = -DT * DT * (divT[i] * np.conj(divT[j])).real
    return {"psi": psi, "xi": xi, "F": F, "divT": divT, "fid": fid, "grad": DT * (1j * divT * F).real,
            "xiH_norm": np.linalg.norm(xiH, axis=1), "A": A, "B": B, "H": A + B}


def raw_step(psi, shape, u_from, u_to):
    """one forward step by the gate sequence of BH_tDMRG::step, not normalised (its own copy of the
    sequence: the second opinion of dense_hessian_raw)"""
    L, p, _ = shape
    n = np.arange(p)
    site = lambda k, v: v.reshape([p if s == k else 1 for s in range(L)])
    G = ed.hop_gate(p, J, DT).reshape(p, p, p, p)
    T = psi.reshape((p,) * L)
    for k in range(L):
        T = T * site(k, np.exp(-0.25j * u_from * DT * n * (n - 1)))
    for a, b in ed.gate_list(L):
        T = np.moveaxis(np.tensordot(G, T, axes=([2, 3], [a - 1, b - 1])), [0, 1], [a - 1, b - 1])
    for k in range(L):
        T = T * site(k, np.exp(-0.25j * u_to * DT * n * (n - 1)))
    return T.reshape(-1)


def dense_hessian_raw(ref, shape, u):
    """H of dense_trajectory computed another way: the row state dH psi_i carried unnormalised by raw_step,
    columns first, the two terms summed entry by entry (psi, xi, divT and F are taken from ref)"""
    N = len(u)
    dH = ed.dH_full(shape[0], shape[1])
    H = np.zeros((N, N))
    for i in range(N - 2, 0, -1):
        phi = dH * ref["psi"][i]
        for j in range(i, N - 1):
            if j > i:
                phi = raw_step(phi, shape, u[j - 1], u[j])
            v = DT * DT * ((ref["F"] * np.vdot(dH * ref["xi"][j], phi)).real
                           - (ref["divT"][i] * np.conj(ref["divT"][j])).real)
            H[i, j] = H[j, i] = v
    return H


@functools.lru_cache(maxsize=None)
def traj_reference(name, n=None, k=0):
    """dense_trajectory of a case at traj_controls(name, n, k), computed once and shared (do not modify)"""
    (_, _, init), (_, _, target) = traj_states(name)
    return dense_trajectory(init, target, traj_shape(name), traj_controls(name, n, k))


def hessian_scale(ref):
    """S = max|A| + max|B|: the two terms cancel (tenfold on these cases), so deviations of H are stated
    against the terms' scale"""
    return float(np.abs(ref["A"]).max() + np.abs(ref["B"]).max())
