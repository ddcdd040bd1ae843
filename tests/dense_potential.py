"""Inputs and references of the static site potential sum_k eps_k n_k (DESIGN.md section 15;
test_dense_potential_reference.py on the CPU, test_potential_gpu.py on the device).

Dense: dense_trajectory.dense_trajectory restated with ed.exact_step(..., eps=...), plus the sensitivities
s[t, k] = dt Re(i <xi_t|n_k|psi_t> F) of the cost to a site potential (numpy only).

Oracle-composed: the CPU oracle knows no potential and stays as it is.  One trapped step is E step_0 E with
E = prod_k exp(-i tau eps_k n_k / 2), diagonal in the physical indices, so it is applied exactly to the
compact blocks of an MPS (e_pass) around the oracle's own Stepper.step; getHessian is formed from these steps,
the oracle's apply_dH and its overlaps by the reference's calcHessianRow.  This second CPU reference truncates
like the engines do, and its distance from dense sets the device bounds.

The states and controls are dense_trajectory.TRAJ_CASES'; the potential of a case is
eps_k = 0.35 (k - (L+1)/2)^2 + 0.6 k + r_k, r uniform in [-1, 1] from the case's seed: a trap, a tilt and
disorder, asymmetric, no two sites equal.  A steep case replaces eps_2 by 400: its half-phase argument
tau eps n / 2 reaches 10, far outside the range of the engines' short sine / cosine series."""
import functools

import numpy as np

import dense_reference as D
import dense_trajectory as T
from optimalcontrolmps_amd import ed

# name -> (trajectory case, seed of r, steep)
POT_CASES = {
    "T_L5p5Q5": ("T_L5p5Q5", 31, False),
    "T_L4p4Q7": ("T_L4p4Q7", 32, False),
    "T_L5p6Q5": ("T_L5p6Q5", 33, False),
    "T_L8p4Q8": ("T_L8p4Q8", 34, False),
    "T_L9p3Q9": ("T_L9p3Q9", 35, False),
    "T_L5p5Q5_steep": ("T_L5p5Q5", 31, True),
    "T_L9p3Q9_steep": ("T_L9p3Q9", 35, True),
}
POT_LDS = ["T_L5p5Q5", "T_L4p4Q7", "T_L5p6Q5"]
POT_HBM = ["T_L8p4Q8", "T_L9p3Q9", "T_L5p5Q5"]
STEEP = 400.0
FD_H = 1e-4
KEYS = ["F", "H", "divT", "fid", "sens", "state"]


def traj_of(name):
    return POT_CASES[name][0]


def potential(name):
    traj, seed, steep = POT_CASES[name]
    L = T.traj_shape(traj)[0]
    k = np.arange(1, L + 1)
    eps = 0.35 * (k - (L + 1) / 2) ** 2 + 0.6 * k + np.random.default_rng(seed).uniform(-1.0, 1.0, L)
    if steep:
        eps[1] = STEEP
    return eps


def site_occupations(x, y, shape):
    """<x|n_k|y>, k = 1..L, of two dense vectors"""
    L, p, _ = shape
    g = np.indices((p,) * L).reshape(L, -1)
    return np.array([np.vdot(x, g[k] * y) for k in range(L)])


def sensitivities(psi, xi, F, shape):
    """s[t, k] = dt Re(i <xi_t|n_k|psi_t> F) and the raw matrix elements"""
    nk = np.array([site_occupations(xi[t], psi[t], shape) for t in range(len(psi))])
    return D.DT * (1j * nk * F).real, nk


def dense_trajectory(init, target, shape, u, eps):
    """dense_trajectory.dense_trajectory with the potential eps in every step, and "sens" (N, L), "nk" (N, L)"""
    L, p, _ = shape
    N = len(u)
    dH = ed.dH_full(L, p)
    step = lambda v, a, b, fwd: ed.exact_step(v, L, p, D.J, D.DT, a, b, fwd, eps=eps)
    psi, xi = [init], [target]
    for i in range(N - 1):
        psi.append(step(psi[-1], u[i], u[i + 1], True))
    for i in range(N - 1, 0, -1):
        xi.insert(0, step(xi[0], u[i], u[i - 1], False))
    psi, xi = np.array(psi), np.array(xi)
    F = np.vdot(psi[-1], target)
    divT = np.array([np.vdot(xi[i], dH * psi[i]) for i in range(N)])
    fid = np.array([abs(np.vdot(target, s)) ** 2 for s in psi])
    xiH = dH * xi
    A, B = np.zeros((N, N)), np.zeros((N, N))
    for i in range(1, N - 1):
        phi = dH * psi[i]
        n = np.linalg.norm(phi)
        A[i, i] = D.DT * D.DT * (F * np.vdot(xiH[i], phi)).real
        phi = phi / n
        for j in range(i + 1, N - 1):
            phi = step(phi, u[j - 1], u[j], True)
            A[i, j] = A[j, i] = D.DT * D.DT * (F * n * np.vdot(xiH[j], phi)).real
        for j in range(1, N - 1):
            B[i, j] = -D.DT * D.DT * (divT[i] * np.conj(divT[j])).real
    sens, nk = sensitivities(psi, xi, F, shape)
    return {"psi": psi, "xi": xi, "F": F, "divT": divT, "fid": fid, "grad": D.DT * (1j * divT * F).real,
            "xiH_norm": np.linalg.norm(xiH, axis=1), "A": A, "B": B, "H": A + B, "sens": sens, "nk": nk}


def dense_cost(init, target, shape, u, eps):
    """0.5 (1 - |<target|psi_{N-1}>|^2)"""
    L, p, _ = shape
    psi = init
    for i in range(len(u) - 1):
        psi = ed.exact_step(psi, L, p, D.J, D.DT, u[i], u[i + 1], True, eps=eps)
    return 0.5 * (1.0 - abs(np.vdot(target, psi)) ** 2)


@functools.lru_cache(maxsize=None)
def pot_reference(name, n=None, k=0):
    """the dense reference of a case at traj_controls(traj, n, k), computed once and shared (do not modify)"""
    traj = traj_of(name)
    (_, _, init), (_, _, target) = T.traj_states(traj)
    return dense_trajectory(init, target, T.traj_shape(traj), T.traj_controls(traj, n, k), potential(name))


# ---------------------------------------------------------------------------- exact E on compact blocks
def e_pass(dims, data, shape, eps, tau):
    """E |state> on the compact format: block (k, q, n) times exp(-i tau eps_k n / 2)"""
    L, p, Q = shape
    d = np.asarray(dims).reshape(L + 1, Q + 1)
    out = np.array(data, dtype=np.complex128)
    off = 0
    for k in range(1, L + 1):
        for q in range(Q + 1):
            for n in range(p):
                if q + n > Q:
                    continue
                sz = int(d[k - 1, q]) * int(d[k, q + n])
                out[off:off + sz] *= np.exp(-0.5j * tau * eps[k - 1] * n)
                off += sz
    assert off == len(out) and sum(b.size for *_, b in ed.mps_blocks(dims, data, L, p, Q)) == off
    return out


class Composed:
    """getHessian of the trapped chain from the oracle's primitives and exact E passes"""

    def __init__(self, O, shape, eps):
        self.O, self.shape, self.eps = O, shape, np.asarray(eps, float)
        self.st = O.Stepper(*shape, D.J, D.DT, D.CUTOFF, D.MAXM)

    def step(self, m, u_from, u_to, forward=True):
        tau = D.DT if forward else -D.DT
        a = self.O.MPS(*self.shape, m.dims, e_pass(m.dims, m.data, self.shape, self.eps, tau))
        b = self.st.step(a, u_from, u_to, forward)
        return self.O.MPS(*self.shape, b.dims, e_pass(b.dims, b.data, self.shape, self.eps, tau))

    def hessian(self, init, target, u):
        """a dict like dense_trajectory's, the states as MPS lists psi, xi, xiH"""
        st, N = self.st, len(u)
        psi, xi = [init], [target]
        for i in range(N - 1):
            psi.append(self.step(psi[-1], u[i], u[i + 1], True))
        for i in range(N - 1, 0, -1):
            xi.insert(0, self.step(xi[0], u[i], u[i - 1], False))
        F = st.overlap(psi[-1], target)
        divT = np.array([st.overlap_dH(xi[i], psi[i]) for i in range(N)])
        fid = np.array([abs(st.overlap(target, s)) ** 2 for s in psi])
        xiH = [st.apply_dH(x) for x in xi]
        H = np.zeros((N, N))
        for i in range(1, N - 1):       # calcHessianRow (src/OptimalControl.cpp:251-283)
            psiH = st.apply_dH(psi[i])
            norm = np.sqrt(st.overlap(psiH, psiH).real)
            H[i, i] += D.DT * D.DT * ((F * st.overlap(xiH[i], psiH)).real - (divT[i] * np.conj(divT[i])).real)
            for j in range(i + 1, N - 1):
                psiH = self.step(psiH, u[j - 1], u[j], True)
                v = D.DT * D.DT * ((F * st.overlap(xiH[j], psiH) * norm).real - (divT[i] * np.conj(divT[j])).real)
                H[i, j] += v
                H[j, i] += v
        dpsi, dxi = [D.dense_of(m) for m in psi], [D.dense_of(m) for m in xi]
        sens, _ = sensitivities(dpsi, dxi, F, self.shape)
        return {"psi": psi, "xi": xi, "xiH": xiH, "F": F, "divT": divT, "fid": fid, "H": H, "sens": sens}


def sens_scale(ref):
    """dt max |<xi_t|n_k|psi_t>|: the unit of the sensitivities' deviation (|F| <= 1)"""
    return D.DT * float(np.abs(ref["nk"]).max())
