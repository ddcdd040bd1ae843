"""ctypes binding of liboptimalcontrolmps_amd.so (include/ocmps.h).

The shared library is built in-tree (``build_native()``, also run by
``__graft_entry__.build()``) with hipcc for gfx950 and lives next to this
file.  There is no fallback: if the library is missing or the HIP runtime has
no GPU, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_NAME = "liboptimalcontrolmps_amd.so"
LIB_PATH = os.environ.get("OCG_LIB", os.path.join(PKG_DIR, LIB_NAME))
CSRC = os.path.join(PKG_DIR, "csrc")
HEADER = os.path.join(ROOT, "include", "ocmps.h")

OCG_ERRORS = {1: "EINVAL", 2: "ECAP", 3: "EHIP", 4: "ESTATE", 5: "ENUM", 6: "ENOMEM"}


class OcgError(RuntimeError):
    pass


def sources():
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".hpp", ".cpp", ".h"))] + [HEADER]


def build_native(force: bool = False, nt: int | None = None, verbose: bool = False) -> str:
    """Compile csrc/ocmps.hip (LDS chain engine + C-ABI) and csrc/hbm.hip (HBM
    engine) for gfx950 into objects (in parallel) and link the in-tree shared
    library.  Each object is rebuilt only when a source it depends on changed."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    bdir = os.path.join(PKG_DIR, "build")
    os.makedirs(bdir, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
    if nt:
        flags.append(f"-DOCG_NT={int(nt)}")
    deps = {
        "ocmps": ["ocmps.hip", "engine.hpp", "engine_device.hpp", "kernels.hpp", "params.hpp", "hbm.hpp",
                  "fast.hpp", "fast_plan.hpp", "fast_chain.hpp", "fast_overlap.hpp", "observe.hpp",
                  "observe_eig.hpp", "observe_sample.hpp", "observe_energy.hpp", "observe_pair.hpp",
                  "observe_string.hpp", "observe_front.hpp"],
        "hbm": ["hbm.hip", "hbm.hpp", "hbm_device.hpp", "hbm_eig.hpp", "hbm_coop.hpp", "observe.hpp",
                "observe_eig.hpp", "observe_sample.hpp", "observe_energy.hpp", "observe_pair.hpp",
                "observe_string.hpp", "observe_front.hpp"],
    }
    tag = f"nt{int(nt)}" if nt else "prod"
    objs, procs = [], []
    for name, srcs in deps.items():
        obj = os.path.join(bdir, f"{name}.{tag}.o")
        objs.append(obj)
        newest = max([os.path.getmtime(os.path.join(CSRC, f)) for f in srcs] + [os.path.getmtime(HEADER)])
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            cmd = [hipcc] + flags + ["-c", os.path.join(CSRC, srcs[0]), "-o", obj + ".tmp"]
            if verbose:
                print(" ".join(cmd))
            procs.append((subprocess.Popen(cmd), obj))
    for pr, obj in procs:
        if pr.wait() != 0:
            raise OcgError(f"hipcc failed building {obj}")
        os.replace(obj + ".tmp", obj)
    if force or procs or not os.path.exists(LIB_PATH) or \
            os.path.getmtime(LIB_PATH) < max(os.path.getmtime(o) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH + ".tmp"] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


_lib = None
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
szp = C.POINTER(C.c_size_t)
bp = C.POINTER(C.c_byte)


class OcgInfo(C.Structure):
    _fields_ = [("L", C.c_int), ("p", C.c_int), ("Q", C.c_int), ("mps_max_nelem", C.c_size_t),
                ("lds_bytes", C.c_int), ("block_threads", C.c_int), ("device", C.c_int), ("fast_chain", C.c_int)]


class OcgPathStats(C.Structure):
    _fields_ = [("size", C.c_size_t), ("pipe_runs", C.c_long), ("pipe_fallbacks", C.c_long),
                ("ckpt_runs", C.c_long), ("ckpt_k", C.c_long), ("coop_launches", C.c_long),
                ("coop_groups", C.c_long), ("coop_fallbacks", C.c_long)]


# (name, restype, argtypes) for every entry point of include/ocmps.h
SIGNATURES = [
    ("ocg_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                             C.POINTER(C.c_void_p)]),
    ("ocg_create_ex", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                C.c_int, C.POINTER(C.c_void_p)]),
    ("ocg_destroy", C.c_int, [C.c_void_p]),
    ("ocg_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("ocg_last_error", C.c_char_p, [C.c_void_p]),
    ("ocg_get_info", C.c_int, [C.c_void_p, C.POINTER(OcgInfo)]),
    ("ocg_get_info_sz", C.c_int, [C.c_void_p, C.POINTER(OcgInfo), C.c_size_t]),
    ("ocg_abi_version", C.c_int, []),
    ("ocg_get_path_stats", C.c_int, [C.c_void_p, C.POINTER(OcgPathStats)]),
    ("ocg_set_tstep", C.c_int, [C.c_void_p, C.c_double]),
    ("ocg_set_potential", C.c_int, [C.c_void_p, dp]),
    ("ocg_get_potential", C.c_int, [C.c_void_p, dp]),
    ("ocg_mps_nelem", C.c_size_t, [C.c_int, C.c_int, C.c_int, ip]),
    ("ocg_step", C.c_int, [C.c_void_p, ip, dp, C.c_double, C.c_double, C.c_int, ip, dp, C.c_size_t, szp]),
    ("ocg_steps", C.c_int, [C.c_void_p, ip, dp, dp, C.c_int, C.c_int, ip, dp, C.c_size_t, szp]),
    ("ocg_imag_steps", C.c_int, [C.c_void_p, ip, dp, C.c_double, C.c_double, C.c_int, ip, dp, C.c_size_t, szp]),
    ("ocg_ground_state", C.c_int, [C.c_void_p, ip, dp, C.c_double, C.c_int, dp, C.c_int, C.c_double, C.c_int, ip, dp,
                                   C.c_size_t, szp, ip]),
    ("ocg_step_batch", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), dp, dp, C.c_int, ip, C.POINTER(dp), szp,
                                 szp]),
    ("ocg_overlap", C.c_int, [C.c_void_p, ip, dp, ip, dp, C.c_int, dp]),
    ("ocg_apply_dH", C.c_int, [C.c_void_p, ip, dp, ip, dp, C.c_size_t, szp, dp]),
    ("ocg_set_states", C.c_int, [C.c_void_p, ip, dp, ip, dp]),
    ("ocg_propagate", C.c_int, [C.c_void_p, dp, C.c_int, C.c_int]),
    ("ocg_overlap_factor", C.c_int, [C.c_void_p, dp]),
    ("ocg_fidelities", C.c_int, [C.c_void_p, dp]),
    ("ocg_div_t", C.c_int, [C.c_void_p, dp]),
    ("ocg_xi_dH", C.c_int, [C.c_void_p]),
    ("ocg_hessian_rows", C.c_int, [C.c_void_p, dp, C.c_int, ip, C.c_int, dp, dp, dp]),
    ("ocg_hessian", C.c_int, [C.c_void_p, dp, C.c_int, ip, C.c_int, dp, dp, dp]),
    ("ocg_hessian_multi", C.c_int, [C.c_void_p, C.c_int, dp, C.c_int, ip, C.c_int, dp, dp, dp]),
    ("ocg_gradient_multi", C.c_int, [C.c_void_p, C.c_int, dp, C.c_int, dp, dp]),
    ("ocg_gradient", C.c_int, [C.c_void_p, dp, C.c_int, dp, dp]),
    ("ocg_get_state", C.c_int, [C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_size_t, szp]),
    ("ocg_observe", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, ip, C.c_int, dp, dp, ip, dp, dp]),
    ("ocg_observe_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), ip, C.c_int, dp, dp, ip, dp, dp]),
    ("ocg_observe_spectrum", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.c_int, dp, dp, ip]),
    ("ocg_observe_spectrum_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), C.c_int, dp, dp, ip]),
    ("ocg_sample", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, C.c_int, C.c_ulonglong, bp, dp]),
    ("ocg_sample_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), C.c_int, C.c_ulonglong, bp, dp]),
    ("ocg_fock_amplitudes", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, bp, C.c_int, dp]),
    ("ocg_fock_amplitudes_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), bp, C.c_int, dp]),
    ("ocg_observe_moments", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, dp]),
    ("ocg_observe_moments_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), dp]),
    ("ocg_observe_pairs", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, ip, C.c_int, dp, dp, dp]),
    ("ocg_observe_pairs_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), ip, C.POINTER(dp), dp, dp, dp]),
    ("ocg_observe_strings", C.c_int, [C.c_void_p, C.c_int, ip, C.c_int, dp, C.c_int, dp]),
    ("ocg_observe_strings_states", C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(dp), dp, C.c_int, dp]),
    ("ocg_convert_hessian", C.c_int, [C.c_void_p, dp, C.c_int, dp, C.c_int, dp]),
    ("ocg_denmat_decomp", C.c_int, [C.c_void_p, C.c_int, ip, ip, C.POINTER(dp), C.c_double, C.c_int, ip,
                                    C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]),
    ("ocg_kernel_stats", C.c_int, [C.c_void_p, C.c_int, dp, C.POINTER(C.c_long), dp, dp, C.POINTER(C.c_long)]),
    ("ocg_reset_stats", C.c_int, [C.c_void_p]),
    ("ocg_profile", C.c_int, [C.c_void_p, dp, C.c_int]),
]


def lib():
    """Load the native library (raises OcgError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OcgError(f"{LIB_NAME} not built: run optimalcontrolmps_amd.native.build_native() "
                           "or __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ip)


class MPS:
    """Host MPS in the compact U(1)-block interchange format of include/ocmps.h
    (the IQMPS replacement): dims int32[(L+1)*(Q+1)], data complex128."""

    def __init__(self, L, p, Q, dims, data):
        self.L, self.p, self.Q = int(L), int(p), int(Q)
        self.dims = np.ascontiguousarray(np.asarray(dims, dtype=np.int32).reshape(-1))
        self.data = np.ascontiguousarray(np.asarray(data, dtype=np.complex128).reshape(-1))

    def bond_dims(self):
        return self.dims.reshape(self.L + 1, self.Q + 1).sum(axis=1)

    def raw(self):
        return self.data.view(np.float64)

    def copy(self):
        return MPS(self.L, self.p, self.Q, self.dims.copy(), self.data.copy())


def energy(mom, J, U):
    """<H(J, U)> = (-J k1 + U d1) / norm2 from moments (..., 7) of Engine.moments()"""
    mom = np.asarray(mom, np.float64)
    return (-J * mom[..., 1] + U * mom[..., 2]) / mom[..., 0]


def energy_variance(mom, J, U):
    """<H^2> - <H>^2 = (J^2 kk - 2 J U kd_re + U^2 dd) / norm2 - E^2 from moments (..., 7); U may be an
    array over the leading axes (the control of each stored state)"""
    mom = np.asarray(mom, np.float64)
    return (J * J * mom[..., 3] - 2 * J * U * mom[..., 5] + U * U * mom[..., 4]) / mom[..., 0] \
        - energy(mom, J, U) ** 2


def control_sensitivities(pairs, F, tstep):
    """First-order sensitivities of the cost 0.5 (1 - |F|^2) to the controls at every time step, from
    pairs = Engine.observe_pairs(1, None, 0, None) (bra xi_t, ket psi_t) and F = Engine.overlap_factor():
    dU[t] = tstep Re(i <xi_t|D|psi_t> F) (the gradient of Engine.gradient), dJ[t] = tstep Re(i (-<xi_t|K|psi_t>) F)
    for H = -J K + U D, dEps[t][k] = tstep Re(i <xi_t|n_k|psi_t> F) for a site potential sum_k eps_k n_k, and
    overlap[t] = <xi_t|psi_t> (independent of t for exact unitary evolution: its drift measures the truncation).
    They carry the time discretisation of the gradient formula: a total over t takes trapezoid weights (1/2 at
    t = 0 and t = N - 1)."""
    occ, hop, F = np.asarray(pairs["occ"]), np.asarray(pairs["hop"]), complex(F)
    n = np.arange(occ.shape[-1])
    nk = (occ * n).sum(-1)
    D = (occ * (n * (n - 1) / 2)).sum((-1, -2))
    K = hop.sum((-1, -2))
    return {"dU": tstep * (1j * D * F).real, "dJ": tstep * (1j * (-K) * F).real,
            "dEps": tstep * (1j * nk * F).real, "overlap": np.asarray(pairs["ovl"]).copy()}


class Engine:
    """One device context (ocg_ctx): the BH_tDMRG stepper + device-resident
    trajectories of the OptimalControl hot path."""

    ENGINES = {"auto": 0, "lds": 1, "hbm": 2}

    def __init__(self, L, p, npart, J, tstep, cutoff, maxm=0, device=0, engine="auto"):
        self.L, self.p, self.Q = L, p, npart
        self.J, self.tstep, self.cutoff, self.maxm = J, tstep, cutoff, maxm
        h = C.c_void_p()
        rc = lib().ocg_create_ex(device, L, p, npart, J, tstep, cutoff, maxm, self.ENGINES[engine], C.byref(h))
        if rc != 0:
            raise OcgError(f"ocg_create failed ({OCG_ERRORS.get(rc, rc)}): "
                           f"{lib().ocg_last_error(None).decode()}")
        self.h = h
        info = OcgInfo()
        lib().ocg_get_info(self.h, C.byref(info))
        self.info = info
        self.cap = int(info.mps_max_nelem)
        self.N = 0

    def close(self):
        if getattr(self, "h", None):
            lib().ocg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise OcgError(f"{what} failed ({OCG_ERRORS.get(rc, rc)}): {lib().ocg_last_error(self.h).decode()}")

    def _out(self):
        return (np.zeros((self.L + 1) * (self.Q + 1), np.int32), np.zeros(2 * self.cap), C.c_size_t(0))

    def _wrap(self, fd, d, n):
        return MPS(self.L, self.p, self.Q, fd.copy(), d[:2 * n.value].view(np.complex128).copy())

    # ------------------------------------------------ static site potential
    def set_potential(self, eps=None):
        """Site energies eps[L] of the static potential sum_k eps_k n_k (trap, tilt, disorder) of every later
        step, real and imaginary time; None (or all zeros) clears it.  Drops the device trajectories."""
        if eps is None:
            self._chk(lib().ocg_set_potential(self.h, None), "ocg_set_potential")
        else:
            e = np.asarray(eps, np.float64)
            if e.shape != (self.L,):
                raise ValueError(f"eps must have shape ({self.L},)")
            e, pe = _d(e)
            self._chk(lib().ocg_set_potential(self.h, pe), "ocg_set_potential")
        lib().ocg_get_info(self.h, C.byref(self.info))

    @property
    def potential(self):
        """the site energies in force (zeros when none is set)"""
        e = np.zeros(self.L)
        self._chk(lib().ocg_get_potential(self.h, e.ctypes.data_as(dp)), "ocg_get_potential")
        return e

    # ------------------------------------------------ TimeStepper-level
    def step(self, m: MPS, u_from, u_to, forward=True) -> MPS:
        fd, d, n = self._out()
        _, pd = _i(m.dims)
        raw, pr = _d(m.raw())
        self._chk(lib().ocg_step(self.h, pd, pr, u_from, u_to, int(forward), fd.ctypes.data_as(ip),
                                 d.ctypes.data_as(dp), self.cap, C.byref(n)), "ocg_step")
        return self._wrap(fd, d, n)

    def steps(self, m: MPS, u, forward=True) -> MPS:
        fd, d, n = self._out()
        _, pd = _i(m.dims)
        raw, pr = _d(m.raw())
        uu, pu = _d(u)
        self._chk(lib().ocg_steps(self.h, pd, pr, pu, len(uu) - 1, int(forward), fd.ctypes.data_as(ip),
                                  d.ctypes.data_as(dp), self.cap, C.byref(n)), "ocg_steps")
        return self._wrap(fd, d, n)

    def imag_steps(self, m: MPS, U, tau, nsteps) -> MPS:
        """nsteps imaginary-time steps exp(-tau H(J, U)) (ground-state preparation)"""
        fd, d, n = self._out()
        _, pd = _i(m.dims)
        raw, pr = _d(m.raw())
        self._chk(lib().ocg_imag_steps(self.h, pd, pr, float(U), float(tau), int(nsteps), fd.ctypes.data_as(ip),
                                       d.ctypes.data_as(dp), self.cap, C.byref(n)), "ocg_imag_steps")
        return self._wrap(fd, d, n)

    def ground_state(self, m: MPS, U, taus, block=25, tol=1e-13, max_steps=8000):
        """InitializeState's tau schedule on the device in one call (ocg_ground_state):
        returns (state, steps taken)"""
        fd, d, n = self._out()
        _, pd = _i(m.dims)
        raw, pr = _d(m.raw())
        tt, pt = _d(np.asarray(taus, np.float64))
        steps = C.c_int(0)
        self._chk(lib().ocg_ground_state(self.h, pd, pr, float(U), len(tt), pt, int(block), float(tol), int(max_steps),
                                         fd.ctypes.data_as(ip), d.ctypes.data_as(dp), self.cap, C.byref(n),
                                         C.byref(steps)), "ocg_ground_state")
        return self._wrap(fd, d, n), steps.value

    def step_batch(self, states, u_from, u_to, forward=True):
        """one step of every state (own controls each) in a single launch"""
        n = len(states)
        if n == 0:
            return []
        nsq = (self.L + 1) * (self.Q + 1)
        dims = np.ascontiguousarray(np.concatenate([m.dims for m in states]).astype(np.int32))
        raws = [np.ascontiguousarray(m.raw()) for m in states]
        data = (dp * n)(*[r.ctypes.data_as(dp) for r in raws])
        uf, puf = _d(np.asarray(u_from, np.float64).reshape(n))
        ut, put = _d(np.asarray(u_to, np.float64).reshape(n))
        od = np.zeros(n * nsq, np.int32)
        outs = [np.zeros(2 * self.cap) for _ in range(n)]
        odata = (dp * n)(*[o.ctypes.data_as(dp) for o in outs])
        caps = np.full(n, self.cap, dtype=np.uintp)
        nel = np.zeros(n, dtype=np.uintp)
        self._chk(lib().ocg_step_batch(self.h, n, dims.ctypes.data_as(ip), data, puf, put, int(forward),
                                       od.ctypes.data_as(ip), odata, caps.ctypes.data_as(szp),
                                       nel.ctypes.data_as(szp)), "ocg_step_batch")
        return [MPS(self.L, self.p, self.Q, od[i * nsq:(i + 1) * nsq].copy(),
                    outs[i][:2 * int(nel[i])].view(np.complex128).copy()) for i in range(n)]

    def overlap(self, x: MPS, y: MPS, with_dH=False) -> complex:
        out = np.zeros(2)
        _, a = _i(x.dims); rx, b = _d(x.raw()); _, c = _i(y.dims); ry, d = _d(y.raw())
        self._chk(lib().ocg_overlap(self.h, a, b, c, d, int(with_dH), out.ctypes.data_as(dp)), "ocg_overlap")
        return complex(out[0], out[1])

    def apply_dH(self, m: MPS):
        fd, d, n = self._out()
        nrm = C.c_double(0)
        _, pd = _i(m.dims)
        raw, pr = _d(m.raw())
        self._chk(lib().ocg_apply_dH(self.h, pd, pr, fd.ctypes.data_as(ip), d.ctypes.data_as(dp), self.cap,
                                     C.byref(n), C.byref(nrm)), "ocg_apply_dH")
        return self._wrap(fd, d, n), nrm.value

    # ------------------------------------------------ OptimalControl hot path
    def set_states(self, target: MPS, init: MPS):
        _, a = _i(target.dims); rt, b = _d(target.raw()); _, c = _i(init.dims); ri, d = _d(init.raw())
        self._chk(lib().ocg_set_states(self.h, a, b, c, d), "ocg_set_states")

    def propagate(self, u, which=3):
        uu, pu = _d(u)
        self.N = len(uu)
        self._chk(lib().ocg_propagate(self.h, pu, len(uu), which), "ocg_propagate")

    def overlap_factor(self) -> complex:
        out = np.zeros(2)
        self._chk(lib().ocg_overlap_factor(self.h, out.ctypes.data_as(dp)), "ocg_overlap_factor")
        return complex(out[0], out[1])

    def _need_N(self):
        if self.N <= 0:
            raise OcgError("no device trajectories yet: propagate() or hessian() first")

    def fidelities(self):
        self._need_N()
        out = np.zeros(self.N)
        self._chk(lib().ocg_fidelities(self.h, out.ctypes.data_as(dp)), "ocg_fidelities")
        return out

    def div_t(self):
        self._need_N()
        out = np.zeros(2 * self.N)
        self._chk(lib().ocg_div_t(self.h, out.ctypes.data_as(dp)), "ocg_div_t")
        return out.view(np.complex128).copy()

    def xi_dH(self):
        self._chk(lib().ocg_xi_dH(self.h), "ocg_xi_dH")

    def hessian_rows(self, u, rows, F: complex, divT, H=None):
        uu, pu = _d(u)
        N = len(uu)
        r, pr = _i(rows)
        Fa = np.array([F.real, F.imag])
        dv = np.ascontiguousarray(np.asarray(divT, np.complex128)).view(np.float64)
        if H is None:
            H = np.zeros((N, N))
        H = np.ascontiguousarray(H, dtype=np.float64)
        self._chk(lib().ocg_hessian_rows(self.h, pu, N, pr, len(r), Fa.ctypes.data_as(dp), dv.ctypes.data_as(dp),
                                         H.ctypes.data_as(dp)), "ocg_hessian_rows")
        return H

    def hessian(self, u, rows=None, H=None):
        """fused getHessian(u, new_control=true) fidelity part for `rows`
        (default 1..N-2): returns (H, divT, F); device trajectories are left
        as after propagate(u, 3) + xi_dH()"""
        uu, pu = _d(u)
        N = len(uu)
        self.N = N  # the device trajectories now have N states (fidelities / div_t size their outputs by it)
        if rows is None:
            rows = range(1, N - 1)
        r, pr = _i(list(rows))
        if H is None:
            H = np.zeros((N, N))
        H = np.ascontiguousarray(H, dtype=np.float64)
        dv = np.zeros(2 * N)
        Fa = np.zeros(2)
        self._chk(lib().ocg_hessian(self.h, pu, N, pr, len(r), H.ctypes.data_as(dp), dv.ctypes.data_as(dp),
                                    Fa.ctypes.data_as(dp)), "ocg_hessian")
        return H, dv.view(np.complex128).copy(), complex(Fa[0], Fa[1])

    def hessian_multi(self, U, rows=None):
        """K control vectors (rows of U, K x N) in one ocg_hessian_multi call:
        returns (H (K, N, N), divT (K, N), F (K,)); the device keeps control 0's
        trajectories"""
        Um = np.ascontiguousarray(np.atleast_2d(np.asarray(U, dtype=np.float64)))
        K, N = Um.shape
        self.N = N
        if rows is None:
            rows = range(1, N - 1)
        r, pr = _i(list(rows))
        H = np.zeros((K, N, N))
        dv = np.zeros((K, 2 * N))
        Fa = np.zeros((K, 2))
        self._chk(lib().ocg_hessian_multi(self.h, K, Um.ctypes.data_as(dp), N, pr, len(r), H.ctypes.data_as(dp),
                                          dv.ctypes.data_as(dp), Fa.ctypes.data_as(dp)), "ocg_hessian_multi")
        return H, dv.view(np.complex128).copy(), Fa[:, 0] + 1j * Fa[:, 1]

    def gradient(self, u):
        """getAnalyticGradient's device part for one control (ocg_gradient):
        returns (divT (N,), F); on the HBM engine, when the stored trajectories
        would not fit, psi || xi meet in the middle and none are kept"""
        uu, pu = _d(u)
        N = len(uu)
        dv = np.zeros(2 * N)
        Fa = np.zeros(2)
        self._chk(lib().ocg_gradient(self.h, pu, N, dv.ctypes.data_as(dp), Fa.ctypes.data_as(dp)), "ocg_gradient")
        self.N = N
        return dv.view(np.complex128).copy(), complex(Fa[0], Fa[1])

    def gradient_multi(self, U):
        """psi || xi + divT + F for K control vectors (rows of U) in one call:
        returns (divT (K, N), F (K,)); the device keeps control 0's trajectories"""
        Um = np.ascontiguousarray(np.atleast_2d(np.asarray(U, dtype=np.float64)))
        K, N = Um.shape
        self.N = N
        dv = np.zeros((K, 2 * N))
        Fa = np.zeros((K, 2))
        self._chk(lib().ocg_gradient_multi(self.h, K, Um.ctypes.data_as(dp), N, dv.ctypes.data_as(dp),
                                           Fa.ctypes.data_as(dp)), "ocg_gradient_multi")
        return dv.view(np.complex128).copy(), Fa[:, 0] + 1j * Fa[:, 1]

    def convert_hessian(self, Hu, V):
        """ControlBasis::convertHessian on the device: V Hu V^T (V is M x N)"""
        H, ph = _d(Hu)
        Vm, pv = _d(V)
        M, N = Vm.shape
        out = np.zeros((M, M))
        self._chk(lib().ocg_convert_hessian(self.h, ph, N, pv, M, out.ctypes.data_as(dp)), "ocg_convert_hessian")
        return out

    def denmat_decomp(self, mats, cutoff=None, maxm=None):
        """ITensor denmatDecomp (Fromleft) of independent dense complex blocks
        (rows <= cols <= any, rows <= 512) through the HBM engine's batched
        decomposition path (ocg_denmat_decomp): returns [(k, w, A, B)] with A
        (rows x k, orthonormal columns), B = A^H M (k x cols) and the rows Gram
        eigenvalues w as the eigensolver left them."""
        n = len(mats)
        Ms = [np.ascontiguousarray(np.asarray(m, np.complex128)) for m in mats]
        rows, pr = _i([m.shape[0] for m in Ms])
        cols, pc = _i([m.shape[1] for m in Ms])
        ws = [np.zeros(m.shape[0]) for m in Ms]
        As = [np.zeros(2 * m.shape[0] * m.shape[0]) for m in Ms]
        Bs = [np.zeros(2 * m.shape[0] * m.shape[1]) for m in Ms]
        arr = lambda xs: (dp * n)(*[x.view(np.float64).ctypes.data_as(dp) for x in xs])
        kept = np.zeros(n, np.int32)
        self._chk(lib().ocg_denmat_decomp(self.h, n, pr, pc, arr(Ms), self.cutoff if cutoff is None else cutoff,
                                          self.maxm if maxm is None else maxm, kept.ctypes.data_as(ip), arr(ws),
                                          arr(As), arr(Bs)), "ocg_denmat_decomp")
        out = []
        for i, m in enumerate(Ms):
            k, r, c = int(kept[i]), m.shape[0], m.shape[1]
            out.append((k, ws[i], As[i].view(np.complex128)[:r * k].reshape(r, k),
                        Bs[i].view(np.complex128)[:k * c].reshape(k, c)))
        return out

    def state(self, which, t) -> MPS:
        fd, d, n = self._out()
        self._chk(lib().ocg_get_state(self.h, which, t, fd.ctypes.data_as(ip), d.ctypes.data_as(dp), self.cap,
                                      C.byref(n)), "ocg_get_state")
        return self._wrap(fd, d, n)

    OBSERVE_OUTPUTS = ("norm2", "occ", "bond", "ada", "nn")

    def _observe_out(self, n, nrows, outputs):
        L, p = self.L, self.p
        bad = set(outputs) - set(self.OBSERVE_OUTPUTS)
        if bad:
            raise ValueError(f"unknown observe outputs {sorted(bad)}")
        full = {"norm2": lambda: np.zeros(n), "occ": lambda: np.zeros((n, L, p)),
                "bond": lambda: np.zeros((n, L + 1), np.int32),
                "ada": lambda: np.zeros((n, nrows, L), np.complex128), "nn": lambda: np.zeros((n, nrows, L))}
        return {k: full[k]() for k in self.OBSERVE_OUTPUTS if k in outputs}

    @staticmethod
    def _observe_ptrs(out, nrows):
        """the five output pointers of ocg_observe; NULL (skipped, its work not done) for what is not asked for"""
        def ptr(k, t):
            return out[k].ctypes.data_as(t) if k in out and (nrows or k not in ("ada", "nn")) else None
        return ptr("norm2", dp), ptr("occ", dp), ptr("bond", ip), ptr("ada", dp), ptr("nn", dp)

    def observe(self, which=0, ts=None, rows=(), outputs=OBSERVE_OUTPUTS):
        """Observables of the device trajectory states (ocg_observe): which 0 psi_t,
        1 xi_t, 2 xiH_t; ts state indices (default all), rows start sites in 1..L.
        Returns a dict of numpy arrays: norm2 (nt,), occ (nt, L, p) (raw, not divided
        by norm2), bond (nt, L+1), ada (nt, nrows, L) complex = <a+_i a_j> and nn
        (nt, nrows, L) = <n_i n_j>, both for j >= i (entries j < i are 0).  `outputs`
        selects a subset of these: what is left out is not computed."""
        tt, pt = _i(list(range(self.N)) if ts is None else list(ts))
        rr, pr = _i(list(rows))
        out = self._observe_out(len(tt), len(rr), outputs)
        self._chk(lib().ocg_observe(self.h, int(which), pt, len(tt), pr, len(rr), *self._observe_ptrs(out, len(rr))),
                  "ocg_observe")
        return out

    def observe_states(self, states, rows=(), outputs=OBSERVE_OUTPUTS):
        """The observables of observe() for caller-supplied host states (any gauge or
        norm), staged on the device in batches (ocg_observe_states)."""
        n = len(states)
        rr, pr = _i(list(rows))
        out = self._observe_out(n, len(rr), outputs)
        if n == 0:
            return out
        dims = np.ascontiguousarray(np.concatenate([m.dims for m in states]).astype(np.int32))
        raws = [np.ascontiguousarray(m.raw()) for m in states]
        data = (dp * n)(*[r.ctypes.data_as(dp) for r in raws])
        self._chk(lib().ocg_observe_states(self.h, n, dims.ctypes.data_as(ip), data, pr, len(rr),
                                           *self._observe_ptrs(out, len(rr))), "ocg_observe_states")
        return out

    SPECTRUM_OUTPUTS = ("entropy", "schmidt", "sector")

    def _spectrum_out(self, n, wcap, outputs):
        bad = set(outputs) - set(self.SPECTRUM_OUTPUTS)
        if bad:
            raise ValueError(f"unknown spectrum outputs {sorted(bad)}")
        nb = self.L - 1
        full = {"entropy": lambda: np.zeros((n, nb)), "schmidt": lambda: np.zeros((n, nb, wcap)),
                "sector": lambda: np.full((n, nb, wcap), -1, np.int32)}
        out = {k: full[k]() for k in self.SPECTRUM_OUTPUTS if k in outputs}
        ptr = lambda k, t: out[k].ctypes.data_as(t) if k in out else None
        return out, (ptr("entropy", dp), ptr("schmidt", dp), ptr("sector", ip))

    def spectrum(self, which=0, ts=None, outputs=SPECTRUM_OUTPUTS):
        """Entanglement spectra of the device trajectory states (ocg_observe_spectrum):
        which / ts as observe().  Returns a dict of numpy arrays: entropy (nt, L-1) at
        the bonds b = 1..L-1, schmidt (nt, L-1, wcap) the raw Schmidt weights of each
        bond (their sum is norm2), descending and padded with 0, and sector
        (nt, L-1, wcap) the left particle count of each weight, padded with -1; wcap is
        the largest bond dimension of the request.  `outputs` selects a subset."""
        tt, pt = _i(list(range(self.N)) if ts is None else list(ts))
        wcap = 0
        if len(tt) and ("schmidt" in outputs or "sector" in outputs):
            wcap = int(self.observe(which, tt, outputs=("bond",))["bond"].max())
        out, ptrs = self._spectrum_out(len(tt), wcap, outputs)
        self._chk(lib().ocg_observe_spectrum(self.h, int(which), pt, len(tt), wcap, *ptrs), "ocg_observe_spectrum")
        return out

    def spectrum_states(self, states, outputs=SPECTRUM_OUTPUTS):
        """spectrum() for caller-supplied host states of any gauge or norm
        (ocg_observe_spectrum_states)."""
        n = len(states)
        wcap = max([int(m.bond_dims().max()) for m in states], default=0)
        out, ptrs = self._spectrum_out(n, wcap, outputs)
        if n == 0:
            return out
        dims = np.ascontiguousarray(np.concatenate([m.dims for m in states]).astype(np.int32))
        raws = [np.ascontiguousarray(m.raw()) for m in states]
        data = (dp * n)(*[r.ctypes.data_as(dp) for r in raws])
        self._chk(lib().ocg_observe_spectrum_states(self.h, n, dims.ctypes.data_as(ip), data, wcap, *ptrs),
                  "ocg_observe_spectrum_states")
        return out

    def _staged(self, states):
        n = len(states)
        dims = np.ascontiguousarray(np.concatenate([m.dims for m in states]).astype(np.int32))
        raws = [np.ascontiguousarray(m.raw()) for m in states]
        return dims, raws, (dp * n)(*[r.ctypes.data_as(dp) for r in raws])

    def sample(self, which=0, ts=None, nshots=1, seed=0, logp=True):
        """Fock-state snapshots of the device trajectory states (ocg_sample): which / ts
        as observe().  Returns dict(config int8 (nt, nshots, L), logp (nt, nshots)):
        nshots occupation configurations per state drawn from |<n|s>|^2 / <s|s> and the
        log-probability of each.  The random numbers depend on (seed, t, shot, site)
        alone: a state's shots do not depend on what else is requested, and which is not
        mixed in.  A zero state gives -1 everywhere and logp = -inf.  logp=False skips
        that output."""
        tt, pt = _i(list(range(self.N)) if ts is None else list(ts))
        nshots = int(nshots)
        out = {"config": np.zeros((len(tt), max(nshots, 0), self.L), np.int8)}
        if logp:
            out["logp"] = np.zeros((len(tt), max(nshots, 0)))
        self._chk(lib().ocg_sample(self.h, int(which), pt, len(tt), nshots, int(seed) & (2 ** 64 - 1),
                                   out["config"].ctypes.data_as(bp),
                                   out["logp"].ctypes.data_as(dp) if logp else None), "ocg_sample")
        return out

    def sample_states(self, states, nshots=1, seed=0, logp=True):
        """sample() for caller-supplied host states of any gauge or norm (ocg_sample_states);
        the position of a state in the list takes the place of t in the random numbers."""
        n, nshots = len(states), int(nshots)
        out = {"config": np.zeros((n, max(nshots, 0), self.L), np.int8)}
        if logp:
            out["logp"] = np.zeros((n, max(nshots, 0)))
        if n == 0:
            return out
        dims, raws, data = self._staged(states)
        self._chk(lib().ocg_sample_states(self.h, n, dims.ctypes.data_as(ip), data, nshots, int(seed) & (2 ** 64 - 1),
                                          out["config"].ctypes.data_as(bp),
                                          out["logp"].ctypes.data_as(dp) if logp else None), "ocg_sample_states")
        return out

    def fock_amplitudes(self, which=0, ts=None, configs=()):
        """<n|s> of the configurations configs (nconf, L) for the device trajectory states
        (ocg_fock_amplitudes): complex (nt, nconf), raw (sum over all n of |amp|^2 = norm2)."""
        tt, pt = _i(list(range(self.N)) if ts is None else list(ts))
        cf = np.ascontiguousarray(np.asarray(configs, np.int8).reshape(-1, self.L))
        out = np.zeros((len(tt), len(cf)), np.complex128)
        self._chk(lib().ocg_fock_amplitudes(self.h, int(which), pt, len(tt), cf.ctypes.data_as(bp), len(cf),
                                            out.ctypes.data_as(dp)), "ocg_fock_amplitudes")
        return out

    def fock_amplitudes_states(self, states, configs=()):
        """fock_amplitudes() for caller-supplied host states (ocg_fock_amplitudes_states)."""
        n = len(states)
        cf = np.ascontiguousarray(np.asarray(configs, np.int8).reshape(-1, self.L))
        out = np.zeros((n, len(cf)), np.complex128)
        if n == 0:
            return out
        dims, raws, data = self._staged(states)
        self._chk(lib().ocg_fock_amplitudes_states(self.h, n, dims.ctypes.data_as(ip), data, cf.ctypes.data_as(bp),
                                                   len(cf), out.ctypes.data_as(dp)), "ocg_fock_amplitudes_states")
        return out

    def moments(self, which=0, ts=None):
        """Energy moments of the device trajectory states (ocg_observe_moments): which /
        ts as observe().  Returns (nt, 7): norm2, k1 = <K>, d1 = <D>, kk = <K K>,
        dd = <D D>, kd_re, kd_im = <K D>, raw (not divided by norm2), for H = -J K + U D
        with K the hopping sum and D = sum n (n - 1) / 2: see energy() and
        energy_variance() of this module."""
        tt, pt = _i(list(range(self.N)) if ts is None else list(ts))
        out = np.zeros((len(tt), 7))
        self._chk(lib().ocg_observe_moments(self.h, int(which), pt, len(tt), out.ctypes.data_as(dp)),
                  "ocg_observe_moments")
        return out

    def moments_states(self, states):
        """moments() for caller-supplied host states of any gauge or norm
        (ocg_observe_moments_states)."""
        n = len(states)
        out = np.zeros((n, 7))
        if n == 0:
            return out
        dims, raws, data = self._staged(states)
        self._chk(lib().ocg_observe_moments_states(self.h, n, dims.ctypes.data_as(ip), data, out.ctypes.data_as(dp)),
                  "ocg_observe_moments_states")
        return out

    PAIR_OUTPUTS = ("ovl", "occ", "hop")

    def _pairs_out(self, n, outputs):
        bad = set(outputs) - set(self.PAIR_OUTPUTS)
        if bad:
            raise ValueError(f"unknown pair outputs {sorted(bad)}")
        L, p = self.L, self.p
        full = {"ovl": (n,), "occ": (n, L, p), "hop": (n, L - 1, 2)}
        out = {k: np.zeros(full[k], np.complex128) for k in self.PAIR_OUTPUTS if k in outputs}
        return out, [out[k].ctypes.data_as(dp) if k in out else None for k in self.PAIR_OUTPUTS]

    def observe_pairs(self, which_x, tx, which_y, ty, outputs=PAIR_OUTPUTS):
        """Transition matrix elements between device trajectory states (ocg_observe_pairs): pair e has the
        bra state tx[e] of trajectory which_x and the ket state ty[e] of which_y (0 psi_t, 1 xi_t, 2 xiH_t;
        None: 0..n-1).  Returns a dict of complex arrays, raw (not divided by any norm): ovl (n,) = <x|y>,
        occ (n, L, p) = <x|P_k(n)|y> and hop (n, L-1, 2) = <x|a+_b a_{b+1}|y>, <x|a_b a+_{b+1}|y>.
        `outputs` selects a subset: what is left out is not computed."""
        n = self.N if tx is None and ty is None else len(tx if tx is not None else ty)
        ax, px = (None, None) if tx is None else _i(list(tx))
        ay, py = (None, None) if ty is None else _i(list(ty))
        if ax is not None and ay is not None and len(ax) != len(ay):
            raise ValueError("tx and ty differ in length")
        out, ptrs = self._pairs_out(n, outputs)
        self._chk(lib().ocg_observe_pairs(self.h, int(which_x), px, int(which_y), py, n, *ptrs), "ocg_observe_pairs")
        return out

    def observe_pairs_states(self, xs, ys, outputs=PAIR_OUTPUTS):
        """observe_pairs() for caller-supplied host states of any gauge or norm: pair e is (xs[e], ys[e])
        (ocg_observe_pairs_states)."""
        if len(xs) != len(ys):
            raise ValueError("xs and ys differ in length")
        n = len(xs)
        out, ptrs = self._pairs_out(n, outputs)
        if n == 0:
            return out
        dx, rx, datx = self._staged(xs)
        dy, ry, daty = self._staged(ys)
        self._chk(lib().ocg_observe_pairs_states(self.h, n, dx.ctypes.data_as(ip), datx, dy.ctypes.data_as(ip), daty,
                                                 *ptrs), "ocg_observe_pairs_states")
        return out

    def _string_tables(self, f):
        f = np.ascontiguousarray(np.asarray(f, np.complex128))
        if f.ndim != 3 or f.shape[1:] != (self.L, self.p):
            raise ValueError(f"operator tables must have shape (nops, {self.L}, {self.p})")
        return f

    def observe_strings(self, which, ts, f):
        """Expectations of products of diagonal one-site operators in the device trajectory states
        (ocg_observe_strings): which / ts as observe(); f complex (nops, L, p), operator m is the product
        over the sites k of sum_n f[m][k-1][n] P_k(n) (a site whose table is all 1 is outside the
        operator's support).  Returns complex (nt, nops) = <s|O_m|s>, raw (not divided by norm2)."""
        tt, pt = _i(list(range(self.N)) if ts is None else list(ts))
        f = self._string_tables(f)
        out = np.zeros((len(tt), len(f)), np.complex128)
        self._chk(lib().ocg_observe_strings(self.h, int(which), pt, len(tt), f.ctypes.data_as(dp), len(f),
                                            out.ctypes.data_as(dp)), "ocg_observe_strings")
        return out

    def observe_strings_states(self, states, f):
        """observe_strings() for caller-supplied host states of any gauge or norm
        (ocg_observe_strings_states)."""
        n = len(states)
        f = self._string_tables(f)
        out = np.zeros((n, len(f)), np.complex128)
        if n == 0:
            return out
        dims, raws, data = self._staged(states)
        self._chk(lib().ocg_observe_strings_states(self.h, n, dims.ctypes.data_as(ip), data, f.ctypes.data_as(dp),
                                                   len(f), out.ctypes.data_as(dp)), "ocg_observe_strings_states")
        return out

    def _norm2_of_strings(self, which, ts, f):
        """observe_strings() with the identity appended: (values, norm2)"""
        f = np.concatenate([f, np.ones((1, self.L, self.p), np.complex128)])
        out = self.observe_strings(which, ts, f)
        return out[:, :-1], out[:, -1].real

    def parity_order(self, which, ts, i, nbar):
        """The parity (string) order from site i (1-based): real (nt, L), entry j-1 =
        <prod_{k=i..j} (-1)^(n_k - nbar)> / norm2 for j >= i, entries below i are 0."""
        i = int(i)
        if not 1 <= i <= self.L:
            raise ValueError("site out of 1..L")
        sign = np.array([(-1.0) ** (n - int(nbar)) for n in range(self.p)])
        f = np.ones((self.L - i + 1, self.L, self.p), np.complex128)
        for m in range(len(f)):
            f[m, i - 1:i + m] = sign
        val, norm2 = self._norm2_of_strings(which, ts, f)
        out = np.zeros((len(val), self.L))
        out[:, i - 1:] = val.real / norm2[:, None]
        return out

    def counting_statistics(self, which, ts, i, j):
        """The distribution of the boson number in the sites i..j (1-based, inclusive): real (nt, Q+1),
        entry m = P(N_A = m).  The Q+1 generating-function values G_r = <exp(i theta_r N_A)>,
        theta_r = 2 pi r / (Q+1), come from the device; P(m) = Re[sum_r exp(-i theta_r m) G_r / (Q+1)] / norm2
        (exact, since N_A <= Q) is formed on the host."""
        i, j = int(i), int(j)
        if not 1 <= i <= j <= self.L:
            raise ValueError("block out of 1 <= i <= j <= L")
        Q1 = self.Q + 1
        theta = 2 * np.pi * np.arange(Q1) / Q1
        f = np.ones((Q1, self.L, self.p), np.complex128)
        f[:, i - 1:j, :] = np.exp(1j * theta[:, None, None] * np.arange(self.p)[None, None, :])
        G, norm2 = self._norm2_of_strings(which, ts, f)
        dft = np.exp(-1j * np.outer(theta, np.arange(Q1)))  # [r][m]
        return (G @ dft).real / Q1 / norm2[:, None]

    def stats(self, kind):
        ms = C.c_double(); n = C.c_long(); b = C.c_double(); f = C.c_double(); s = C.c_long()
        self._chk(lib().ocg_kernel_stats(self.h, kind, C.byref(ms), C.byref(n), C.byref(b), C.byref(f),
                                         C.byref(s)), "ocg_kernel_stats")
        return {"ms": ms.value, "launches": n.value, "alg_bytes": b.value, "alg_flops": f.value,
                "sweep_steps": s.value}

    def path_stats(self):
        """named path counters of the HBM engine (ocg_get_path_stats): pipelined /
        two-phase-fallback / checkpointed getHessians, multi-CU eigenvalue launches,
        blocks and groups re-run on one CU"""
        st = OcgPathStats()
        st.size = C.sizeof(OcgPathStats)
        self._chk(lib().ocg_get_path_stats(self.h, C.byref(st)), "ocg_get_path_stats")
        return {k: getattr(st, k) for k, _ in OcgPathStats._fields_ if k != "size"}

    def profile(self, reset=True):
        out = np.zeros(32)
        self._chk(lib().ocg_profile(self.h, out.ctypes.data_as(dp), int(reset)), "ocg_profile")
        return out

    def reset_stats(self):
        self._chk(lib().ocg_reset_stats(self.h), "ocg_reset_stats")
