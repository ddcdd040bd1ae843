"""The C++ facade of the control sensitivities: tests/cpp/pairs_driver.cpp runs
OptimalControl::getControlSensitivities on the finite-difference fixture of
test_pair_gpu.py (L = p = Q = 5, N_t = 21, gamma = 0) and compares dU with
getAnalyticGradient, checks the particle-number sum rule of dEps, the reuse of the
stored trajectories with new_control = false, and the lengths a GROUP instance returns."""
import json
import os
import subprocess

import numpy as np
import pytest

import facade_build as fb
from optimalcontrolmps_amd import ed

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _build():
    src = os.path.join(fb.HERE, "cpp", "pairs_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "pairs_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def _write(directory, name, U):
    L, p, Q = 5, 5, 5
    dims, data = ed.mps_from_full(ed.ground_state_full(L, p, Q, 1.0, U)[0], L, p, Q)
    dims = np.ascontiguousarray(np.asarray(dims).reshape(-1), dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.complex128)
    with open(os.path.join(directory, name + ".bin"), "wb") as f:
        f.write(np.array([L, p, Q, dims.size, data.size], dtype=np.int32).tobytes() + dims.tobytes() + data.tobytes())


def test_control_sensitivities(tmp_path):
    _write(str(tmp_path), "init", 2.5)
    _write(str(tmp_path), "target", 4.0)
    r = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    dt, N, L = 0.01, 21, 5
    scale = dt * js["grad_max_over_dt"]  # = tstep max |Re(i divT F)| <= tstep |F| max |divT|
    print(f"  dU against getAnalyticGradient {js['dev_grad']:.3e} / {js['dev_grad2']:.3e} (bound {TOL * scale:.3e}), "
          f"sum_k dEps against Q tstep Re(i ovl F) {js['dev_sum']:.3e}, |F| {js['absF']:.6f}, "
          f"propagation launches {js['prop']}")
    assert js["n"] == N and js["n_eps"] == N and js["sites"] == L
    assert js["dev_grad"] <= TOL * scale and js["dev_grad2"] <= TOL * scale
    assert js["dev_sum"] <= TOL * dt * js["absF"]
    # new_control = false: the same numbers, nothing propagated
    assert js["reused_equal"]
    assert js["prop"][1] == js["prop"][0] and js["prop"][3] == js["prop"][2] and js["prop"][0] > 0
    # GROUP: on the time grid, not projected back; the gradient is on the basis
    assert js["group_n"] == N and js["group_n_J"] == N and js["group_n_eps"] == N and js["group_n_ovl"] == N
    assert js["group_grad_n"] == 5
    # the totals with trapezoid weights are the finite differences test_pair_gpu.py takes (FD_J = -6.624e-2,
    # FD_U = 1.780e-2 from the engines at J +- 1e-5 and u +- 1e-5), to the 1e-3 of that test
    w = np.ones(N)
    w[0] = w[-1] = 0.5
    assert abs((w * np.array(js["dJ"])).sum() / -6.624077e-2 - 1) <= 1e-3
    assert abs((w * np.array(js["dU"])).sum() / 1.780051e-2 - 1) <= 1e-3
