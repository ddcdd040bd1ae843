"""The static site potential through the C++ facade: tests/cpp/potential_driver.cpp sets the trap of
dense_potential's (5,5,5) case on a GpuTDMRG, takes OptimalControl::getHessian with setThreadCount(2)
(every context makeEngine creates carries the potential) and prints it with 17 digits: the Python
binding's Engine.hessian of the same inputs, bit for bit.  getPsitEnergies refuses the trapped chain with
std::invalid_argument and works again without the potential; a single GpuTDMRG::step with and without it
equals Engine.step; the InitializeState overload that takes site energies returns the trapped ground state
(the infidelity and TOL of tests/test_ground_state.py) and refuses its energy out-parameter."""
import json
import os
import subprocess

import numpy as np
import pytest

import dense_potential as P
import dense_reference as D
import dense_trajectory as T
import facade_build as fb
from optimalcontrolmps_amd import ed

pytestmark = pytest.mark.gpu

NAME = "T_L5p5Q5"
U_GS = 2.5


def _build():
    src = os.path.join(fb.HERE, "cpp", "potential_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "potential_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def _write(directory, name, shape, dims, data):
    dims = np.ascontiguousarray(np.asarray(dims).reshape(-1), dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.complex128)
    with open(os.path.join(directory, name + ".bin"), "wb") as f:
        f.write(np.array([*shape, dims.size, data.size], dtype=np.int32).tobytes() + dims.tobytes() + data.tobytes())


def _mps(js, shape):
    from optimalcontrolmps_amd.native import MPS
    x = np.asarray(js["data"], np.float64)
    return MPS(*shape, np.asarray(js["dims"], np.int32), x[0::2] + 1j * x[1::2])


def test_facade_potential(tmp_path):
    from optimalcontrolmps_amd.native import MPS, Engine
    shape = T.traj_shape(NAME)
    L, p, Q = shape
    (di, xi, _), (dt, xt, _) = T.traj_states(NAME)
    u, eps = T.traj_controls(NAME), P.potential(NAME)
    _write(str(tmp_path), "init", shape, di, xi)
    _write(str(tmp_path), "target", shape, dt, xt)
    with open(os.path.join(str(tmp_path), "controls.txt"), "w") as f:
        f.write(" ".join(repr(float(x)) for x in u))
    r = subprocess.run([_build(), str(tmp_path), repr(U_GS)] + [repr(float(e)) for e in eps],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    assert js["zero_before"] and js["roundtrip"]

    e = Engine(*shape, D.J, D.DT, D.CUTOFF, D.MAXM)
    init = MPS(*shape, di, xi)
    e.set_states(MPS(*shape, dt, xt), init)
    one0 = e.step(init, 3.0, 7.0, True)
    e.set_potential(eps)
    H, _, _ = e.hessian(u)
    one = e.step(init, 3.0, 7.0, True)
    e.close()
    assert np.array_equal(np.asarray(js["H"]), H)
    ref = P.pot_reference(NAME)
    print(f"FIG {NAME} facade_H {np.abs(H - ref['H']).max() / T.hessian_scale(ref):.3e}")
    for got, want in ((js["step"], one), (js["step0"], one0)):
        m = _mps(got, shape)
        assert np.array_equal(m.dims, want.dims) and np.array_equal(m.data, want.data)
    assert not np.array_equal(one.data, one0.data)

    assert "site potential" in js["threw"] and "homogeneous" in js["threw"]
    assert js["n_energy"] == len(u) and np.isfinite(js["energy0"])
    assert "site potential" in js["gs_threw"]
    gs, _ = ed.ground_state_full(L, p, Q, D.J, U_GS, eps)
    m = _mps(js["gs"], shape)
    v = ed.full_from_mps(m.dims, m.data, L, p, Q)
    infid = 1.0 - abs(np.vdot(gs, v)) ** 2 / (np.vdot(v, v).real * np.vdot(gs, gs).real)
    print(f"FIG facade trapped_gs_infidelity {infid:.3e}")
    assert infid < 2e-7
