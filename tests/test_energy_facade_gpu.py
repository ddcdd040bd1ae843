"""The C++ facade of the device energy moments: tests/cpp/energy_driver.cpp runs
OptimalControl::getPsitEnergies on a config-1 ramp (N_t = 21) and compares <K>
and <D> of every psi_t with the host correlationFunction / expectationValues
over getPsit() to 1e-10, and InitializeState's energy / variance
out-parameters with the moments it reports beside them."""
import json
import os
import subprocess

import pytest

import facade_build as fb
from optimalcontrolmps_amd import ed

pytestmark = pytest.mark.gpu


def _build():
    src = os.path.join(fb.HERE, "cpp", "energy_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "energy_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def test_energies_device_vs_host(tmp_path):
    fb.write_states(str(tmp_path))
    r = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    print(f"  <K> deviation {js['dev_k1']:.3e}, <D> deviation {js['dev_d1']:.3e}, E deviation {js['dev_e']:.3e}; "
          f"E {js['e_first']:.6f} -> {js['e_last']:.6f}, Var {js['var_first']:.3e} -> {js['var_last']:.3e}; "
          f"ground state E {js['gs_e']:.9f} Var {js['gs_var']:.3e}")
    assert js["entries"] == 21
    assert js["dev_k1"] < 1e-10 and js["dev_d1"] < 1e-10
    assert js["dev_e"] < 5.1e-9          # the two bounds propagated: (J + max u) 1e-10, max u = 50
    assert js["dev_helper"] == 0.0 and js["subset_equal"]
    # psi_0 is the ED ground state of H(u_0): its energy, and a variance at rounding level; the ramp heats
    e0 = ed.ground_state_full(5, 5, 5, 1.0, 2.5)[1]
    assert abs(js["e_first"] - e0) < 1e-9 and abs(js["var_first"]) < 1e-9
    assert js["var_last"] > 1e-3 and js["min_var"] > -1e-9
    # InitializeState: the out-parameters are what its moments give, and the state is the one it returns anyway
    assert js["gs_e"] == js["gs_e_from_moments"] and js["gs_var"] == js["gs_var_from_moments"]
    assert js["gs_same_state"] and abs(js["gs_norm2"] - 1) < 1e-9
    # The state is the Trotter fixed point of imaginary time, not the eigenstate: with an infidelity eps <= 1e-7
    # (InitializeState.hpp: 6e-8 at this shape) and a spectral width W <= 2 J (L - 1) p + U L (L - 1) / 2 = 65,
    # 0 <= E - E0 <= eps W = 6.5e-6 and Var <= eps W^2 = 4.3e-4.
    assert -1e-9 <= js["gs_e"] - e0 <= 6.5e-6 and -1e-9 < js["gs_var"] <= 4.3e-4
