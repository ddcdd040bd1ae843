"""The C++ facade of the device observables: tests/cpp/observe_driver.cpp runs
the CalculateDefects loop (and AnalyzeQuench's correlation matrices) at the
config-1 shape, N_t = 21, once on OptimalControl::getPsitObservables and the
TrajectoryObservables overloads of correlations.hpp, once with the host
functions over getPsit(); the two agree to 1e-10."""
import json
import os
import subprocess

import numpy as np
import pytest

import facade_build as fb

pytestmark = pytest.mark.gpu


def _build():
    src = os.path.join(fb.HERE, "cpp", "observe_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "observe_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def test_defects_loop_device_vs_host(tmp_path):
    fb.write_states(str(tmp_path))
    r = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    for k, v in js.items():
        if k.startswith("dev_"):
            print(f"  {k}: {v:.3e}")
            assert v < 1e-10, k
    assert js["bonds_equal"] and js["mirrored"] and js["subset_equal"]
    assert js["dev_exp_A"] == 0 and js["dev_exp_Adag"] == 0  # exactly 0 on both sides (particle conservation)
    assert len(js["rho"]) == 21 and abs(js["F2"][0] - 1) < 1e-12
    assert 0 < js["term_last"] <= 5 + 1e-9
