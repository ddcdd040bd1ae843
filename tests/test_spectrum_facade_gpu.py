"""The C++ facade of the device entanglement entropies:
tests/cpp/spectrum_driver.cpp runs AnalyzeQuench's entropy loop at the config-1
shape, N_t = 21, once as entanglementEntropy(getPsitObservables(ts, rows,
true), e) and once with the host entanglementEntropy(sites, psi_t[e]) over
getPsit(); the two agree within 1e-9 at every t and bond, and asking a
TrajectoryObservables taken without the entropies for them throws."""
import json
import os
import subprocess

import pytest

import facade_build as fb

pytestmark = pytest.mark.gpu


def _build():
    src = os.path.join(fb.HERE, "cpp", "spectrum_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "spectrum_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def test_entropy_loop_device_vs_host(tmp_path):
    fb.write_states(str(tmp_path))
    r = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    print(f"  entropy deviation {js['dev_entropy']:.3e}, weight sum deviation {js['dev_sum']:.3e}")
    assert js["dev_entropy"] < 1e-9
    assert js["dev_sum"] < 1e-10
    assert js["threw"] and js["plain_same"] and js["subset_equal"]
    assert len(js["mid"]) == 21 and 0 < js["entropy_max"] < 5
