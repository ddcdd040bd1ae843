"""The C++ facade of the device snapshots: tests/cpp/sample_driver.cpp draws 256
shots of every psi_t at the config-1 shape, N_t = 21, once with
OptimalControl::samplePsit (ocg_sample) and once with the host sampleFock over
getPsit(), which shares the algorithm and the random numbers: the same
configurations, except where a decision's u lies within 1e-9 of a CDF boundary
(at most one such shot per 1000), logp within 1e-9, the same defect histogram at
the final time, and getPsitFockProbability of (1,1,1,1,1) against the host
contraction of getPsit()."""
import json
import os
import subprocess

import pytest

import facade_build as fb

pytestmark = pytest.mark.gpu


def _build():
    src = os.path.join(fb.HERE, "cpp", "sample_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "sample_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def test_snapshots_device_vs_host(tmp_path):
    fb.write_states(str(tmp_path))
    r = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    print(f"  {js['differ']} of {js['shots']} shots differ, logp deviation {js['dev_logp']:.3e}, "
          f"Mott probability deviation {js['dev_mott']:.3e} ({js['mott_first']:.4f} -> {js['mott_last']:.4f})")
    assert js["shots"] == 21 * 256 and js["bad"] == 0
    assert js["unexplained"] == 0 and js["differ"] * 1000 <= js["shots"]
    assert js["dev_logp"] < 1e-9
    assert js["dev_mott"] < 1e-12
    assert js["subset_equal"]
    assert sum(js["hist_dev"]) == 256
    if js["differ"] == 0:
        assert js["hist_dev"] == js["hist_host"]
    else:
        assert sum(abs(a - b) for a, b in zip(js["hist_dev"], js["hist_host"])) <= 2 * js["differ"]
    assert 0 < js["mott_first"] < 1 and 0 < js["mott_last"] < 1
