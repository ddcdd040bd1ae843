"""The C++ facade of the string-operator expectations: tests/cpp/strings_driver.cpp runs
OptimalControl::getPsitParityOrder, getPsitCountingStatistics and getPsitStringExpectations on the short
config-1 ramp of test_pair_facade_gpu.py (L = p = Q = 5, N_t = 21, gamma = 0) and compares them with the host
stringExpectation of correlations.hpp over getPsit(), to 1e-12 (both are exact contractions of the same
states; the values are divided by norm2, so the scale is 1), and checks that nothing is propagated."""
import json
import os
import subprocess

import pytest

import facade_build as fb
from test_pair_facade_gpu import _write

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _build():
    src = os.path.join(fb.HERE, "cpp", "strings_driver.cpp")
    os.makedirs(fb.BUILD, exist_ok=True)
    out = os.path.join(fb.BUILD, "strings_gpu")
    inc = os.path.join(fb.PKG, "include", "optimalcontrolmps")
    deps = [src, os.path.join(fb.ROOT, "include", "ocmps.h")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out + ".tmp", src, f"-L{fb.PKG}",
                               "-loptimalcontrolmps_amd", f"-Wl,-rpath,{fb.PKG}"])
        os.replace(out + ".tmp", out)
    return out


def test_parity_order_and_counting_statistics(tmp_path):
    _write(str(tmp_path), "init", 2.5)
    _write(str(tmp_path), "target", 4.0)
    r = subprocess.run([_build(), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout)
    N, L, Q = 21, 5, 5
    print(f"  parity order {js['dev_par']:.3e}, counting statistics {js['dev_cnt']:.3e}, raw expectations "
          f"{js['dev_raw']:.3e} against stringExpectation over getPsit() (tol {TOL:g}); |sum P - 1| "
          f"{js['sum_dev']:.3e}; propagation launches {js['prop']}")
    assert js["n_par"] == 3 and js["n_cnt"] == 3 and js["n_all"] == N
    assert js["cols_par"] == L and js["cols_cnt"] == Q + 1
    assert js["dev_par"] <= TOL and js["dev_cnt"] <= TOL and js["dev_raw"] <= TOL
    assert js["sum_dev"] <= TOL and js["below"] == 0
    # nothing is propagated by the observables, and the stored trajectories still serve the gradient
    assert js["prop"][0] > 0 and js["prop"][1] == js["prop"][0] and js["prop"][2] == js["prop"][0]
    assert js["grad_equal"]
    # the full chain holds Q = L bosons: parity (-1)^(Q - L nbar) = 1 exactly; shorter strings lie inside (-1, 1)
    first, last = js["par_first"], js["par_last"]
    assert abs(first[L - 1] - 1) <= TOL and abs(last[L - 1] - 1) <= TOL
    assert all(-1 < v < 1 for v in first[:L - 1] + last[:L - 1])
    assert min(js["cnt_last"]) >= -TOL
