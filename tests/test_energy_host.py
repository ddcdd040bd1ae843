"""The host driver of ocg_observe_moments (csrc/observe_energy.hpp through
observe.hpp's run_chunk: table and list building, workspace sizing, output
indexing) over a CPU backend, built as a stand-alone program with
AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/energy_host.cpp: the
workspace is what the dry run counted, NaN-filled).  Its moments on both paths
against energy_reference to 1e-12 (norm2 + max |moment|): plain double sums in
another order than numpy's."""
import os
import subprocess

import numpy as np
import pytest

import energy_reference as E
import observe_reference as R
import spectrum_reference as S
from optimalcontrolmps_amd import ed

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("energy_host") / "energy_host")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(HERE, "cpp", "energy_host.cpp"), "-o", exe])
    return exe


def _cases():
    rng = np.random.default_rng(12)
    L, p, Q = 5, 4, 5
    narrow = [S.random_mps(rng, L, p, Q, 1, 3) for _ in range(2)]
    narrow.append(S.pad_sector(*narrow[0], L, p, Q, 2, 1))
    edge = [S.random_mps(rng, 3, 4, 3, lo, hi) for lo, hi in ((15, 16), (15, 17), (16, 16), (17, 17))]
    cut = [S.random_mps(rng, 5, 3, 5, 1, 4), ed.mps_from_full(ed.ground_state_full(5, 3, 5, 1.0, 8.0)[0], 5, 3, 5),
           R.fock(5, 3, 5, [1] * 5)]
    hard = [S.random_mps(rng, 6, 2, 3, 1, 3), R.fock(6, 2, 3, [1, 0, 1, 0, 1, 0])]
    return {"narrow": (L, p, Q, narrow), "tile_edge": (3, 4, 3, edge), "level_cut": (5, 3, 5, cut),
            "hard_core": (6, 2, 3, hard)}


@pytest.mark.parametrize("name", ["narrow", "tile_edge", "level_cut", "hard_core"])
def test_host_driver_under_asan_ubsan(program, tmp_path, name):
    L, p, Q, sts = _cases()[name]
    path = tmp_path / "states.txt"
    with open(path, "w") as f:
        f.write(f"{L} {p} {Q} {len(sts)}\n")
        for dims, data in sts:
            f.write(" ".join(str(int(d)) for d in np.asarray(dims).reshape(-1)) + "\n")
            f.write(" ".join(repr(float(x)) for x in np.asarray(data, np.complex128).view(np.float64)) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    cp = subprocess.run([program, str(path)], capture_output=True, text=True, env=env, timeout=600)
    bad = [m for m in ("ERROR: AddressSanitizer", "runtime error:") if m in cp.stderr]
    assert cp.returncode == 0 and not bad, (cp.returncode, cp.stderr[-3000:])
    rows = [ln.split() for ln in cp.stdout.splitlines()]
    assert len(rows) == 2 * len(sts)
    refs = [E.moments_ref(d, x, L, p, Q) for d, x in sts]
    paths = set()
    for r in rows:
        i, mom = int(r[1]), np.array([float(v) for v in r[2:]])
        dev = float(np.abs(mom - refs[i]).max())
        print(f"  {r[0]} state {i}: {dev / E.tol_scale(refs[i]):.3e} of the scale")
        assert dev <= 1e-12 * E.tol_scale(refs[i])
        paths.add(r[0])
    assert paths == {"chain", "list"}
    if name == "tile_edge":  # both sides of the dispatch in one chunk
        widest = [int(np.max(d)) for d, _ in sts]
        assert 16 in widest and max(widest) > 16
