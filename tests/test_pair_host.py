"""The host driver of ocg_observe_pairs (csrc/observe_pair.hpp through observe.hpp's
run_chunk: table and list building, workspace sizing, output indexing) over a CPU
backend, built as a stand-alone program with AddressSanitizer +
UndefinedBehaviorSanitizer (tests/cpp/pairs_host.cpp: the workspace is what the dry
run counted, NaN-filled).  Its numbers on both paths against pair_reference.pairs_ref
to 1e-12 of sqrt(<x|x><y|y>) (times p - 1 for hop): plain double sums in another order
than numpy's."""
import os
import subprocess

import numpy as np
import pytest

import observe_reference as R
import pair_reference as P
import spectrum_reference as S
from optimalcontrolmps_amd import ed

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairs_host") / "pairs_host")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(HERE, "cpp", "pairs_host.cpp"), "-o", exe])
    return exe


def _cases():
    rng = np.random.default_rng(12)
    L, p, Q = 5, 4, 5
    a, b, c = (S.random_mps(rng, L, p, Q, lo, hi) for lo, hi in ((1, 3), (2, 4), (1, 2)))
    narrow = [(a, b), (b, a), (c, c), (S.pad_sector(*a, L, p, Q, 2, 1), b), (a, P.drop_sector(*b, L, p, Q, 2, 1)),
              (P.drop_sector(*b, L, p, Q, 3, 4), c)]
    e = [S.random_mps(rng, 3, 4, 3, lo, hi) for lo, hi in ((15, 16), (16, 16), (17, 17), (15, 17), (1, 3))]
    edge = [(e[0], e[1]), (e[0], e[2]), (e[2], e[1]), (e[3], e[3]), (e[4], e[2]), (e[4], e[0])]
    g = ed.mps_from_full(ed.ground_state_full(5, 3, 5, 1.0, 8.0)[0], 5, 3, 5)
    f = R.fock(5, 3, 5, [1] * 5)
    r = S.random_mps(rng, 5, 3, 5, 1, 4)
    cut = [(r, g), (g, f), (f, f), (R.fock(5, 3, 5, [1, 2, 0, 1, 1]), f), (f, R.fock(5, 3, 5, [1, 1, 1, 2, 0]))]
    h = S.random_mps(rng, 6, 2, 3, 1, 3)
    hard = [(h, R.fock(6, 2, 3, [1, 0, 1, 0, 1, 0])), (h, S.random_mps(rng, 6, 2, 3, 1, 2))]
    bond = [(S.random_mps(rng, 2, 3, 2, 1, 1), S.random_mps(rng, 2, 3, 2, 1, 1))]
    return {"narrow": (L, p, Q, narrow), "tile_edge": (3, 4, 3, edge), "level_cut": (5, 3, 5, cut),
            "hard_core": (6, 2, 3, hard), "single_bond": (2, 3, 2, bond)}


@pytest.mark.parametrize("name", ["narrow", "tile_edge", "level_cut", "hard_core", "single_bond"])
def test_host_driver_under_asan_ubsan(program, tmp_path, name):
    L, p, Q, prs = _cases()[name]
    path = tmp_path / "pairs.txt"
    with open(path, "w") as f:
        f.write(f"{L} {p} {Q} {len(prs)}\n")
        for pr in prs:
            for dims, data in pr:
                f.write(" ".join(str(int(d)) for d in np.asarray(dims).reshape(-1)) + "\n")
                f.write(" ".join(repr(float(x)) for x in np.asarray(data, np.complex128).view(np.float64)) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    cp = subprocess.run([program, str(path)], capture_output=True, text=True, env=env, timeout=600)
    bad = [m for m in ("ERROR: AddressSanitizer", "runtime error:") if m in cp.stderr]
    assert cp.returncode == 0 and not bad, (cp.returncode, cp.stderr[-3000:])
    rows = [ln.split() for ln in cp.stdout.splitlines()]
    assert len(rows) == 2 * len(prs)
    refs = [P.pairs_ref(*x, *y, L, p, Q) for x, y in prs]
    scales = [P.norm_of(*x, L, p, Q) * P.norm_of(*y, L, p, Q) for x, y in prs]
    paths = set()
    for r in rows:
        i = int(r[1])
        v = np.array([float(s) for s in r[2:]]).view(np.complex128)
        assert len(v) == 1 + L * p + 2 * (L - 1) and np.isfinite(v.view(np.float64)).all()
        got = {"ovl": v[0], "occ": v[1:1 + L * p].reshape(L, p), "hop": v[1 + L * p:].reshape(L - 1, 2)}
        dev = P.deviation(got, refs[i], p, scales[i])
        print(f"  {r[0]} pair {i}: {dev:.3e} of the scale")
        assert dev <= 1e-12
        paths.add(r[0])
    assert paths == {"chain", "list"}
    if name == "tile_edge":  # both sides of the dispatch in one chunk, and a narrow bra with a wide ket on the lists
        assert [r[0] for r in rows[:len(prs)]] == ["chain", "list", "list", "list", "list", "chain"]
