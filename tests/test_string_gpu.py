"""ocg_observe_strings / ocg_observe_strings_states on the device (csrc/observe_string.hpp) on both engines
and on both paths: the chain kernels k_obs_string_env + k_obs_string (states whose bond sectors are all at
most 16 wide) and the task-list path (OCG_OBS_STRING_CHAIN=0 forces it).  Reference:
string_reference.strings_ref on the engine's own get_state output or on the host states, which
test_string_reference.py pins to the dense numbers.

Tolerance: TOL = 1e-10, the project's observable tolerance, relative to norm2 prod_k max_n |f[k][n]|.

Launches of one chunk (ocg_kernel_stats kind 9): 2 on the chain kernels, 2 (L - 1) + 2 M + 1 on the lists,
M the longest support of the request (an empty support counts 1).
"""
import os
import re

import numpy as np
import pytest

import observe_reference as R
import spectrum_reference as S
import string_reference as T
from optimalcontrolmps_amd import ed
from test_observe_gpu import C1, C1_U, CHAINS, _c1_engine, _mps
from test_pair_gpu import C1_TS, c1_runs  # noqa: F401  (the fixture)
from test_string_reference import random_tables, support_variants

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10
PATHS = ["chain", "list"]


def _path(monkeypatch, path):
    if path == "list":
        monkeypatch.setenv("OCG_OBS_STRING_CHAIN", "0")
    else:
        monkeypatch.delenv("OCG_OBS_STRING_CHAIN", raising=False)


def list_launches(L, f):
    longest = max([1] + [b - a + 1 for a, b in filter(None, (T.support(x) for x in f))])
    return 2 * (L - 1) + 2 * longest + 1


def _norm2(m):
    return float(R.observe_ref(m.dims, m.data, m.L, m.p, m.Q)["norm2"])


def _check(out, sts, f, what=""):
    """device numbers against the block reference of the host states; returns the references and scales"""
    assert out.shape == (len(sts), len(f)) and out.dtype == np.complex128
    refs = np.array([T.strings_ref(m.dims, m.data, m.L, m.p, m.Q, f) for m in sts])
    sc = np.array([T.scale(_norm2(m), f) for m in sts])
    worst = float((np.abs(out - refs) / sc).max())
    print(f"  {what}: largest deviation {worst:.3e} of the scale (tol {TOL:g})")
    assert worst <= TOL
    return refs, sc


def _tables(L, p, Q, seed=1):
    """random complex operators, the support variants, a parity row and a block's counting statistics"""
    rng = np.random.default_rng(seed)
    return np.concatenate([random_tables(rng, 2, L, p), support_variants(rng, L, p), T.parity_tables(L, p, 1, 1),
                           T.counting_tables(L, p, Q, min(2, L), min(4, L))])


# ------------------------------------------------------------ config-1 shape
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_config1_shape(c1_runs, engine, path, monkeypatch):
    """psi_t, xi_t and xiH_t against the reference, and the ties to the existing calls at the same states"""
    eng, sts = c1_runs(engine)
    _path(monkeypatch, path)
    L, p, Q = C1["L"], C1["p"], C1["Q"]
    f = _tables(L, p, Q)
    for w in (0, 1, 2):
        _check(eng.observe_strings(w, C1_TS, f), sts[w], f, f"{engine} {path} which {w}")
    rows = list(range(1, L + 1))
    one = eng.observe(0, C1_TS, rows)
    n2 = one["norm2"]
    nn = np.arange(p)
    # the identity is norm2; a one-site table is sum_n f occ
    rng = np.random.default_rng(2)
    g = T.identity(L, p, 1 + L)
    for k in range(L):
        g[1 + k, k] = random_tables(rng, 1, 1, p)[0, 0]
    out = eng.observe_strings(0, C1_TS, g)
    assert np.abs(out[:, 0] - n2).max() <= TOL * n2.max()
    for k in range(L):
        want = (g[1 + k, k] * one["occ"][:, k, :]).sum(-1)
        assert (np.abs(out[:, 1 + k] - want) <= TOL * T.scale(n2, g[1 + k])).all()
    # F_i = F_j = n is corr_nn[i][j]
    pairs = [(i, j) for i in rows for j in range(i + 1, L + 1)]
    g = T.identity(L, p, len(pairs))
    for m, (i, j) in enumerate(pairs):
        g[m, i - 1] = g[m, j - 1] = nn
    out = eng.observe_strings(0, C1_TS, g)
    for m, (i, j) in enumerate(pairs):
        assert np.abs(out[:, m] - one["nn"][:, i - 1, j - 1]).max() <= TOL * (p - 1) ** 2 * n2.max()
    # a product of projectors is |<n|s>|^2
    cfg = np.array([[1] * L, [2, 0] + [1] * (L - 2), [0, 1, 2] + [1] * (L - 3)], np.int8)
    assert (cfg.sum(1) == Q).all()
    g = np.zeros((len(cfg), L, p), complex)
    for m, c in enumerate(cfg):
        g[m, np.arange(L), c] = 1
    amp = eng.fock_amplitudes(0, C1_TS, cfg)
    assert np.abs(eng.observe_strings(0, C1_TS, g) - np.abs(amp) ** 2).max() <= TOL * n2.max()
    # counting statistics of the left block [1, b]: the weight of the Schmidt spectrum of bond b per sector
    sp = eng.spectrum(0, C1_TS)
    for b in range(1, L):
        P = eng.counting_statistics(0, C1_TS, 1, b)
        assert P.shape == (len(C1_TS), Q + 1)
        want = np.array([[sp["schmidt"][t, b - 1][sp["sector"][t, b - 1] == m].sum() for m in range(Q + 1)]
                         for t in range(len(C1_TS))]) / n2[:, None]
        assert np.abs(P - want).max() <= TOL and np.abs(P.sum(1) - 1).max() <= TOL
    # the parity row against its tables
    par = eng.parity_order(0, C1_TS, 2, 1)
    ref = eng.observe_strings(0, C1_TS, T.parity_tables(L, p, 2, 1)).real / n2[:, None]
    assert par.shape == (len(C1_TS), L) and not par[:, 0].any() and np.abs(par[:, 1:] - ref).max() <= TOL


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("L,p,Q,J,Ui,Uf", CHAINS + [(2, 3, 2, 1.0, 2.0, 10.0)])
@pytest.mark.parametrize("path", PATHS)
def test_general_chains(states, engine, L, p, Q, J, Ui, Uf, path, monkeypatch):
    """L = 3 and p - 1 < Q (empty sectors, the level cut) and L = 2, the trajectory states in each engine's own
    block layout"""
    from optimalcontrolmps_amd.native import MPS, Engine
    _path(monkeypatch, path)
    eng = Engine(L, p, Q, J, 0.01, 1e-8, engine=engine)
    if L == 2:
        gs = [MPS(L, p, Q, *ed.mps_from_full(ed.ground_state_full(L, p, Q, J, U)[0], L, p, Q)) for U in (Uf, Ui)]
        eng.set_states(*gs)
    else:
        eng.set_states(_mps(states, L, p, Q, J, Uf), _mps(states, L, p, Q, J, Ui))
    eng.propagate(np.random.default_rng(7).uniform(2, 10, 9), 3)
    f = _tables(L, p, Q, 3)
    ts = [0, 4, 8, 8]
    for w in (0, 1):
        _check(eng.observe_strings(w, ts, f), [eng.state(w, t) for t in ts], f, f"{engine} {path} which {w}")


# ------------------------------------------------------------ caller-supplied states
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("lo,hi", [(1, 3), (15, 17), (63, 66)])
def test_random_complex_states(engine, lo, hi, monkeypatch):
    """complex, non-canonical, unnormalised states; 15..17 crosses the chain / list dispatch and the MFMA tile
    edge, 63..66 the HBM engine's tile edges"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 3, 4, 3
    rng = np.random.default_rng(5)

    def draw(a, b):
        return MPS(L, p, Q, *S.random_mps(rng, L, p, Q, a, b))
    sts = [draw(lo, hi) for _ in range(3)]
    f = _tables(L, p, Q, 4)
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, 128, engine=engine)
    if (lo, hi) == (15, 17):
        assert max(int(m.dims.max()) for m in sts) > 16
        sts += [draw(16, 16), draw(15, 16), draw(17, 17), draw(16, 17)]
        assert int(sts[6].dims.max()) == 17
        eng.reset_stats()
        eng.observe_strings_states(sts[3:5], f)
        assert eng.stats(9)["launches"] == 2
        eng.reset_stats()
        eng.observe_strings_states(sts[5:], f)
        assert eng.stats(9)["launches"] == list_launches(L, f)
        eng.reset_stats()
        eng.observe_strings_states(sts[3:], f)  # both paths in one chunk
        assert eng.stats(9)["launches"] == 2 + list_launches(L, f)
    sts.append(MPS(L, p, Q, *S.pad_sector(sts[0].dims, sts[0].data, L, p, Q, 1, 1)))  # a zero-padded sector
    out = eng.observe_strings_states(sts, f)
    refs, sc = _check(out, sts, f, f"{engine} {lo}..{hi}")
    assert (np.abs(refs[-1] - refs[0]) / sc[0]).max() <= 1e-13
    assert (np.abs(out[-1] - out[0]) / sc[0]).max() <= TOL
    if hi <= 16:
        monkeypatch.setenv("OCG_OBS_STRING_CHAIN", "0")
        _check(eng.observe_strings_states(sts, f), sts, f, f"{engine} {lo}..{hi} list")


def test_chi256_state():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 20, 7, 20
    z = np.load(os.path.join(HERE, "golden", "c4_warm256.npz"), allow_pickle=False)
    x = MPS(L, p, Q, z["dims"], z["data"])
    assert max(x.bond_dims()) == 256
    eng = Engine(L, p, Q, 1.0, 0.005, 1e-8, 256, engine="hbm")
    # a short support, a long support and the empty support
    f = T.identity(L, p, 3)
    f[0, 9:11] = np.exp(0.7j * np.arange(p))
    f[1, 2:18] = (-1.0) ** (np.arange(p) - 1)
    eng.reset_stats()
    ps = eng.path_stats()
    out = eng.observe_strings_states([x], f)
    assert eng.path_stats() == ps
    s9 = eng.stats(9)
    assert s9["launches"] == list_launches(L, f) == 2 * (L - 1) + 2 * 16 + 1
    assert s9["alg_flops"] > 0 and s9["alg_bytes"] > 0 and s9["ms"] > 0
    _check(out, [x], f, "chi 256")


# ------------------------------------------------------------ launches and the two paths
@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_chain_kernel_against_list_path(c1_runs, engine, monkeypatch):
    eng, sts = c1_runs(engine)
    L, p, Q = C1["L"], C1["p"], C1["Q"]
    sets = {"all": _tables(L, p, Q), "short": T.counting_tables(L, p, Q, 2, 4), "empty": T.identity(L, p, 2),
            "one": T.parity_tables(L, p, 3, 1)[:1]}
    for name, f in sets.items():
        for w, ts in ((0, C1_TS), (1, [5])):
            eng.reset_stats()
            a = eng.observe_strings(w, ts, f)
            assert eng.stats(9)["launches"] == 2  # whatever nops and nt are
            monkeypatch.setenv("OCG_OBS_STRING_CHAIN", "0")
            eng.reset_stats()
            b = eng.observe_strings(w, ts, f)
            assert eng.stats(9)["launches"] == list_launches(L, f)
            monkeypatch.delenv("OCG_OBS_STRING_CHAIN")
            n2 = eng.observe(w, ts, outputs=("norm2",))["norm2"]
            dev = float((np.abs(a - b) / T.scale(n2[:, None], f[None])).max())
            print(f"  {name}, which {w}: chain against lists {dev:.3e} of the scale")
            assert dev <= TOL
    assert list_launches(L, sets["short"]) == 2 * (L - 1) + 2 * 3 + 1
    assert list_launches(L, sets["empty"]) == list_launches(L, sets["one"]) == 2 * (L - 1) + 3


# ------------------------------------------------------------ independence of the request
def _need(eng, t, f):
    """the chunk workspace one state's request takes, from the message of the OCG_ENOMEM it gets under a budget
    of one byte"""
    from optimalcontrolmps_amd.native import OcgError
    with pytest.raises(OcgError, match="ENOMEM") as ei:
        eng.observe_strings(0, [t], f)
    return int(re.search(r"\((\d+) B\)", str(ei.value)).group(1))


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_results_do_not_depend_on_the_request(c1_runs, engine, path, monkeypatch):
    eng, _ = c1_runs(engine)
    _path(monkeypatch, path)
    f = _tables(C1["L"], C1["p"], C1["Q"])
    every = eng.observe_strings(0, None, f)
    assert every.shape == (C1["Nt"], len(f))
    # an operator alone, with others, reordered; repeated and reordered ts
    assert np.array_equal(eng.observe_strings(0, [7], f[3:4]), every[[7], 3:4])
    perm = np.random.default_rng(0).permutation(len(f))
    pick = [20, 7, 7, 0, 13]
    assert np.array_equal(eng.observe_strings(0, pick, f[perm]), every[pick][:, perm])
    assert np.array_equal(eng.observe_strings(0, pick, f[[2, 2, 9]]), every[pick][:, [2, 2, 9]])
    # every state in a chunk of its own
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    need = max(_need(eng, t, f) for t in (0, 10, 20))
    monkeypatch.setenv("OCG_OBS_BUDGET", str(need))
    eng.reset_stats()
    split = eng.observe_strings(0, None, f)
    chunks = eng.stats(9)["launches"] // (2 if path == "chain" else list_launches(C1["L"], f))
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert chunks > 1 and np.array_equal(split, every)
    # host copies of the same states, staged
    if engine == "lds":  # (the compact format is the LDS engine's own block layout: the same operands)
        ts = [3, 20]
        assert np.array_equal(eng.observe_strings_states([eng.state(0, t) for t in ts], f), every[ts])


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_strings_leave_the_device_state(states, engine):
    eng = _c1_engine(states, engine)
    f = _tables(C1["L"], C1["p"], C1["Q"])
    H0, divT0, F0 = eng.hessian(C1_U)
    ps = eng.path_stats()
    eng.observe_strings(0, None, f)
    eng.observe_strings(2, [3, 3, 20], f[:2])
    eng.counting_statistics(1, [5], 2, 4)
    assert eng.path_stats() == ps
    H, divT, F = eng.hessian(C1_U)
    assert np.array_equal(H, H0) and np.array_equal(divT, divT0) and F == F0


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_errors(states, engine, monkeypatch):
    from optimalcontrolmps_amd import native as nat
    eng = _c1_engine(states, engine)
    L, p = C1["L"], C1["p"]
    f = _tables(L, p, C1["Q"])

    def fails(code, *a):
        with pytest.raises(nat.OcgError, match=code):
            eng.observe_strings(*a)
    fails("ESTATE", 0, [0], f)                       # before any propagate
    eng.propagate(C1_U, 3)
    assert eng.observe_strings(0, [0], f).shape == (1, len(f))
    fails("ESTATE", 2, [0], f)                       # no xi_dH yet
    for bad in ((0, [C1["Nt"]]), (0, [-1]), (3, [0]), (-1, [0])):
        fails("EINVAL", *bad, f)
    for v in (np.nan, np.inf):                       # a table entry that is not finite
        g = f.copy()
        g[1, 2, 1] = complex(1.0, v)
        fails("EINVAL", 0, [0], g)
    buf = np.full(8, 7.0)
    ptr = buf.ctypes.data_as(nat.dp)
    fp = np.ascontiguousarray(f).ctypes.data_as(nat.dp)
    one = (nat.C.c_int * 1)(0)
    lib = nat.lib()
    assert lib.ocg_observe_strings(eng.h, 0, one, 1, fp, -1, ptr) == 1        # nops < 0
    assert lib.ocg_observe_strings(eng.h, 0, one, 1, None, 2, ptr) == 1       # no tables
    # nops == 0 or nt == 0 writes nothing
    assert lib.ocg_observe_strings(eng.h, 0, one, 1, None, 0, ptr) == 0 and (buf == 7).all()
    assert lib.ocg_observe_strings(eng.h, 0, None, 0, fp, len(f), ptr) == 0 and (buf == 7).all()
    assert eng.observe_strings(0, [], f).shape == (0, len(f))
    assert eng.observe_strings(0, [1, 2], f[:0]).shape == (2, 0)
    assert eng.observe_strings_states([], f).shape == (0, len(f))
    # a budget too small for one state with all its operators
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    fails("ENOMEM", 0, [3], f)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert eng.observe_strings(0, [3], f).shape == (1, len(f))
    # a bond sector above order 512
    from optimalcontrolmps_amd.native import MPS
    dims = np.zeros((L + 1, C1["Q"] + 1), np.int32)
    st = eng.state(0, 0)
    dims[:] = st.dims.reshape(dims.shape)
    dims[2, 2] = 513
    wide = MPS(L, p, C1["Q"], dims.reshape(-1), np.zeros(ed.nelem(dims, L, p, C1["Q"]), np.complex128))
    with pytest.raises(nat.OcgError, match="ECAP"):
        eng.observe_strings_states([wide], f[:1])
