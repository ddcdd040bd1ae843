"""ocg_observe_moments / ocg_observe_moments_states on the device
(csrc/observe_energy.hpp) on both engines and on both paths: the chain kernel
k_obs_energy (states whose bond sectors are all at most 16 wide) and the
task-list path (OCG_OBS_ENERGY_CHAIN=0 forces it).  Reference:
energy_reference.moments_ref on the engine's own get_state output or on the
host state, which test_energy_reference.py pins to the dense moments.

Tolerance: 1e-10 (norm2 + max |moment|), the project's observable tolerance
scaled by the magnitudes; the variance of an eigenstate to the same tolerance
propagated, 1e-10 (J^2 |kk| + 2 |J U kd_re| + U^2 |dd| + E^2) / norm2.
"""
import os
import re

import numpy as np
import pytest

import energy_reference as E
import observe_reference as R
import spectrum_reference as S
from optimalcontrolmps_amd import ed
from test_observe_gpu import C1, C1_U, CHAINS, _c1_engine, _mps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10
PATHS = ["chain", "list"]


def _path(monkeypatch, path):
    if path == "list":
        monkeypatch.setenv("OCG_OBS_ENERGY_CHAIN", "0")
    else:
        monkeypatch.delenv("OCG_OBS_ENERGY_CHAIN", raising=False)


def _check(mom, sts, what=""):
    """device moments against the block reference of the host states sts; returns the references"""
    assert mom.shape == (len(sts), 7) and mom.dtype == np.float64
    refs = np.array([E.moments_ref(m.dims, m.data, m.L, m.p, m.Q) for m in sts])
    worst = 0.0
    for got, ref in zip(mom, refs):
        dev = float(np.abs(got - ref).max()) / E.tol_scale(ref)
        worst = max(worst, dev)
    print(f"  {what}: largest deviation {worst:.3e} of (norm2 + max|moment|) (tol {TOL:g})")
    assert worst <= TOL
    return refs


# ------------------------------------------------------------ config-1 shape
C1_TS = [0, 1, 10, 20]


@pytest.fixture(scope="module")
def c1_runs(states):
    """per engine: the context after propagate + xi_dH and the host copies of the states at C1_TS"""
    cache = {}

    def get(engine):
        if engine not in cache:
            eng = _c1_engine(states, engine)
            eng.propagate(C1_U, 3)
            eng.xi_dH()
            cache[engine] = (eng, [[eng.state(w, t) for t in C1_TS] for w in (0, 1, 2)])
        return cache[engine]
    return get


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_config1_shape(c1_runs, engine, path, monkeypatch):
    """psi_t, xi_t and the unnormalised xiH_t (centre wherever the sweep left it)"""
    eng, sts = c1_runs(engine)
    _path(monkeypatch, path)
    for which in (0, 1, 2):
        assert max(int(m.dims.max()) for m in sts[which]) <= 16
        refs = _check(eng.moments(which, C1_TS), sts[which], f"{engine} {path} which {which}")
        if which < 2:
            assert np.abs(refs[:, 0] - 1).max() < 1e-6
    # psi_0 is the ground state at U = 2.5: its energy is the ED eigenvalue, its variance is rounding
    mom = eng.moments(0, [0])[0]
    from optimalcontrolmps_amd.native import energy, energy_variance
    e0 = ed.ground_state_full(C1["L"], C1["p"], C1["Q"], C1["J"], 2.5)[1]
    assert abs(energy(mom, C1["J"], 2.5) - e0) < 1e-9
    assert abs(energy_variance(mom, C1["J"], 2.5)) < 1e-7  # (the stored state went through one 1e-8 cut)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("L,p,Q,J,Ui,Uf", CHAINS)
@pytest.mark.parametrize("path", PATHS)
def test_general_chains(states, engine, L, p, Q, J, Ui, Uf, path, monkeypatch):
    """L = 3 and p - 1 < Q (empty sectors, a+ at the level cut, missing partners), the trajectory states in
    each engine's own block layout"""
    from optimalcontrolmps_amd.native import Engine
    _path(monkeypatch, path)
    eng = Engine(L, p, Q, J, 0.01, 1e-8, engine=engine)
    eng.set_states(_mps(states, L, p, Q, J, Uf), _mps(states, L, p, Q, J, Ui))
    eng.propagate(np.random.default_rng(7).uniform(2, 10, 9), 3)
    ts = [0, 4, 8]
    for which in (0, 1):
        _check(eng.moments(which, ts), [eng.state(which, t) for t in ts], f"{engine} {path} which {which}")


def test_hbm_wide_trajectory_states():
    """sectors above 16 in the HBM engine's own trajectory layout: the task lists, beside narrow states of the
    same trajectory on the chain kernel in one call"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 10, 4, 10
    f = MPS(L, p, Q, *R.fock(L, p, Q, [1] * L))
    eng = Engine(L, p, Q, 1.0, 0.03, 1e-10, 128, engine="hbm")
    eng.set_states(f, f)
    eng.propagate(np.linspace(2.0, 6.0, 31), 1)
    ts = [0, 1, 15, 30]
    sts = [eng.state(0, t) for t in ts]
    assert sts[0].dims.max() <= 16 < sts[-1].dims.max()
    refs = _check(eng.moments(0, ts), sts, "hbm wide")
    assert np.abs(refs[0] - [1.0, 0.0, 0.0, 4.0 * (L - 1), 0.0, 0.0, 0.0]).max() < 1e-13


# ------------------------------------------------------------ caller-supplied states
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("lo,hi", [(1, 3), (15, 17), (63, 66)])
def test_random_complex_states(engine, lo, hi, monkeypatch):
    """complex, non-canonical, unnormalised states; 15..17 crosses the chain / list dispatch and the MFMA tile edge"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 3, 4, 3
    rng = np.random.default_rng(5)
    sts = [MPS(L, p, Q, *S.random_mps(rng, L, p, Q, lo, hi)) for _ in range(3)]
    if (lo, hi) == (15, 17):
        assert max(int(m.dims.max()) for m in sts) > 16
        # both sides of the dispatch in one call: states that stay on the chain kernel beside them
        sts += [MPS(L, p, Q, *S.random_mps(rng, L, p, Q, 16, 16)), MPS(L, p, Q, *S.random_mps(rng, L, p, Q, 15, 16))]
    pad = S.pad_sector(sts[0].dims, sts[0].data, L, p, Q, 1, 1)
    sts.append(MPS(L, p, Q, *pad))
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, 128, engine=engine)
    mom = eng.moments_states(sts)
    refs = _check(mom, sts, f"{engine} {lo}..{hi}")
    assert np.abs(refs[:, 6]).min() > 0  # complex states: <K D> has an imaginary part
    if hi <= 16:
        monkeypatch.setenv("OCG_OBS_ENERGY_CHAIN", "0")
        _check(eng.moments_states(sts), sts, f"{engine} {lo}..{hi} list")


def test_chi256_state():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 20, 7, 20
    z = np.load(os.path.join(HERE, "golden", "c4_warm256.npz"), allow_pickle=False)
    st = MPS(L, p, Q, z["dims"], z["data"])
    assert max(st.bond_dims()) == 256
    eng = Engine(L, p, Q, 1.0, 0.005, 1e-8, 256, engine="hbm")
    eng.reset_stats()
    ps = eng.path_stats()
    _check(eng.moments_states([st]), [st], "chi 256")
    assert eng.path_stats() == ps
    s9 = eng.stats(9)
    assert s9["launches"] == 2 * L + 1 and s9["alg_flops"] > 0 and s9["alg_bytes"] > 0 and s9["ms"] > 0


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_chain_kernel_against_list_path(c1_runs, engine, monkeypatch):
    eng, sts = c1_runs(engine)
    for which in (0, 1, 2):
        eng.reset_stats()
        a = eng.moments(which, C1_TS)
        assert eng.stats(9)["launches"] == 1  # the whole chunk in one launch
        monkeypatch.setenv("OCG_OBS_ENERGY_CHAIN", "0")
        eng.reset_stats()
        b = eng.moments(which, C1_TS)
        assert eng.stats(9)["launches"] == 2 * C1["L"] + 1
        monkeypatch.delenv("OCG_OBS_ENERGY_CHAIN")
        dev = max(float(np.abs(x - y).max()) / E.tol_scale(y) for x, y in zip(a, b))
        print(f"  which {which}: chain against lists {dev:.3e} of the scale")
        assert dev <= TOL


# ------------------------------------------------------------ exact cases
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_exact_product_states(engine, path, monkeypatch):
    from optimalcontrolmps_amd.native import MPS, Engine
    _path(monkeypatch, path)
    for L, p, kk in ((5, 3, 16.0), (5, 2, 0.0), (4, 5, 12.0)):
        f = MPS(L, p, L, *R.fock(L, p, L, [1] * L))
        half = f.copy()
        half.data[0] *= 0.5
        mom = Engine(L, p, L, 1.0, 0.01, 1e-8, engine=engine).moments_states([f, half])
        print(f"  L {L} p {p}: {mom[0]}")
        assert mom[0][0] == 1.0 and not mom[0][[1, 2, 4, 5, 6]].any()
        # sqrt(2)^2 is one rounding above 2: 4 (L - 1) to rounding, and exactly 0 at p = 2
        assert abs(mom[0][3] - kk) <= 1e-14 * kk and (kk > 0 or mom[0][3] == 0.0)
        assert np.array_equal(mom[1], 0.25 * mom[0])
    # a doubly occupied site
    L, p, Q = 4, 3, 4
    d = MPS(L, p, Q, *R.fock(L, p, Q, [2, 0, 1, 1]))
    mom = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine).moments_states([d])[0]
    assert mom[0] == 1.0 and mom[2] == 1.0 and mom[4] == 1.0 and mom[1] == 0.0 and mom[5] == 0.0 and mom[6] == 0.0
    _check(mom[None], [d], "doubly occupied")


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("L,p,Q,U", [(5, 5, 5, 2.5), (5, 3, 5, 8.0)])
@pytest.mark.parametrize("path", PATHS)
def test_ed_ground_states(engine, L, p, Q, U, path, monkeypatch):
    from optimalcontrolmps_amd.native import MPS, Engine, energy, energy_variance
    _path(monkeypatch, path)
    J = 1.0
    psi, e0 = ed.ground_state_full(L, p, Q, J, U)
    st = MPS(L, p, Q, *ed.mps_from_full(psi, L, p, Q))
    mom = Engine(L, p, Q, J, 0.01, 1e-8, engine=engine).moments_states([st])[0]
    _check(mom[None], [st], f"{engine} {path}")
    n2, k1, d1, kk, dd, kdr, kdi = mom
    en, var = float(energy(mom, J, U)), float(energy_variance(mom, J, U))
    etol = TOL * (abs(J * k1) + abs(U * d1) + abs(e0) * n2) / n2
    vtol = TOL * (J * J * abs(kk) + 2 * abs(J * U * kdr) + U * U * abs(dd) + en * en) / n2
    print(f"  E - E0 = {en - e0:.3e} (tol {etol:.3e}), Var = {var:.3e} (tol {vtol:.3e}), kd_im = {kdi:.3e}")
    assert abs(en - e0) <= etol
    assert abs(var) <= vtol
    assert abs(kdi) <= TOL * E.tol_scale(mom)


# ------------------------------------------------------------ independence of the request
def _need(eng, t):
    """the chunk workspace one state's request takes, from the message of the OCG_ENOMEM it gets under a
    budget of one byte"""
    from optimalcontrolmps_amd.native import OcgError
    with pytest.raises(OcgError, match="ENOMEM") as ei:
        eng.moments(0, [t])
    return int(re.search(r"\((\d+) B\)", str(ei.value)).group(1))


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_results_do_not_depend_on_the_request(c1_runs, engine, path, monkeypatch):
    eng, _ = c1_runs(engine)
    _path(monkeypatch, path)
    every = eng.moments(0)
    assert every.shape == (C1["Nt"], 7)
    assert np.array_equal(eng.moments(0, [7]), every[7:8])
    pick = [20, 7, 7, 0, 13]
    assert np.array_equal(eng.moments(0, pick), every[pick])
    assert np.array_equal(eng.moments(0, list(range(C1["Nt"]))[::-1]), every[::-1])
    # every state in a chunk of its own
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    need = max(_need(eng, t) for t in (0, 10, 20))
    monkeypatch.setenv("OCG_OBS_BUDGET", str(need))
    split = eng.moments(0)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert np.array_equal(split, every)
    # host copies of the same states, staged
    if engine == "lds":  # (the compact format is the LDS engine's own block layout: the same operands)
        assert np.array_equal(eng.moments_states([eng.state(0, t) for t in (3, 20)]), every[[3, 20]])


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_moments_leave_the_device_state(states, engine):
    eng = _c1_engine(states, engine)
    H0, divT0, F0 = eng.hessian(C1_U)
    ps = eng.path_stats()
    eng.moments(0)
    eng.moments(1, [3, 3, 20])
    eng.moments(2, [5])
    assert eng.path_stats() == ps
    H, divT, F = eng.hessian(C1_U)
    assert np.array_equal(H, H0) and np.array_equal(divT, divT0) and F == F0


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_errors(states, engine, monkeypatch):
    from optimalcontrolmps_amd import native as nat
    eng = _c1_engine(states, engine)

    def fails(code, *a):
        with pytest.raises(nat.OcgError, match=code):
            eng.moments(*a)
    fails("ESTATE", 0, [0])                       # before any propagate
    eng.propagate(C1_U, 3)
    assert eng.moments(0, [0]).shape == (1, 7)
    fails("ESTATE", 2, [0])                       # no xi_dH yet
    for bad in ((0, [C1["Nt"]]), (0, [-1]), (3, [0]), (-1, [0])):
        fails("EINVAL", *bad)
        assert abs(eng.moments(0, [20])[0, 0] - 1) < 1e-6
    # nt == 0 writes nothing
    buf = np.full(7, 7.0)
    assert nat.lib().ocg_observe_moments(eng.h, 0, None, 0, buf.ctypes.data_as(nat.dp)) == 0 and (buf == 7).all()
    assert eng.moments(0, []).shape == (0, 7) and eng.moments_states([]).shape == (0, 7)
    # a budget too small for one state
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    fails("ENOMEM", 0, [3])
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert eng.moments(0, [3]).shape == (1, 7)
    assert nat.lib().ocg_abi_version() == 7
