"""ocg_observe / ocg_observe_states on the device (csrc/observe.hpp) on both
engines.  Every reference is taken from the engine's own get_state output (the
dense state vector where it is small, else the numpy restatement of
observe_reference.py, which test_observe_reference.py pins to the state
vector), so a bond dimension that differs from the oracle's cannot matter.

Tolerances: 1e-10 against the state vector (that of test_observables.py),
1e-9 between the engines and at chi = 256 (the project's trajectory-level
tolerance); sum rules to 1e-10 relative to the norm.
"""
import os

import numpy as np
import pytest

import observe_reference as R
from conftest import state_key
from optimalcontrolmps_amd import ed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("norm2", "occ", "ada", "nn")


def _mps(states, L, p, Q, J, U):
    from optimalcontrolmps_amd.native import MPS
    k = state_key(L, p, Q, J, U)
    return MPS(L, p, Q, states[k + "/dims"], states[k + "/data"])


def _dense_ref(eng, which, ts, rows):
    """the observables of the engine's own states from their state vectors, stacked over ts"""
    per = []
    for t in ts:
        m = eng.state(which, t)
        d = R.observe_dense(R.dense_of(m), eng.L, eng.p, rows)
        d["bond"] = m.bond_dims()
        per.append(d)
    return {k: np.stack([np.asarray(d[k]) for d in per]) for k in KEYS + ("bond",)}


def _block_ref(states, rows):
    per = [R.observe_ref(m.dims, m.data, m.L, m.p, m.Q, rows) for m in states]
    return {k: np.stack([np.asarray(d[k]) for d in per]) for k in KEYS + ("bond",)}


def _sum_rules(out, Q, rel=1e-10):
    scale = np.maximum(np.abs(out["norm2"]), 1e-300)
    assert (np.abs(out["occ"].sum(-1) - out["norm2"][:, None]) <= rel * scale[:, None]).all()
    ntot = (np.arange(out["occ"].shape[-1]) * out["occ"]).sum((-1, -2))
    assert (np.abs(ntot - Q * out["norm2"]) <= rel * Q * scale).all()


def _check(out, ref, tol):
    for k in KEYS:
        dev = float(np.abs(out[k] - ref[k]).max()) if ref[k].size else 0.0
        print(f"  {k}: max deviation {dev:.3e} (tol {tol:g})")
        assert dev < tol, k
    assert np.array_equal(out["bond"], ref["bond"])


# ------------------------------------------------------------ config-1 shape
C1 = dict(L=5, p=5, Q=5, J=1.0, dt=0.01, cut=1e-8, maxm=80, Nt=21)


def _c1_engine(states, engine):
    from optimalcontrolmps_amd.native import Engine
    c = C1
    eng = Engine(c["L"], c["p"], c["Q"], c["J"], c["dt"], c["cut"], c["maxm"], engine=engine)
    eng.set_states(_mps(states, c["L"], c["p"], c["Q"], c["J"], 50.0), _mps(states, c["L"], c["p"], c["Q"], c["J"], 2.5))
    return eng


C1_U = np.linspace(2.5, 50.0, C1["Nt"])
C1_ROWS = list(range(1, C1["L"] + 1))


@pytest.fixture(scope="module")
def c1_runs(states):
    """per engine: the context after propagate + xi_dH and its all-t, all-rows observables"""
    cache = {}

    def get(engine):
        if engine not in cache:
            eng = _c1_engine(states, engine)
            eng.propagate(C1_U, 3)
            eng.xi_dH()
            cache[engine] = (eng, [eng.observe(w, None, C1_ROWS) for w in (0, 1, 2)])
        return cache[engine]
    return get


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_config1_shape_vs_state_vector(c1_runs, engine, which):
    """GPU tests 1 and 5 of the feature: psi_t, xi_t and xiH_t, all t, all rows, against the
    state vectors of the engine's own states to 1e-10"""
    eng, outs = c1_runs(engine)
    out = outs[which]
    ref = _dense_ref(eng, which, range(C1["Nt"]), C1_ROWS)
    _check(out, ref, 1e-10)
    _sum_rules(out, C1["Q"])
    assert out["ada"].shape == (C1["Nt"], C1["L"], C1["L"]) and out["ada"].dtype == np.complex128
    # entries j < i are written as 0, diagonals are real
    for i in range(C1["L"]):
        assert not out["ada"][:, i, :i].any() and not out["nn"][:, i, :i].any()
        assert not out["ada"][:, i, i].imag.any()
    if which < 2:
        assert np.abs(out["norm2"] - 1).max() < 1e-6  # cutoff 1e-8 per truncation


def test_engines_agree(c1_runs):
    """the two engines' numbers at the trajectory-level tolerance"""
    _, a = c1_runs("lds")
    _, b = c1_runs("hbm")
    for which in range(3):
        for k in KEYS:
            assert np.abs(a[which][k] - b[which][k]).max() < 1e-9 * max(1.0, float(np.abs(b[which][k]).max())), (which, k)


CHAINS = [(5, 6, 5, 1.0, 2.0, 12.0), (3, 4, 3, 2.0, 2.0, 12.0), (4, 3, 4, 1.0, 2.0, 10.0)]


@pytest.mark.parametrize("L,p,Q,J,Ui,Uf", CHAINS)
def test_general_chains(states, L, p, Q, J, Ui, Uf):
    """L = 3 (centre on site 2 = L - 1) and p - 1 < Q (empty sectors, missing (q, n + 1) partners)"""
    from optimalcontrolmps_amd.native import Engine
    eng = Engine(L, p, Q, J, 0.01, 1e-8)
    eng.set_states(_mps(states, L, p, Q, J, Uf), _mps(states, L, p, Q, J, Ui))
    u = np.random.default_rng(7).uniform(2, 10, 9)
    eng.propagate(u, 3)
    rows = list(range(1, L + 1))
    for which in (0, 1):
        out = eng.observe(which, None, rows)
        _check(out, _dense_ref(eng, which, range(9), rows), 1e-10)
        _sum_rules(out, Q)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_observe_leaves_the_device_state(states, engine):
    eng = _c1_engine(states, engine)
    eng.propagate(C1_U, 3)

    def snap():
        return [eng.fidelities(), eng.div_t()] + [eng.state(w, t).data for w in (0, 1) for t in (0, 9, 20)]
    before = snap()
    ps = eng.path_stats()
    eng.observe(0, None, C1_ROWS)
    eng.observe(1, [3, 3, 20], [2])
    assert all(np.array_equal(a, b) for a, b in zip(before, snap()))
    assert eng.path_stats() == ps
    H, divT, F = eng.hessian(C1_U)
    fresh = _c1_engine(states, engine)
    H2, divT2, F2 = fresh.hessian(C1_U)
    assert np.array_equal(H, H2) and np.array_equal(divT, divT2) and F == F2


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_results_do_not_depend_on_the_request(c1_runs, engine, monkeypatch):
    eng, outs = c1_runs(engine)
    full = outs[0]
    one = eng.observe(0, [7], [2])
    for k in KEYS + ("bond",):
        want = full[k][7:8] if full[k].ndim < 3 or k == "occ" else full[k][7:8, 1:2]
        assert np.array_equal(one[k], want), k
    rep = eng.observe(0, [20, 7, 7], [2])
    for k in KEYS + ("bond",):
        f = full[k] if full[k].ndim < 3 or k == "occ" else full[k][:, 1:2]
        assert np.array_equal(rep[k], f[[20, 7, 7]]), k
    # another chunking (here: every state a chunk of its own) changes no bit
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    split = eng.observe(0, None, C1_ROWS)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    for k in KEYS + ("bond",):
        assert np.array_equal(split[k], full[k]), k
    # an output that is not asked for changes nothing in the others
    from optimalcontrolmps_amd import native as nat
    n2 = np.zeros(1)
    ts = np.array([7], np.int32)
    eng._chk(nat.lib().ocg_observe(eng.h, 0, ts.ctypes.data_as(nat.ip), 1, None, 0, n2.ctypes.data_as(nat.dp), None,
                                   None, None, None), "ocg_observe")
    assert n2[0] == full["norm2"][7]


def test_hbm_across_the_mfma_tile_edge():
    """sectors above 16 rows (k_gemm's 16 x 16 MFMA sub-tile, its 32 x 32 tile partly filled)"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 10, 4, 10
    f = MPS(L, p, Q, *R.fock(L, p, Q, [1] * L))
    eng = Engine(L, p, Q, 1.0, 0.03, 1e-10, 128, engine="hbm")
    eng.set_states(f, f)
    eng.propagate(np.linspace(2.0, 6.0, 31), 1)
    ts, rows = [0, 1, 15, 30], [1, 5, 10]
    sts = [eng.state(0, t) for t in ts]
    assert sts[-1].dims.max() > 16
    out = eng.observe(0, ts, rows)
    _check(out, _block_ref(sts, rows), 1e-10)
    _sum_rules(out, Q)
    # the Fock state itself: exact 0 / 1 occupations, an exactly diagonal a+a
    assert np.array_equal(out["occ"][0], np.tile(np.eye(p)[1], (L, 1)))
    want = np.zeros((len(rows), L), complex)
    for ri, i in enumerate(rows):
        want[ri, i - 1] = 1.0
    assert np.array_equal(out["ada"][0], want)


def test_chi256_observe_states():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 20, 7, 20
    z = np.load(os.path.join(HERE, "golden", "c4_warm256.npz"), allow_pickle=False)
    c4 = np.load(os.path.join(HERE, "golden", "c4.npz"), allow_pickle=False)
    sts = [MPS(L, p, Q, z["dims"], z["data"]), MPS(L, p, Q, c4["w256h/tgt_dims"], c4["w256h/tgt_data"])]
    assert max(sts[0].bond_dims()) == 256
    eng = Engine(L, p, Q, 1.0, 0.005, 1e-8, 256, engine="hbm")
    ps = eng.path_stats()
    out = eng.observe_states(sts, [10])
    assert eng.path_stats() == ps
    _check(out, _block_ref(sts, [10]), 1e-9)
    _sum_rules(out, Q)
    st = eng.stats(9)
    assert st["launches"] > 0 and st["alg_flops"] > 0 and st["alg_bytes"] > 0 and st["ms"] > 0
    eng.reset_stats()
    assert eng.stats(9) == {"ms": 0.0, "launches": 0, "alg_bytes": 0.0, "alg_flops": 0.0, "sweep_steps": 0}


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_hand_made_states(engine):
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 4, 3, 4
    occ = [2, 0, 1, 1]
    f = MPS(L, p, Q, *R.fock(L, p, Q, occ))
    h = f.copy()
    h.data[0] *= 0.5
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine)
    rows = list(range(1, L + 1))
    out = eng.observe_states([f, h], rows)
    assert np.array_equal(out["norm2"], [1.0, 0.25])
    assert np.array_equal(out["occ"][0], np.eye(p)[occ])
    n = np.array(occ, float)
    assert np.array_equal(out["nn"][0], np.triu(np.outer(n, n)))
    assert np.array_equal(out["ada"][0], np.diag(n))
    for k in KEYS:
        assert np.array_equal(out[k][1], 0.25 * out[k][0]), k
    assert np.array_equal(out["bond"], np.ones((2, L + 1), np.int32))
    # more states than one staging batch holds
    many = eng.observe_states([f, h, h] * 30, [1], outputs=("norm2", "nn"))
    assert set(many) == {"norm2", "nn"}
    assert np.array_equal(many["norm2"], [1.0, 0.25, 0.25] * 30)
    assert np.array_equal(many["nn"][:, 0], np.outer([1.0, 0.25, 0.25] * 30, np.triu(np.outer(n, n))[0]))
    # the W state of one boson on four sites: rho_ij = 1/4 for all i <= j, <n_i n_j> = 0 off the diagonal
    L, p, Q = 4, 2, 1
    psi = np.zeros(p ** L, complex)
    for k in range(L):
        psi[p ** k] = 0.5
    w = MPS(L, p, Q, *ed.mps_from_full(psi, L, p, Q))
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine)
    out = eng.observe_states([w], rows)
    assert abs(out["norm2"][0] - 1) < 1e-14
    assert np.abs(out["ada"][0] - 0.25 * np.triu(np.ones((L, L)))).max() < 1e-14
    assert np.abs(out["nn"][0] - 0.25 * np.eye(L)).max() < 1e-14
    assert np.abs(out["occ"][0] - [0.75, 0.25]).max() < 1e-14


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_errors(states, engine, monkeypatch):
    from optimalcontrolmps_amd.native import OcgError
    eng = _c1_engine(states, engine)

    def fails(code, *a):
        with pytest.raises(OcgError, match=code):
            eng.observe(*a)
    fails("ESTATE", 0, [0], [1])                      # before any propagate
    eng.propagate(C1_U, 3)
    assert eng.observe(0, [0], [1])["norm2"].shape == (1,)
    fails("ESTATE", 2, [0], [1])                      # no xi_dH yet
    assert eng.observe(1, [4], [])["occ"].shape == (1, 5, 5)
    for bad in ((0, [C1["Nt"]], [1]), (0, [-1], [1]), (0, [0], [0]), (0, [0], [C1["L"] + 1]), (3, [0], [1])):
        fails("EINVAL", *bad)
        ok = eng.observe(0, [20], [5])
        assert abs(ok["norm2"][0] - 1) < 1e-6 and ok["ada"].shape == (1, 1, 5)
    if engine == "hbm":                               # a meet-in-the-middle gradient keeps no trajectories
        monkeypatch.setenv("OCG_HBM_MID", "1")
        eng.gradient(C1_U)
        fails("ESTATE", 0, [0], [1])
        monkeypatch.delenv("OCG_HBM_MID")
        eng.propagate(C1_U, 3)
        assert abs(eng.observe(0, [20], [])["norm2"][0] - 1) < 1e-6
