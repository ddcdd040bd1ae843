"""ocg_sample / ocg_fock_amplitudes and their _states variants on the device
(csrc/observe_sample.hpp's kernel after csrc/observe.hpp's right sweep) on both
engines.  References: the dense state vector of the engine's own get_state
output where it is small (sample_reference.replay_dense: every decision of a
shot replayed against the exact conditionals for the same random number), else
the numpy restatement sample_ref, which test_sample_reference.py pins to the
state vector.

Exemption rule of every replay: a decision whose u lies within 1e-9 of a
normalised dense CDF boundary may fall on either side, the replay continues
with the drawn n, and at most one exempted decision per 1000 shots of a case.
Tolerances: logp 1e-10 absolute against the state vector, 1e-9 between the
engines and at chi = 256; amplitudes 1e-13 sqrt(norm2).
"""
import os
import re

import numpy as np
import pytest

import observe_reference as R
import sample_reference as SR
import spectrum_reference as S
from optimalcontrolmps_amd import ed
from test_observe_gpu import C1, C1_U, CHAINS, _c1_engine, _mps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261015


def _replay(out, e, m, seed, id, ltol=1e-10):
    """the shots of entry e against the state vector of the host state m"""
    cf, lp = out["config"][e], out["logp"][e]
    assert cf.dtype == np.int8 and (cf.sum(axis=1) == m.Q).all() and cf.min() >= 0 and cf.max() < m.p
    r = SR.replay_dense(R.dense_of(m), m.L, m.p, cf, lp, seed, id)
    assert r["mismatch"] == 0, r
    assert r["exempt"] * 1000 <= len(cf), r
    assert r["logp_dev"] <= ltol, r
    return r


def _worst(rs):
    return {"exempt": sum(r["exempt"] for r in rs), "logp_dev": max(r["logp_dev"] for r in rs),
            "min_dist": min(r["min_dist"] for r in rs)}


# ------------------------------------------------------------ config-1 shape
C1_TS = [0, 1, 10, 20]


@pytest.fixture(scope="module")
def c1_runs(states):
    """per engine: the context after propagate + xi_dH and 512 shots of psi_t, xi_t, xiH_t at C1_TS"""
    cache = {}

    def get(engine):
        if engine not in cache:
            eng = _c1_engine(states, engine)
            eng.propagate(C1_U, 3)
            eng.xi_dH()
            cache[engine] = (eng, [eng.sample(w, C1_TS, 512, SEED) for w in (0, 1, 2)])
        return cache[engine]
    return get


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_config1_shape_vs_state_vector(c1_runs, engine, which):
    eng, outs = c1_runs(engine)
    out = outs[which]
    assert out["config"].shape == (len(C1_TS), 512, C1["L"]) and out["logp"].shape == (len(C1_TS), 512)
    rs = [_replay(out, e, eng.state(which, t), SEED, t) for e, t in enumerate(C1_TS)]
    print(f"  {_worst(rs)}")


def test_engines_agree(c1_runs):
    ea, a = c1_runs("lds")
    _, b = c1_runs("hbm")
    for which in range(3):
        differ = 0
        for e, t in enumerate(C1_TS):
            psi = R.dense_of(ea.state(which, t))
            differ += SR.compare_configs(a[which]["config"][e], b[which]["config"][e], psi, C1["L"], C1["p"], SEED, t)
            same = (a[which]["config"][e] == b[which]["config"][e]).all(axis=1)
            assert np.abs(a[which]["logp"][e][same] - b[which]["logp"][e][same]).max() < 1e-9
        assert differ * 1000 <= 512 * len(C1_TS)


@pytest.mark.parametrize("L,p,Q,J,Ui,Uf", CHAINS)
def test_general_chains(states, L, p, Q, J, Ui, Uf):
    """empty sectors, L = 3 and odd block orders"""
    from optimalcontrolmps_amd.native import Engine
    eng = Engine(L, p, Q, J, 0.01, 1e-8)
    eng.set_states(_mps(states, L, p, Q, J, Uf), _mps(states, L, p, Q, J, Ui))
    eng.propagate(np.random.default_rng(7).uniform(2, 10, 9), 3)
    ts = [0, 4, 8]
    for which in (0, 1):
        out = eng.sample(which, ts, 256, 3)
        rs = [_replay(out, e, eng.state(which, t), 3, t) for e, t in enumerate(ts)]
        print(f"  which {which}: {_worst(rs)}")
        cf = SR.all_configs(L, p, Q)
        amp = eng.fock_amplitudes(which, ts, cf)
        for e, t in enumerate(ts):
            psi = R.dense_of(eng.state(which, t))
            assert np.abs(amp[e] - psi[[SR.flat_index(c, p) for c in cf]]).max() <= 1e-13 * np.linalg.norm(psi)


# ------------------------------------------------------------ caller-supplied states
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("lo,hi", [(1, 3), (17, 20), (63, 66)])
def test_random_complex_states(engine, lo, hi):
    """complex non-canonical states with sector orders on both sides of 16 and of the 64-lane wave"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 3, 4, 3
    rng = np.random.default_rng(5)
    sts = [MPS(L, p, Q, *S.random_mps(rng, L, p, Q, lo, hi)) for _ in range(2)]
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, 128, engine=engine)
    out = eng.sample_states(sts, 512, 9)
    cf = SR.all_configs(L, p, Q)
    amp = eng.fock_amplitudes_states(sts, cf)
    assert amp.shape == (2, len(cf)) and amp.dtype == np.complex128
    for e, m in enumerate(sts):
        print("  ", _replay(out, e, m, 9, e))
        psi = R.dense_of(m)
        n2 = float(np.vdot(psi, psi).real)
        dev = np.abs(amp[e] - psi[[SR.flat_index(c, p) for c in cf]]).max()
        print(f"   amplitudes: {dev / np.sqrt(n2):.3e} sqrt(norm2)")
        assert dev <= 1e-13 * np.sqrt(n2)
        assert abs((np.abs(amp[e]) ** 2).sum() - n2) <= 1e-12 * n2


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_packed_and_wide_kernels_agree(engine):
    """a state with sectors up to 3 wide alone (four shots per wave) and in a chunk with a state above 16 (one
    wave per shot): the same bits"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 3, 4, 3
    rng = np.random.default_rng(8)
    small = MPS(L, p, Q, *S.random_mps(rng, L, p, Q, 1, 3))
    edge = MPS(L, p, Q, *S.random_mps(rng, L, p, Q, 16, 16))
    big = MPS(L, p, Q, *S.random_mps(rng, L, p, Q, 17, 20))
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, 128, engine=engine)
    cf = SR.all_configs(L, p, Q)
    for m in (small, edge):
        alone, mixed = eng.sample_states([m], 203, 2), eng.sample_states([m, big], 203, 2)     # 203: a part-filled wave
        assert np.array_equal(alone["config"][0], mixed["config"][0])
        assert np.array_equal(alone["logp"][0], mixed["logp"][0])
        assert np.array_equal(eng.fock_amplitudes_states([m], cf)[0], eng.fock_amplitudes_states([m, big], cf)[0])
        _replay(alone, 0, m, 2, 0)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_hand_made_states(engine):
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 4, 3, 4
    occ = [2, 0, 1, 1]
    f = MPS(L, p, Q, *R.fock(L, p, Q, occ))
    h = f.copy()
    h.data[0] *= 2.0
    z = f.copy()
    z.data[:] = 0
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine)
    out = eng.sample_states([f, h, z], 64, 1)
    for e in range(2):
        assert (out["config"][e] == np.array(occ, np.int8)).all()
        assert np.array_equal(out["logp"][e], np.zeros(64))
    assert (out["config"][2] == -1).all() and np.isneginf(out["logp"][2]).all()
    amp = eng.fock_amplitudes_states([f, h, z], [occ, [1, 1, 1, 1]])
    assert np.array_equal(amp, np.array([[1, 0], [2, 0], [0, 0]], complex))
    # the W state of one boson on four sites, and the same state with a zero-padded sector
    L, p, Q = 4, 2, 1
    psi = np.zeros(p ** L, complex)
    for k in range(L):
        psi[p ** k] = 0.5
    dims, data = ed.mps_from_full(psi, L, p, Q)
    d2, x2 = S.pad_sector(dims, data, L, p, Q, 2, 1)
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine)
    w, wp = MPS(L, p, Q, dims, data), MPS(L, p, Q, d2, x2)
    out = eng.sample_states([w], 256, 4)
    pad = eng.sample_states([wp], 256, 4)
    assert (out["config"].sum(-1) == 1).all() and out["config"].min() == 0 and out["config"].max() == 1
    assert sorted(set(np.argmax(out["config"][0], axis=1))) == [0, 1, 2, 3]
    assert np.abs(out["logp"] - np.log(0.25)).max() < 1e-14
    assert np.array_equal(pad["config"], out["config"]) and np.abs(pad["logp"] - out["logp"]).max() < 1e-14
    _replay(out, 0, w, 4, 0)


def test_chi256_sample_states():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 20, 7, 20
    z = np.load(os.path.join(HERE, "golden", "c4_warm256.npz"), allow_pickle=False)
    m = MPS(L, p, Q, z["dims"], z["data"])
    assert max(m.bond_dims()) == 256
    eng = Engine(L, p, Q, 1.0, 0.005, 1e-8, 256, engine="hbm")
    ps = eng.path_stats()
    eng.reset_stats()
    out = eng.sample_states([m], 64, 5)
    assert eng.path_stats() == ps
    st = eng.stats(9)
    assert st["launches"] > 0 and st["alg_flops"] > 0 and st["alg_bytes"] > 0 and st["ms"] > 0
    assert st["launches"] == 2 * (L - 1) + 1     # the right sweep's two GEMM launches per site, then one launch
    ref = SR.sample_ref(m.dims, m.data, L, p, Q, 64, 5, 0)
    # replay against sample_ref on the same blocks: a shot that differs must differ first at a decision
    # whose u is within 1e-9 of a CDF boundary; sample_ref's own running sums are the boundaries here
    differ = np.flatnonzero((out["config"][0] != ref["config"]).any(axis=1))
    print(f"  shots that differ from sample_ref: {len(differ)}")
    assert len(differ) * 1000 <= 64
    same = np.setdiff1d(np.arange(64), differ)
    dev = np.abs(out["logp"][0][same] - ref["logp"][same]).max()
    print(f"  logp deviation {dev:.3e}")
    assert dev <= 1e-9
    assert (out["config"][0].sum(axis=1) == Q).all() and out["config"].min() >= 0 and out["config"].max() < p
    amp = eng.fock_amplitudes_states([m], out["config"][0])
    pr = np.abs(amp[0]) ** 2 / ref["norm2"]
    rel = np.abs(pr / np.exp(out["logp"][0]) - 1).max()
    print(f"  |amp|^2 / norm2 against exp(logp): {rel:.3e} relative")
    assert rel <= 1e-9
    assert eng.stats(9)["launches"] == 2 * (L - 1) + 2      # amplitudes: no right sweep, one launch


# ------------------------------------------------------------ determinism, isolation
def _need(eng, t):
    """the chunk workspace one state's request takes, from the message of the OCG_ENOMEM it gets under a
    budget of one byte"""
    from optimalcontrolmps_amd.native import OcgError
    with pytest.raises(OcgError, match="ENOMEM") as ei:
        eng.sample(0, [t], 512, SEED)
    return int(re.search(r"\((\d+) B\)", str(ei.value)).group(1))


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_results_do_not_depend_on_the_request(c1_runs, engine, monkeypatch):
    eng, outs = c1_runs(engine)
    full = outs[0]
    at = {t: e for e, t in enumerate(C1_TS)}

    def same(out, ts, n=512):
        for e, t in enumerate(ts):
            assert np.array_equal(out["config"][e], full["config"][at[t]][:n]), t
            if "logp" in out:
                assert np.array_equal(out["logp"][e], full["logp"][at[t]][:n]), t
    same(eng.sample(0, [10], 512, SEED), [10])
    same(eng.sample(0, [20, 10, 10, 0], 512, SEED), [20, 10, 10, 0])
    same(eng.sample(0, [20, 1], 100, SEED), [20, 1], 100)          # the first 100 shots
    nol = eng.sample(0, [1, 20], 512, SEED, logp=False)
    assert set(nol) == {"config"}
    same(nol, [1, 20])
    # which is not mixed in, the seed is
    assert not np.array_equal(eng.sample(0, [10], 512, SEED + 1)["config"][0], full["config"][at[10]])
    # a state among all the others, and every state in a chunk of its own
    every = eng.sample(0, None, 512, SEED)
    same({k: v[C1_TS] for k, v in every.items()}, C1_TS)
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    need = max(_need(eng, t) for t in range(C1["Nt"]))
    monkeypatch.setenv("OCG_OBS_BUDGET", str(need))
    split = eng.sample(0, None, 512, SEED)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert np.array_equal(split["config"], every["config"]) and np.array_equal(split["logp"], every["logp"])
    # amplitudes: alone, repeated, split
    cf = SR.all_configs(C1["L"], C1["p"], C1["Q"])
    amps = eng.fock_amplitudes(0, None, cf)
    # one wave per shot instead of four shots per wave (every sector here is at most 16 wide)
    monkeypatch.setenv("OCG_OBS_SAMPLE_PACK", "0")
    same(eng.sample(0, C1_TS, 512, SEED), C1_TS)
    assert np.array_equal(eng.fock_amplitudes(0, None, cf), amps)
    monkeypatch.delenv("OCG_OBS_SAMPLE_PACK")
    assert np.array_equal(eng.fock_amplitudes(0, [20, 7, 7], cf[5:9]), amps[[20, 7, 7], 5:9])
    n2 = eng.observe(0, None, (), outputs=("norm2",))["norm2"]
    assert np.abs((np.abs(amps) ** 2).sum(axis=1) - n2).max() <= 1e-12


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_sampling_leaves_the_device_state(states, engine):
    eng = _c1_engine(states, engine)
    eng.propagate(C1_U, 3)

    def snap():
        return [eng.fidelities(), eng.div_t()] + [eng.state(w, t).data for w in (0, 1) for t in (0, 9, 20)]
    before = snap()
    ps = eng.path_stats()
    eng.sample(0, None, 64, 1)
    eng.sample(1, [3, 3, 20], 16, 2)
    eng.fock_amplitudes(0, [5], [[1, 1, 1, 1, 1]])
    assert all(np.array_equal(a, b) for a, b in zip(before, snap()))
    assert eng.path_stats() == ps
    H, divT, F = eng.hessian(C1_U)
    fresh = _c1_engine(states, engine)
    H2, divT2, F2 = fresh.hessian(C1_U)
    assert np.array_equal(H, H2) and np.array_equal(divT, divT2) and F == F2


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_errors(states, engine, monkeypatch):
    from optimalcontrolmps_amd import native as nat
    eng = _c1_engine(states, engine)
    mott = [[1] * C1["L"]]

    def fails(code, f, *a):
        with pytest.raises(nat.OcgError, match=code):
            f(*a)
    fails("ESTATE", eng.sample, 0, [0], 4, 1)                   # before any propagate
    fails("ESTATE", eng.fock_amplitudes, 0, [0], mott)
    eng.propagate(C1_U, 3)
    assert eng.sample(0, [0], 4, 1)["config"].shape == (1, 4, C1["L"])
    fails("ESTATE", eng.sample, 2, [0], 4, 1)                   # no xi_dH yet
    for bad in ((0, [C1["Nt"]], 4, 1), (0, [-1], 4, 1), (3, [0], 4, 1), (0, [0], -1, 1)):
        fails("EINVAL", eng.sample, *bad)
        assert eng.sample(1, [4], 2, 1)["logp"].shape == (1, 2)
    for bad in ([[1, 1, 1, 1, 5]], [[1, 1, 1, 1, -1]], [[1, 1, 1, 1, 2]], [[1] * 5, [0, 0, 0, 0, 4]]):
        fails("EINVAL", eng.fock_amplitudes, 0, [0], bad)
    fails("EINVAL", eng.fock_amplitudes, 0, [C1["Nt"]], mott)
    # nothing requested: success, nothing written
    cfg, lp, amp = np.full((1, 3, C1["L"]), 7, np.int8), np.full((1, 3), 7.0), np.full((1, 1, 2), 7.0)
    ts = np.array([3], np.int32)
    assert nat.lib().ocg_sample(eng.h, 0, ts.ctypes.data_as(nat.ip), 1, 0, 1, cfg.ctypes.data_as(nat.bp),
                                lp.ctypes.data_as(nat.dp)) == 0
    assert nat.lib().ocg_fock_amplitudes(eng.h, 0, ts.ctypes.data_as(nat.ip), 1, None, 0,
                                         amp.ctypes.data_as(nat.dp)) == 0
    assert (cfg == 7).all() and (lp == 7).all() and (amp == 7).all()
    assert eng.sample(0, [3], 0, 1)["config"].shape == (1, 0, C1["L"])
    assert eng.fock_amplitudes(0, [3], np.zeros((0, C1["L"]), np.int8)).shape == (1, 0)
    # a budget too small for one state
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    fails("ENOMEM", eng.sample, 0, [3], 4, 1)
    fails("ENOMEM", eng.fock_amplitudes, 0, [3], mott)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert eng.fock_amplitudes(0, [20], mott).shape == (1, 1)
