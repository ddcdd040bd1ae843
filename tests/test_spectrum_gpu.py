"""ocg_observe_spectrum / ocg_observe_spectrum_states on the device (the
spectrum stages of csrc/observe.hpp on csrc/observe_eig.hpp's kernels) on both
engines.  References: the singular values of the dense state vector of the
engine's own get_state output where it is small (spectrum_dense), else the
numpy block formula (spectrum_ref), which test_spectrum_reference.py pins to
the state vector.

Tolerances: weights 1e-10 * norm2 and entropies 1e-9 against the state vector
(those of test_observe_gpu.py and test_observables.py), 1e-9 between the
engines and at chi = 256; sum rule to 1e-10 relative to norm2.
"""
import os

import numpy as np
import pytest

import observe_reference as R
import spectrum_reference as S
from optimalcontrolmps_amd import ed
from test_observe_gpu import C1, C1_U, CHAINS, _c1_engine, _mps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("entropy", "schmidt", "sector")


def _check_dense(out, e, m, wtol=1e-10, stol=1e-9):
    """entry e of a spectrum() result against the state vector of the host state m"""
    den = S.spectrum_dense(R.dense_of(m), m.L, m.p)
    wdev = max(S.weight_dev(out["schmidt"][e, b], den["weights"][b]) for b in range(m.L - 1))
    sdev = float(np.abs(out["entropy"][e] - den["entropy"]).max())
    assert wdev <= wtol * den["norm2"], (e, wdev, den["norm2"])
    assert sdev <= stol, (e, sdev)
    return wdev / den["norm2"], sdev


def _check_layout(out, e, m, norm2=None):
    """padding, sector counts, ordering and the sum rule of entry e for the host state m"""
    dims = m.dims.reshape(m.L + 1, m.Q + 1)
    for b in range(1, m.L):
        w, s = out["schmidt"][e, b - 1], out["sector"][e, b - 1]
        nb = int(dims[b].sum())
        assert (s[:nb] >= 0).all() and (s[nb:] == -1).all() and not w[nb:].any()
        assert np.array_equal(np.bincount(s[:nb], minlength=m.Q + 1), dims[b])
        assert (np.diff(w[:nb]) <= 0).all()
        ties = np.flatnonzero(np.diff(w[:nb]) == 0)
        assert (s[ties] <= s[ties + 1]).all()
        if norm2 is not None:
            assert abs(w.sum() - norm2) <= 1e-10 * abs(norm2), (e, b, w.sum(), norm2)


def _same(a, b, keys=KEYS):
    """bit-identical up to the padding width"""
    for k in keys:
        x, y = a[k], b[k]
        if k != "entropy":
            w = min(x.shape[-1], y.shape[-1])
            pad = -1 if k == "sector" else 0
            assert (x[..., w:] == pad).all() and (y[..., w:] == pad).all()
            x, y = x[..., :w], y[..., :w]
        assert np.array_equal(x, y), k


# ------------------------------------------------------------ config-1 shape
@pytest.fixture(scope="module")
def c1_runs(states):
    """per engine: the context after propagate + xi_dH, its spectra and its norms / bond dimensions"""
    cache = {}

    def get(engine):
        if engine not in cache:
            eng = _c1_engine(states, engine)
            eng.propagate(C1_U, 3)
            eng.xi_dH()
            cache[engine] = (eng, [eng.spectrum(w) for w in (0, 1, 2)],
                             [eng.observe(w, None, (), outputs=("norm2", "bond")) for w in (0, 1, 2)])
        return cache[engine]
    return get


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_config1_shape_vs_state_vector(c1_runs, engine, which):
    eng, outs, obs = c1_runs(engine)
    out = outs[which]
    nt, nb = C1["Nt"], C1["L"] - 1
    assert out["entropy"].shape == (nt, nb) and out["schmidt"].shape[:2] == (nt, nb)
    assert out["schmidt"].shape == out["sector"].shape and out["sector"].dtype == np.int32
    assert out["schmidt"].shape[2] == obs[which]["bond"].max()
    worst = (0.0, 0.0)
    for t in range(nt):
        m = eng.state(which, t)
        worst = max(worst, _check_dense(out, t, m))
        _check_layout(out, t, m, obs[which]["norm2"][t])
        assert np.array_equal((out["sector"][t] >= 0).sum(-1), obs[which]["bond"][t, 1:-1])
    print(f"  worst weight deviation / norm2, entropy deviation: {worst}")


def test_engines_agree(c1_runs):
    _, a, _ = c1_runs("lds")
    _, b, _ = c1_runs("hbm")
    for which in range(3):
        w = max(a[which]["schmidt"].shape[2], b[which]["schmidt"].shape[2])
        pad = lambda x: np.pad(x, ((0, 0), (0, 0), (0, w - x.shape[2])))
        assert np.abs(pad(a[which]["schmidt"]) - pad(b[which]["schmidt"])).max() < 1e-9
        assert np.abs(a[which]["entropy"] - b[which]["entropy"]).max() < 1e-9


@pytest.mark.parametrize("L,p,Q,J,Ui,Uf", CHAINS)
def test_general_chains(states, L, p, Q, J, Ui, Uf):
    """empty sectors, L = 3 and odd block orders"""
    from optimalcontrolmps_amd.native import Engine
    eng = Engine(L, p, Q, J, 0.01, 1e-8)
    eng.set_states(_mps(states, L, p, Q, J, Uf), _mps(states, L, p, Q, J, Ui))
    eng.propagate(np.random.default_rng(7).uniform(2, 10, 9), 3)
    for which in (0, 1):
        out = eng.spectrum(which)
        n2 = eng.observe(which, None, (), outputs=("norm2",))["norm2"]
        for t in range(9):
            m = eng.state(which, t)
            _check_dense(out, t, m)
            _check_layout(out, t, m, n2[t])


# ------------------------------------------------------------ caller-supplied states
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("L,p,Q,lo,hi", [(5, 4, 5, 1, 3), (4, 4, 4, 17, 20), (3, 4, 3, 63, 66)])
def test_random_complex_states(engine, L, p, Q, lo, hi):
    """a complex, non-identity Renv (the conj question), orders across the 16-row MFMA tile, and orders on
    both sides of the LDS / global-memory switch-over (64)"""
    from optimalcontrolmps_amd.native import MPS, Engine
    rng = np.random.default_rng(5)
    sts = [MPS(L, p, Q, *S.random_mps(rng, L, p, Q, lo, hi)) for _ in range(2)]
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, 128, engine=engine)
    out = eng.spectrum_states(sts)
    n2 = [S.spectrum_dense(R.dense_of(m), L, p)["norm2"] for m in sts]
    for e, m in enumerate(sts):
        print("  ", _check_dense(out, e, m))
        _check_layout(out, e, m, n2[e])
    if hi <= 3:  # the wrong formula is far outside the tolerance: this case can tell
        wrong = S.spectrum_ref(sts[0].dims, sts[0].data, L, p, Q, conj_renv=True)
        assert max(S.weight_dev(out["schmidt"][0, b], wrong["weights"][b]) for b in range(L - 1)) > 1e-3 * n2[0]


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_hand_made_states(engine):
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 4, 3, 4
    occ = [2, 0, 1, 1]
    f = MPS(L, p, Q, *R.fock(L, p, Q, occ))
    h = f.copy()
    h.data[0] *= 0.5
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine)
    out = eng.spectrum_states([f, h])
    assert out["schmidt"].shape == (2, L - 1, 1)
    assert np.array_equal(out["schmidt"][0], np.ones((L - 1, 1))) and np.array_equal(out["schmidt"][1],
                                                                                     np.full((L - 1, 1), 0.25))
    assert np.array_equal(out["entropy"], np.zeros((2, L - 1)))
    for e in range(2):
        assert np.array_equal(out["sector"][e, :, 0], np.cumsum(occ)[:-1])
    # the W state of one boson on four sites
    L, p, Q = 4, 2, 1
    psi = np.zeros(p ** L, complex)
    for k in range(L):
        psi[p ** k] = 0.5
    dims, data = ed.mps_from_full(psi, L, p, Q)
    d2, x2 = S.pad_sector(dims, data, L, p, Q, 2, 1)
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, engine=engine)
    out = eng.spectrum_states([MPS(L, p, Q, dims, data), MPS(L, p, Q, d2, x2)])
    assert out["schmidt"].shape == (2, L - 1, 3)
    for b in range(1, L):
        wl, wr = (L - b) / L, b / L                      # sector 0, sector 1
        want = sorted([(wl, 0), (wr, 1)], key=lambda x: (-x[0], x[1]))
        sref = -sum(x * np.log(x) for x in (wl, wr))
        for e in range(2):
            assert np.abs(out["schmidt"][e, b - 1, :2] - [x[0] for x in want]).max() < 1e-14
            if wl != wr:                                 # (equal weights may differ in the last bit)
                assert np.array_equal(out["sector"][e, b - 1, :2], [x[1] for x in want])
            assert sorted(out["sector"][e, b - 1, :2]) == [0, 1]
            assert abs(out["entropy"][e, b - 1] - sref) < 1e-14
    assert not out["schmidt"][0, :, 2].any() and (out["sector"][0, :, 2] == -1).all()
    # the padded sector: one more weight at bond 2, numerically zero, in sector 1
    assert abs(out["schmidt"][1, 1, 2]) <= 1e-15 and out["sector"][1, 1, 2] == 1
    assert (out["sector"][1, [0, 2], 2] == -1).all()
    assert np.array_equal((out["sector"][1] >= 0).sum(-1), [2, 3, 2])


def test_hbm_above_16_rows_on_a_physical_state():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 10, 4, 10
    f = MPS(L, p, Q, *R.fock(L, p, Q, [1] * L))
    eng = Engine(L, p, Q, 1.0, 0.03, 1e-10, 128, engine="hbm")
    eng.set_states(f, f)
    eng.propagate(np.linspace(2.0, 6.0, 31), 1)
    ts = [0, 15, 30]
    sts = [eng.state(0, t) for t in ts]
    assert sts[-1].dims.max() > 16
    out = eng.spectrum(0, ts)
    n2 = eng.observe(0, ts, (), outputs=("norm2",))["norm2"]
    for e, m in enumerate(sts):
        ref = S.spectrum_ref(m.dims, m.data, L, p, Q)
        w, s = S.padded(ref, out["schmidt"].shape[2])
        assert np.abs(out["schmidt"][e] - w).max() < 1e-10
        assert np.abs(out["entropy"][e] - ref["entropy"]).max() < 1e-10
        _check_layout(out, e, m, n2[e])
    assert np.array_equal(out["schmidt"][0, :, 0], np.ones(L - 1)) and not out["entropy"][0].any()
    assert np.array_equal(out["sector"][0, :, 0], np.arange(1, L))


def test_chi256_spectrum_states():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 20, 7, 20
    z = np.load(os.path.join(HERE, "golden", "c4_warm256.npz"), allow_pickle=False)
    c4 = np.load(os.path.join(HERE, "golden", "c4.npz"), allow_pickle=False)
    sts = [MPS(L, p, Q, z["dims"], z["data"]), MPS(L, p, Q, c4["w256h/tgt_dims"], c4["w256h/tgt_data"])]
    assert max(sts[0].bond_dims()) == 256
    assert max(int(m.dims.max()) for m in sts) >= 32
    eng = Engine(L, p, Q, 1.0, 0.005, 1e-8, 256, engine="hbm")
    ps = eng.path_stats()
    eng.reset_stats()
    out = eng.spectrum_states(sts)
    assert eng.path_stats() == ps
    st = eng.stats(9)
    assert st["launches"] > 0 and st["alg_flops"] > 0 and st["alg_bytes"] > 0 and st["ms"] > 0
    for e, m in enumerate(sts):
        ref = S.spectrum_ref(m.dims, m.data, L, p, Q)
        w, s = S.padded(ref, out["schmidt"].shape[2])
        wdev, sdev = np.abs(out["schmidt"][e] - w).max(), np.abs(out["entropy"][e] - ref["entropy"]).max()
        print(f"  state {e}: weights {wdev / ref['norm2']:.3e} of norm2, entropy {sdev:.3e}")
        assert wdev <= 1e-9 * ref["norm2"] and sdev <= 1e-9
        _check_layout(out, e, m, ref["norm2"])
    # one chunk: the two sweeps (2 GEMM launches per site, no closes), then both eigen stages (orders
    # <= 16 and above: two launches each), their two GEMM launches and the entropy reduction
    assert st["launches"] == 2 * (L - 1) + 2 * L + 2 + 2 + 2 + 1


# ------------------------------------------------------------ paths, determinism, isolation
@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_global_memory_path(c1_runs, engine, monkeypatch):
    eng, outs, _ = c1_runs(engine)
    monkeypatch.setenv("OCG_OBS_EIG_LDS_MAX", "0")
    glob = eng.spectrum(0)
    monkeypatch.delenv("OCG_OBS_EIG_LDS_MAX")
    assert np.abs(glob["schmidt"] - outs[0]["schmidt"]).max() <= 1e-12
    assert np.abs(glob["entropy"] - outs[0]["entropy"]).max() <= 1e-12
    for t in range(C1["Nt"]):
        _check_dense(glob, t, eng.state(0, t))


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_results_do_not_depend_on_the_request(c1_runs, engine, monkeypatch):
    eng, outs, _ = c1_runs(engine)
    full = outs[0]
    _same(eng.spectrum(0, [7]), {k: full[k][7:8] for k in KEYS})
    _same(eng.spectrum(0, [20, 7, 7]), {k: full[k][[20, 7, 7]] for k in KEYS})
    for k in KEYS:
        one = eng.spectrum(0, [7], outputs=(k,))
        assert set(one) == {k}
        _same(one, {k: full[k][7:8]}, (k,))
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    split = eng.spectrum(0)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    _same(split, full)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_spectrum_leaves_the_device_state(states, engine):
    eng = _c1_engine(states, engine)
    eng.propagate(C1_U, 3)

    def snap():
        obs = eng.observe(0, None, [1, 3])
        return [eng.fidelities(), eng.div_t()] + [eng.state(w, t).data for w in (0, 1) for t in (0, 9, 20)] + \
            [obs[k] for k in sorted(obs)]
    before = snap()
    ps = eng.path_stats()
    eng.spectrum(0)
    eng.spectrum(1, [3, 3, 20], outputs=("entropy",))
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

    def fails(code, *a):
        with pytest.raises(nat.OcgError, match=code):
            eng.spectrum(*a)
    fails("ESTATE", 0, [0])                              # before any propagate
    eng.propagate(C1_U, 3)
    assert eng.spectrum(0, [0])["entropy"].shape == (1, C1["L"] - 1)
    fails("ESTATE", 2, [0])                              # no xi_dH yet
    for bad in ((0, [C1["Nt"]]), (0, [-1]), (3, [0])):
        fails("EINVAL", *bad)
        assert eng.spectrum(1, [4])["entropy"].shape == (1, C1["L"] - 1)
    # wcap one below the largest bond dimension: ECAP with weights, fine without
    ts = np.array([10, 20], np.int32)
    wcap = int(eng.observe(0, ts, (), outputs=("bond",))["bond"].max())
    nb = C1["L"] - 1
    ent, w, s = np.zeros((2, nb)), np.zeros((2, nb, wcap)), np.zeros((2, nb, wcap), np.int32)
    call = lambda cap, pw, psec: nat.lib().ocg_observe_spectrum(
        eng.h, 0, ts.ctypes.data_as(nat.ip), 2, cap, ent.ctypes.data_as(nat.dp), pw, psec)
    assert call(wcap, w.ctypes.data_as(nat.dp), s.ctypes.data_as(nat.ip)) == 0
    assert nat.OCG_ERRORS[call(wcap - 1, w.ctypes.data_as(nat.dp), None)] == "ECAP"
    assert nat.OCG_ERRORS[call(wcap - 1, None, s.ctypes.data_as(nat.ip))] == "ECAP"
    e0 = ent.copy()
    ent[:] = 0
    assert call(wcap - 1, None, None) == 0 and np.array_equal(ent, e0)
    if engine == "hbm":                                  # a meet-in-the-middle gradient keeps no trajectories
        monkeypatch.setenv("OCG_HBM_MID", "1")
        eng.gradient(C1_U)
        fails("ESTATE", 0, [0])
        monkeypatch.delenv("OCG_HBM_MID")
        eng.propagate(C1_U, 3)
        assert eng.spectrum(0, [20])["entropy"].shape == (1, C1["L"] - 1)
