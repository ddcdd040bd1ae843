"""ocg_observe_pairs / ocg_observe_pairs_states on the device (csrc/observe_pair.hpp) on
both engines and on both paths: the chain kernel k_obs_pair (pairs whose bond sectors
are all at most 16 wide, both states) and the task-list path (OCG_OBS_PAIR_CHAIN=0
forces it).  Reference: pair_reference.pairs_ref on the engine's own get_state output
or on the host states, which test_pair_reference.py pins to the dense numbers.

Tolerance: TOL = 1e-10, the project's observable tolerance, relative to
sqrt(<x|x><y|y>) c with c = 1 for ovl and occ and c = p - 1 (the largest |<m|a+ a|n>|)
for hop.

Sensitivities against finite differences of the cost (L = p = Q = 5, N_t = 21, the ramp
of FD_U below), measured on an MI355X: r_J = 8.8e-5 and r_U = 6.5e-5 on both engines
(bound 1e-3).
"""
import os
import re

import numpy as np
import pytest

import observe_reference as R
import pair_reference as P
import spectrum_reference as S
from optimalcontrolmps_amd import ed
from test_observe_gpu import C1, C1_U, CHAINS, _c1_engine, _mps

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10
PATHS = ["chain", "list"]
KEYS = ("ovl", "occ", "hop")


def _path(monkeypatch, path):
    if path == "list":
        monkeypatch.setenv("OCG_OBS_PAIR_CHAIN", "0")
    else:
        monkeypatch.delenv("OCG_OBS_PAIR_CHAIN", raising=False)


def _at(out, i):
    return {k: out[k][i] for k in KEYS}


def _scale(x, y):
    return P.norm_of(x.dims, x.data, x.L, x.p, x.Q) * P.norm_of(y.dims, y.data, y.L, y.p, y.Q)


def _check(out, xs, ys, what=""):
    """device numbers against the block reference of the host states; returns the references and scales"""
    n, L, p = len(xs), xs[0].L, xs[0].p
    assert out["ovl"].shape == (n,) and out["occ"].shape == (n, L, p) and out["hop"].shape == (n, L - 1, 2)
    assert all(out[k].dtype == np.complex128 for k in KEYS)
    refs = [P.pairs_ref(x.dims, x.data, y.dims, y.data, L, p, x.Q) for x, y in zip(xs, ys)]
    scales = [_scale(x, y) for x, y in zip(xs, ys)]
    worst = max(P.deviation(_at(out, i), refs[i], p, scales[i]) for i in range(n))
    print(f"  {what}: largest deviation {worst:.3e} of the scale (tol {TOL:g})")
    assert worst <= TOL
    return refs, scales


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
    """(xi_t, psi_t), (psi_t, psi_t), (xiH_t, psi_t) against the reference, the ties to the existing calls,
    the swap of bra and ket and the particle-number sum rule"""
    eng, sts = c1_runs(engine)
    _path(monkeypatch, path)
    L, p, Q, N = C1["L"], C1["p"], C1["Q"], C1["Nt"]
    nn = np.arange(p)
    outs = {}
    for wx in (1, 0, 2):
        outs[wx] = eng.observe_pairs(wx, C1_TS, 0, C1_TS)
        _, sc = _check(outs[wx], sts[wx], sts[0], f"{engine} {path} ({wx}, 0)")
        # sum_k sum_n n occ = Q ovl
        ntot = (outs[wx]["occ"] * nn).sum((-1, -2))
        assert (np.abs(ntot - Q * outs[wx]["ovl"]) <= TOL * np.array(sc)).all()
    # <xi_t|D|psi_t> is div_t
    every = eng.observe_pairs(1, None, 0, None)
    D = (every["occ"] * (nn * (nn - 1) / 2)).sum((-1, -2))
    assert np.abs(D - eng.div_t()).max() <= TOL
    # |<xi_{N-1}|psi_t>|^2 is the fidelity of psi_t
    last = eng.observe_pairs(1, [N - 1] * N, 0, None, outputs=("ovl",))
    assert set(last) == {"ovl"}
    assert np.abs(np.abs(last["ovl"]) ** 2 - eng.fidelities()).max() <= TOL
    # x = y: the one-state observables
    same, one = outs[0], eng.observe(0, C1_TS, list(range(1, L + 1)))
    mom = eng.moments(0, C1_TS)
    assert np.abs(same["ovl"] - one["norm2"]).max() <= TOL and np.abs(same["occ"] - one["occ"]).max() <= TOL
    nb = np.arange(L - 1)
    assert np.abs(same["hop"][:, :, 0] - one["ada"][:, nb, nb + 1]).max() <= TOL * (p - 1)
    assert np.abs(same["hop"][:, :, 1] - same["hop"][:, :, 0].conj()).max() <= TOL * (p - 1)
    assert np.abs(same["hop"].sum((-1, -2)) - mom[:, 1]).max() <= TOL * (p - 1)
    # bra and ket swapped
    swp = eng.observe_pairs(0, C1_TS, 1, C1_TS)
    fwd = outs[1]
    assert np.abs(swp["ovl"] - fwd["ovl"].conj()).max() <= TOL
    assert np.abs(swp["occ"] - fwd["occ"].conj()).max() <= TOL
    assert np.abs(swp["hop"][:, :, 0] - fwd["hop"][:, :, 1].conj()).max() <= TOL * (p - 1)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("L,p,Q,J,Ui,Uf", CHAINS + [(2, 3, 2, 1.0, 2.0, 10.0)])
@pytest.mark.parametrize("path", PATHS)
def test_general_chains(states, engine, L, p, Q, J, Ui, Uf, path, monkeypatch):
    """L = 3 and p - 1 < Q (empty sectors, a+ at the level cut, missing partners) and L = 2 (a single bond, no
    interior site), the trajectory states in each engine's own block layout"""
    from optimalcontrolmps_amd.native import MPS, Engine
    _path(monkeypatch, path)
    eng = Engine(L, p, Q, J, 0.01, 1e-8, engine=engine)
    if L == 2:
        gs = [MPS(L, p, Q, *ed.mps_from_full(ed.ground_state_full(L, p, Q, J, U)[0], L, p, Q)) for U in (Uf, Ui)]
        eng.set_states(*gs)
    else:
        eng.set_states(_mps(states, L, p, Q, J, Uf), _mps(states, L, p, Q, J, Ui))
    eng.propagate(np.random.default_rng(7).uniform(2, 10, 9), 3)
    tx, ty = [0, 4, 8, 8], [0, 4, 8, 2]
    for wx, wy in ((1, 0), (0, 1), (0, 0)):
        _check(eng.observe_pairs(wx, tx, wy, ty), [eng.state(wx, t) for t in tx], [eng.state(wy, t) for t in ty],
               f"{engine} {path} ({wx}, {wy})")


# ------------------------------------------------------------ caller-supplied states
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("lo,hi", [(1, 3), (15, 17), (63, 66)])
def test_random_complex_states(engine, lo, hi, monkeypatch):
    """complex, non-canonical, unnormalised states, bra and ket drawn independently (rectangular environments);
    15..17 crosses the chain / list dispatch and the MFMA tile edge"""
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 3, 4, 3
    rng = np.random.default_rng(5)

    def draw(a, b):
        return MPS(L, p, Q, *S.random_mps(rng, L, p, Q, a, b))
    xs, ys = [draw(lo, hi) for _ in range(3)], [draw(lo, hi) for _ in range(3)]
    eng = Engine(L, p, Q, 1.0, 0.01, 1e-8, 128, engine=engine)
    if (lo, hi) == (15, 17):
        assert max(int(m.dims.max()) for m in xs + ys) > 16
        # pairs that stay on the chain kernel beside them, and a narrow bra with a 17-wide ket on the lists
        xs += [draw(16, 16), draw(15, 16), draw(15, 16)]
        ys += [draw(15, 16), draw(16, 16), draw(17, 17)]
        eng.reset_stats()
        eng.observe_pairs_states(xs[3:5], ys[3:5])
        assert eng.stats(9)["launches"] == 1
        eng.reset_stats()
        eng.observe_pairs_states(xs[5:], ys[5:])
        assert eng.stats(9)["launches"] == 5 * L - 2
    xs.append(MPS(L, p, Q, *S.pad_sector(xs[0].dims, xs[0].data, L, p, Q, 1, 1)))  # a zero-padded sector in x only
    ys.append(ys[0])
    refs, sc = _check(eng.observe_pairs_states(xs, ys), xs, ys, f"{engine} {lo}..{hi}")
    assert P.deviation(refs[-1], refs[0], p, sc[0]) <= 1e-13
    assert min(abs(r["ovl"].imag) for r in refs) > 0
    if hi <= 16:
        monkeypatch.setenv("OCG_OBS_PAIR_CHAIN", "0")
        _check(eng.observe_pairs_states(xs, ys), xs, ys, f"{engine} {lo}..{hi} list")


def test_chi256_state():
    from optimalcontrolmps_amd.native import MPS, Engine
    L, p, Q = 20, 7, 20
    z = np.load(os.path.join(HERE, "golden", "c4_warm256.npz"), allow_pickle=False)
    x = MPS(L, p, Q, z["dims"], z["data"])
    assert max(x.bond_dims()) == 256
    eng = Engine(L, p, Q, 1.0, 0.005, 1e-8, 256, engine="hbm")
    y = eng.step(x, 4.0, 4.2)
    eng.reset_stats()
    ps = eng.path_stats()
    out = eng.observe_pairs_states([x], [y])
    assert eng.path_stats() == ps
    s9 = eng.stats(9)
    assert s9["launches"] == 5 * L - 2 and s9["alg_flops"] > 0 and s9["alg_bytes"] > 0 and s9["ms"] > 0
    _, sc = _check(out, [x], [y], "chi 256")
    nn = np.arange(p)
    assert abs(out["ovl"][0] - eng.overlap(x, y, False)) <= TOL * sc[0]
    assert abs((out["occ"][0] * (nn * (nn - 1) / 2)).sum() - eng.overlap(x, y, True)) <= TOL * sc[0]


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_chain_kernel_against_list_path(c1_runs, engine, monkeypatch):
    eng, sts = c1_runs(engine)
    L, p = C1["L"], C1["p"]
    for wx in (1, 0, 2):
        eng.reset_stats()
        a = eng.observe_pairs(wx, C1_TS, 0, C1_TS)
        assert eng.stats(9)["launches"] == 1  # the whole chunk in one launch
        monkeypatch.setenv("OCG_OBS_PAIR_CHAIN", "0")
        eng.reset_stats()
        b = eng.observe_pairs(wx, C1_TS, 0, C1_TS)
        assert eng.stats(9)["launches"] == 5 * L - 2
        eng.reset_stats()
        c = eng.observe_pairs(wx, C1_TS, 0, C1_TS, outputs=("ovl",))
        assert eng.stats(9)["launches"] == 2 * L + 1 and np.array_equal(c["ovl"], b["ovl"])
        monkeypatch.delenv("OCG_OBS_PAIR_CHAIN")
        dev = max(P.deviation(_at(a, i), _at(b, i), p, _scale(sts[wx][i], sts[0][i])) for i in range(len(C1_TS)))
        print(f"  ({wx}, 0): chain against lists {dev:.3e} of the scale")
        assert dev <= TOL


# ------------------------------------------------------------ exact cases
@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_exact_product_states(engine, path, monkeypatch):
    from optimalcontrolmps_amd.native import MPS, Engine
    _path(monkeypatch, path)
    L, p = 5, 3
    eng = Engine(L, p, L, 1.0, 0.01, 1e-8, engine=engine)
    f = MPS(L, p, L, *R.fock(L, p, L, [1] * L))
    half = f.copy()
    half.data[0] *= 0.5
    out = eng.observe_pairs_states([f, half], [f, f])
    assert out["ovl"][0] == 1 and not out["hop"][0].any()
    assert (out["occ"][0][:, 1] == 1).all() and not out["occ"][0][:, [0, 2]].any()
    for k in KEYS:
        assert np.array_equal(out[k][1], 0.5 * out[k][0])
    # one hop apart at bond b: |.. n_b + 1, n_{b+1} - 1 ..> = a+_b a_{b+1} |1 .. 1> / sqrt((n_b + 1) n_{b+1})
    for b in range(1, L):
        occ = [1] * L
        occ[b - 1], occ[b] = 2, 0
        g = MPS(L, p, L, *R.fock(L, p, L, occ))
        out = eng.observe_pairs_states([g, f], [f, g])
        want = np.sqrt(2.0)
        for e, c in ((0, 0), (1, 1)):  # a+_b a_{b+1} towards g, a_b a+_{b+1} back
            assert out["ovl"][e] == 0 and not out["occ"][e].any()
            hop = out["hop"][e].copy()
            assert abs(hop[b - 1, c] - want) <= np.spacing(want) and hop[b - 1, c].imag == 0
            hop[b - 1, c] = 0
            assert not hop.any()


# ------------------------------------------------------------ independence of the request
def _need(eng, t):
    """the chunk workspace one pair's request takes, from the message of the OCG_ENOMEM it gets under a budget
    of one byte"""
    from optimalcontrolmps_amd.native import OcgError
    with pytest.raises(OcgError, match="ENOMEM") as ei:
        eng.observe_pairs(1, [t], 0, [t])
    return int(re.search(r"\((\d+) B\)", str(ei.value)).group(1))


def _equal(a, b, idx=None):
    return all(np.array_equal(a[k], b[k] if idx is None else b[k][idx]) for k in KEYS)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
@pytest.mark.parametrize("path", PATHS)
def test_results_do_not_depend_on_the_request(c1_runs, engine, path, monkeypatch):
    eng, _ = c1_runs(engine)
    _path(monkeypatch, path)
    every = eng.observe_pairs(1, None, 0, None)
    assert every["ovl"].shape == (C1["Nt"],)
    assert _equal(eng.observe_pairs(1, [7], 0, [7]), every, [7])
    pick = [20, 7, 7, 0, 13]
    assert _equal(eng.observe_pairs(1, pick, 0, pick), every, pick)
    assert _equal(eng.observe_pairs(1, None, 0, list(range(C1["Nt"]))), every)
    sub = eng.observe_pairs(1, pick, 0, pick, outputs=("occ",))
    assert set(sub) == {"occ"} and np.array_equal(sub["occ"], every["occ"][pick])
    # every pair in a chunk of its own
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    need = max(_need(eng, t) for t in (0, 10, 20))
    monkeypatch.setenv("OCG_OBS_BUDGET", str(need))
    split = eng.observe_pairs(1, None, 0, None)
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert _equal(split, every)
    # host copies of the same states, staged
    if engine == "lds":  # (the compact format is the LDS engine's own block layout: the same operands)
        ts = [3, 20]
        staged = eng.observe_pairs_states([eng.state(1, t) for t in ts], [eng.state(0, t) for t in ts])
        assert _equal(staged, every, ts)


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_pairs_leave_the_device_state(states, engine):
    eng = _c1_engine(states, engine)
    H0, divT0, F0 = eng.hessian(C1_U)
    ps = eng.path_stats()
    eng.observe_pairs(1, None, 0, None)
    eng.observe_pairs(2, [3, 3, 20], 0, [1, 2, 3])
    eng.observe_pairs(0, [5], 2, [5])
    assert eng.path_stats() == ps
    H, divT, F = eng.hessian(C1_U)
    assert np.array_equal(H, H0) and np.array_equal(divT, divT0) and F == F0


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_errors(states, engine, monkeypatch):
    from optimalcontrolmps_amd import native as nat
    eng = _c1_engine(states, engine)

    def fails(code, *a):
        with pytest.raises(nat.OcgError, match=code):
            eng.observe_pairs(*a)
    fails("ESTATE", 1, [0], 0, [0])                  # before any propagate
    eng.propagate(C1_U, 3)
    assert eng.observe_pairs(1, [0], 0, [0])["ovl"].shape == (1,)
    fails("ESTATE", 2, [0], 0, [0])                  # no xi_dH yet
    fails("ESTATE", 0, [0], 2, [0])
    for bad in ((0, [C1["Nt"]], 0, [0]), (0, [0], 0, [-1]), (3, [0], 0, [0]), (0, [0], -1, [0])):
        fails("EINVAL", *bad)
        assert abs(eng.observe_pairs(0, [20], 0, [20])["ovl"][0] - 1) < 1e-6
    # npairs == 0 writes nothing
    buf = np.full(8, 7.0)
    ptr = buf.ctypes.data_as(nat.dp)
    assert nat.lib().ocg_observe_pairs(eng.h, 1, None, 0, None, 0, ptr, ptr, ptr) == 0 and (buf == 7).all()
    assert eng.observe_pairs(1, [], 0, [])["occ"].shape == (0, C1["L"], C1["p"])
    assert eng.observe_pairs_states([], [])["hop"].shape == (0, C1["L"] - 1, 2)
    # a budget too small for one pair
    monkeypatch.setenv("OCG_OBS_BUDGET", "1")
    fails("ENOMEM", 1, [3], 0, [3])
    monkeypatch.delenv("OCG_OBS_BUDGET")
    assert eng.observe_pairs(1, [3], 0, [3])["ovl"].shape == (1,)


# ------------------------------------------------------------ sensitivities against finite differences
SENS = dict(L=5, p=5, Q=5, J=1.0, dt=0.01, cut=1e-8, maxm=80, Nt=21)
SENS_U = np.linspace(2.5, 6, 21) + 0.7 * np.sin(np.linspace(0, 5, 21))


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_sensitivities_against_finite_differences(engine):
    """sum_t w_t dJ[t] and sum_t w_t dU[t] (trapezoid weights w) against central differences of the cost
    0.5 (1 - |F|^2) over J +- 1e-5 and u +- 1e-5: relative deviation at most 1e-3, the tolerance of the GRAPE
    gradient against finite differences in test_facade_gpu.py.  The CPU oracle alone gives 8.8e-5 and 6.5e-5;
    a wrong sign, a conjugated F or a lost factor 2 gives at least 0.5."""
    from optimalcontrolmps_amd.native import MPS, Engine, control_sensitivities
    c = SENS
    L, p, Q = c["L"], c["p"], c["Q"]
    ini = MPS(L, p, Q, *ed.mps_from_full(ed.ground_state_full(L, p, Q, c["J"], 2.5)[0], L, p, Q))
    tgt = MPS(L, p, Q, *ed.mps_from_full(ed.ground_state_full(L, p, Q, c["J"], 4.0)[0], L, p, Q))

    def cost(J, u):
        e = Engine(L, p, Q, J, c["dt"], c["cut"], c["maxm"], engine=engine)
        e.set_states(tgt, ini)
        e.propagate(u, 1)
        return 0.5 * (1 - abs(e.overlap_factor()) ** 2)
    d = 1e-5
    fd_J = (cost(c["J"] + d, SENS_U) - cost(c["J"] - d, SENS_U)) / (2 * d)
    fd_U = (cost(c["J"], SENS_U + d) - cost(c["J"], SENS_U - d)) / (2 * d)
    eng = Engine(L, p, Q, c["J"], c["dt"], c["cut"], c["maxm"], engine=engine)
    eng.set_states(tgt, ini)
    divT, F = eng.gradient(SENS_U)
    s = control_sensitivities(eng.observe_pairs(1, None, 0, None), F, c["dt"])
    assert s["dU"].shape == s["dJ"].shape == s["overlap"].shape == (c["Nt"],) and s["dEps"].shape == (c["Nt"], L)
    w = np.ones(c["Nt"])
    w[0] = w[-1] = 0.5
    r_J = abs((w * s["dJ"]).sum() - fd_J) / abs(fd_J)
    r_U = abs((w * s["dU"]).sum() - fd_U) / abs(fd_U)
    print(f"  {engine}: FD_J = {fd_J:.6e}, FD_U = {fd_U:.6e}, r_J = {r_J:.3e}, r_U = {r_U:.3e}")
    print(f"  truncation diagnostic: max |<xi_t|psi_t> F - |F|^2| = {np.abs(s['overlap'] * F - abs(F) ** 2).max():.3e}")
    assert r_J <= 1e-3 and r_U <= 1e-3
    grad = c["dt"] * (1j * divT * F).real
    assert np.abs(s["dU"] - grad).max() <= TOL * c["dt"] * abs(F) * np.abs(divT).max()
    # sum_k dEps[t][k] = Q tstep Re(i <xi_t|psi_t> F)
    assert np.abs(s["dEps"].sum(1) - Q * c["dt"] * (1j * s["overlap"] * F).real).max() <= TOL * c["dt"] * abs(F)
