"""The static site potential sum_k eps_k n_k (ocg_set_potential) on both engines,
against the dense references of dense_potential.py (pinned on the CPU by test_dense_potential_reference.py).

Engines: J = 1, dt = 0.01, cutoff 1e-14, Maxm 512 (nothing binds).  LDS engine: the one-wave chain (E passes
around the padded step) and the general chain (OCG_NO_FAST: per-site phases inside apply_gate); HBM engine:
the stored, pipelined and checkpointed getHessian, the stored and the meet-in-the-middle gradient.

Bounds.  Every quantity against dense: max(1e-12, 10 x the oracle-composed reference's own deviation from
dense on that case and quantity, tests/golden/dense_potential.json), in the units of
test_dense_trajectory_gpu.py (F absolute, divT relative to max|divT|, fidelities absolute, H relative to
S = max|A| + max|B|, states by dense_reference.deviation and the relative norm of xiH, the gradient to the sum
of the divT and F bounds) and, for the sensitivities s[t, k] = dt Re(i <xi_t|n_k|psi_t> F), relative to
dt max|<xi_t|n_k|psi_t>|.  Equalities between two device paths of one arithmetic are bit for bit.  Every
assertion prints its figure ("FIG ..." lines).

The round trip.  BH_tDMRG::step backward sweeps the bonds in the forward order, so a forward step followed by
the backward step with the same controls returns the input only to the order of the splitting (the dense
reference itself comes back 9e-5 away on (5,5,5), 2.2e-4 on (4,4,7), with or without a potential).  The round
trip is therefore held against the dense round trip within the state bound, and its distance from the input
is printed.

Worst figures observed on an MI355X next to their bounds: see DESIGN.md section 15."""
import json
import os

import numpy as np
import pytest

import dense_potential as P
import dense_reference as D
import dense_trajectory as T
from optimalcontrolmps_amd import ed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "dense_potential.json")) as _f:
    GOLDEN = json.load(_f)["cases"]

LDS_KINDS = ("onewave", "general")
HBM_ENV = ("OCG_HBM_PIPE", "OCG_HBM_CKPT", "OCG_HBM_CKPT_MID", "OCG_HBM_MID", "OCG_HBM_FASTGAUGE")
UNIFORM = 1.7


def _engine(monkeypatch, name, kind, eps="case", **env):
    """a context of the case's shape with its target and init set and the case's potential (eps: "case",
    None, or an array) in force; env: OCG_NO_PLANS and the HBM path switches (all others unset)"""
    from optimalcontrolmps_amd.native import MPS, Engine
    if kind == "general":
        monkeypatch.setenv("OCG_NO_FAST", "1")
    else:
        monkeypatch.delenv("OCG_NO_FAST", raising=False)
    monkeypatch.delenv("OCG_NO_FAST_OVL", raising=False)
    for var in HBM_ENV + ("OCG_NO_PLANS",):
        if var in env:
            monkeypatch.setenv(var, str(env[var]))
        else:
            monkeypatch.delenv(var, raising=False)
    traj = P.traj_of(name)
    shape = T.traj_shape(traj)
    e = Engine(*shape, D.J, D.DT, D.CUTOFF, D.MAXM, engine="hbm" if kind == "hbm" else "lds")
    fast = 1 if kind == "onewave" else 0
    assert e.info.fast_chain == fast
    if eps is not None:
        e.set_potential(P.potential(name) if isinstance(eps, str) else eps)
        assert e.info.fast_chain == fast        # the one-wave chain keeps running with a potential
    (di, xi, _), (dt, xt, _) = T.traj_states(traj)
    e.set_states(MPS(*shape, dt, xt), MPS(*shape, di, xi))
    return e


def _fig(case, what, value):
    print(f"FIG {case} {what} {value:.3e}")
    return value


def _bound(name, key):
    return max(1e-12, 10.0 * GOLDEN[name][key])


def _check_scalars(name, tag, ref, F, divT, fid=None):
    dmax = np.abs(ref["divT"]).max()
    assert _fig(name, f"{tag}_F", abs(F - ref["F"])) <= _bound(name, "F")
    assert _fig(name, f"{tag}_divT", np.abs(divT - ref["divT"]).max() / dmax) <= _bound(name, "divT")
    g = D.DT * (1j * np.asarray(divT) * F).real
    assert _fig(name, f"{tag}_grad", np.abs(g - ref["grad"]).max() / (D.DT * dmax)) \
        <= _bound(name, "divT") + _bound(name, "F")
    if fid is not None:
        assert _fig(name, f"{tag}_fid", np.abs(fid - ref["fid"]).max()) <= _bound(name, "fid")


def _check_H(name, tag, ref, H):
    N = len(ref["divT"])
    assert H.shape == (N, N) and not H[0].any() and not H[N - 1].any() and np.array_equal(H, H.T)
    assert _fig(name, f"{tag}_H", np.abs(H - ref["H"]).max() / T.hessian_scale(ref)) <= _bound(name, "H")


def _check_states(name, tag, e, ref):
    """state(0 / 1 / 2, t) against psi_t, xi_t and dH xi_t (its norm and its direction), t = 0, N/2, N-1"""
    N, shape = len(ref["divT"]), T.traj_shape(P.traj_of(name))
    worst = 0.0
    for t in (0, N // 2, N - 1):
        for which, r in ((0, ref["psi"][t]), (1, ref["xi"][t])):
            worst = max(worst, *D.deviation(r, D.dense_of(e.state(which, t))))
        w = D.dense_of(e.state(2, t))
        n = np.linalg.norm(w)
        xh = D.dense_apply_dH(ref["xi"][t], shape)
        worst = max(worst, abs(n - ref["xiH_norm"][t]) / ref["xiH_norm"][t],
                    *D.deviation(xh / ref["xiH_norm"][t], w / n))
    assert _fig(name, f"{tag}_state", worst) <= _bound(name, "state")


def _check_final_ranks(name, e, ref):
    N = len(ref["divT"])
    ranks = D.schmidt_ranks(ref["psi"][-1], T.traj_shape(P.traj_of(name)))[0]
    assert np.array_equal(e.state(0, N - 1).dims, ranks.reshape(-1))


def _unfused(e, u):
    N = len(u)
    e.propagate(u, 3)
    divT, F, fid = e.div_t(), e.overlap_factor(), e.fidelities()
    e.xi_dH()
    return e.hessian_rows(u, list(range(1, N - 1)), F, divT), divT, F, fid


def _same_state(a, b):
    return np.array_equal(a.dims, b.dims) and np.array_equal(a.data, b.data)


def _controls(name, k=0):
    return T.traj_controls(P.traj_of(name), None, k)


LDS = [(n, k) for n in P.POT_LDS + ["T_L5p5Q5_steep"] for k in LDS_KINDS]
LDS_IDS = ["%s-%s" % nk for nk in LDS]


# ------------------------------------------------------------------------------------------ LDS engine
@pytest.mark.parametrize("name,kind", LDS, ids=LDS_IDS)
def test_lds_drivers(monkeypatch, name, kind):
    """the unfused driver sequence, ocg_hessian and ocg_gradient against dense (odd chain, even chain,
    p = 6, and the steep case); fused == unfused bit for bit"""
    u, ref = _controls(name), P.pot_reference(name)
    e = _engine(monkeypatch, name, kind)
    H, divT, F, fid = _unfused(e, u)
    _check_scalars(name, f"{kind}_unfused", ref, F, divT, fid)
    _check_H(name, f"{kind}_unfused", ref, H)
    _check_final_ranks(name, e, ref)
    _check_states(name, f"{kind}_unfused", e, ref)
    N = len(u)
    kept = [e.state(w, t) for w in (0, 1, 2) for t in (0, N // 2, N - 1)]
    H2, divT2, F2 = e.hessian(u)
    assert np.array_equal(H2, H) and np.array_equal(divT2, divT) and F2 == F
    assert np.array_equal(e.fidelities(), fid)
    assert all(_same_state(a, b) for a, b in zip(kept, [e.state(w, t) for w in (0, 1, 2) for t in (0, N // 2, N - 1)]))
    _check_scalars(name, f"{kind}_fused", ref, F2, divT2, e.fidelities())
    _check_H(name, f"{kind}_fused", ref, H2)
    d3, F3 = e.gradient(u)
    _check_scalars(name, f"{kind}_gradient", ref, F3, d3)
    e.close()


@pytest.mark.parametrize("name,kind", [(n, k) for n in P.POT_LDS for k in LDS_KINDS],
                         ids=["%s-%s" % (n, k) for n in P.POT_LDS for k in LDS_KINDS])
def test_lds_multi(monkeypatch, name, kind):
    """ocg_hessian_multi with K = 3 distinct control vectors, every member against its own dense reference"""
    K = 3
    us = np.array([_controls(name, k) for k in range(K)])
    e = _engine(monkeypatch, name, kind)
    H, divT, F = e.hessian_multi(us)
    for k in range(K):
        ref = P.pot_reference(name, None, k)
        _check_scalars(name, f"{kind}_multi_{k}", ref, F[k], divT[k])
        _check_H(name, f"{kind}_multi_{k}", ref, H[k])
    # the context keeps control 0's trajectories
    ref = P.pot_reference(name, None, 0)
    assert _fig(name, f"{kind}_multi_fid", np.abs(e.fidelities() - ref["fid"]).max()) <= _bound(name, "fid")
    _check_states(name, f"{kind}_multi", e, ref)
    _check_final_ranks(name, e, ref)
    e.close()


@pytest.mark.parametrize("name", P.POT_LDS)
def test_lds_plans_do_not_matter(monkeypatch, name):
    """the general chain with its decomposition plans and with OCG_NO_PLANS=1: bit for bit (the plans cache
    index arithmetic only; the potential's phases are read per site either way)"""
    u = _controls(name)
    got = []
    for plans_off in ("0", "1"):
        e = _engine(monkeypatch, name, "general", OCG_NO_PLANS=plans_off)
        H, divT, F = e.hessian(u)
        got.append((H, divT, F, e.state(0, len(u) - 1), e.state(1, 0)))
        e.close()
    a, b = got
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert _same_state(a[3], b[3]) and _same_state(a[4], b[4])
    _check_H(name, "general_noplans", P.pot_reference(name), b[0])


# ------------------------------------------------------------------------------------------ HBM engine
@pytest.mark.parametrize("name", P.POT_HBM + ["T_L9p3Q9_steep"])
def test_hbm_stored_and_pipelined(monkeypatch, name):
    """the stored two-phase getHessian (OCG_HBM_PIPE=0) and the pipelined one (OCG_HBM_PIPE=1) against dense
    and against each other bit for bit (even chain, odd chain, the small chain, and the steep case)"""
    u, ref = _controls(name), P.pot_reference(name)
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_PIPE=0)
    H, divT, F = e.hessian(u)
    assert e.path_stats()["pipe_runs"] == 0
    _check_scalars(name, "hbm_stored", ref, F, divT, e.fidelities())
    _check_H(name, "hbm_stored", ref, H)
    _check_final_ranks(name, e, ref)
    _check_states(name, "hbm_stored", e, ref)
    fid = e.fidelities()
    e.close()
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_PIPE=1)
    H2, divT2, F2 = e.hessian(u)
    assert e.path_stats()["pipe_runs"] == 1 and e.path_stats()["pipe_fallbacks"] == 0
    assert np.array_equal(H2, H) and np.array_equal(divT2, divT) and F2 == F and np.array_equal(e.fidelities(), fid)
    _check_states(name, "hbm_pipe", e, ref)
    e.close()


def test_hbm_checkpointed_and_mid(monkeypatch):
    """the checkpointed getHessian (OCG_HBM_CKPT=3) and the meet-in-the-middle gradient (OCG_HBM_MID=1), bit
    for bit against the stored paths"""
    name = "T_L9p3Q9"
    u, ref = _controls(name), P.pot_reference(name)
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_PIPE=0)
    H, divT, F = e.hessian(u)
    e.close()
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_CKPT=3)
    H2, divT2, F2 = e.hessian(u)
    st = e.path_stats()
    assert st["ckpt_runs"] == 1 and st["ckpt_k"] == 3 and st["pipe_runs"] == 0
    assert np.array_equal(H2, H) and np.array_equal(divT2, divT) and F2 == F
    e.close()
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_MID=0)
    d0, F0 = e.gradient(u)
    e.close()
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_MID=1)
    d1, F1 = e.gradient(u)
    e.close()
    assert np.array_equal(d0, divT) and F0 == F and np.array_equal(d1, d0) and F1 == F0
    _check_scalars(name, "hbm_mid", ref, F1, d1)


def test_hbm_step_batch(monkeypatch):
    """ocg_step_batch with three states (own controls each) == three ocg_step calls, bit for bit"""
    from optimalcontrolmps_amd.native import MPS
    name = "T_L8p4Q8"
    shape = T.traj_shape(name)
    e = _engine(monkeypatch, name, "hbm")
    (di, xi, _), (dt, xt, _) = T.traj_states(name)
    a = MPS(*shape, di, xi)
    states = [a, MPS(*shape, dt, xt), e.step(a, 4.0, 6.0)]
    uf, ut = [3.0, 5.5, 8.0], [7.0, 2.5, 9.0]
    batch = e.step_batch(states, uf, ut, True)
    for i in range(3):
        assert _same_state(batch[i], e.step(states[i], uf[i], ut[i], True))
    e.close()


# ------------------------------------------------------------------------------------------ both engines
BOTH = [("T_L5p5Q5", "onewave"), ("T_L5p5Q5", "general"), ("T_L4p4Q7", "onewave"), ("T_L4p4Q7", "general"),
        ("T_L8p4Q8", "hbm"), ("T_L9p3Q9", "hbm")]
BOTH_IDS = ["%s-%s" % nk for nk in BOTH]


@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_round_trip(monkeypatch, name, kind):
    """ocg_step forward then backward with the same controls against the dense round trip (see the module
    docstring: the input itself comes back only to the order of the splitting)"""
    from optimalcontrolmps_amd.native import MPS
    shape = T.traj_shape(name)
    L, p, _ = shape
    eps = P.potential(name)
    e = _engine(monkeypatch, name, kind)
    (di, xi, psi), _ = T.traj_states(name)
    fw = e.step(MPS(*shape, di, xi), 3.0, 7.0, True)
    bk = e.step(fw, 7.0, 3.0, False)
    d1 = ed.exact_step(psi, L, p, D.J, D.DT, 3.0, 7.0, True, eps=eps)
    d2 = ed.exact_step(d1, L, p, D.J, D.DT, 7.0, 3.0, False, eps=eps)
    _fig(name, f"{kind}_roundtrip_from_input", max(D.deviation(psi, D.dense_of(bk))))
    _fig(name, f"{kind}_roundtrip_dense_from_input", max(D.deviation(psi, d2)))
    assert _fig(name, f"{kind}_forward", max(D.deviation(d1, D.dense_of(fw)))) <= _bound(name, "state")
    assert _fig(name, f"{kind}_roundtrip", max(D.deviation(d2, D.dense_of(bk)))) <= _bound(name, "state")
    e.close()


@pytest.mark.parametrize("name,kind", BOTH, ids=BOTH_IDS)
def test_uniform_potential_is_a_global_phase(monkeypatch, name, kind):
    """eps_k = 1.7 on every site: the untrapped fidelities, gradient and H to 1e-12 (odd and even chains: a
    lonely-site phase wrong by a site-independent factor would pass on one parity only)"""
    u = _controls(name)
    e = _engine(monkeypatch, name, kind, eps=None)
    H0, d0, F0 = e.hessian(u)
    fid0 = e.fidelities()
    e.set_potential(np.full(e.L, UNIFORM))
    H1, d1, F1 = e.hessian(u)
    fid1 = e.fidelities()
    ref = T.traj_reference(name)
    dmax = np.abs(ref["divT"]).max()
    g0, g1 = D.DT * (1j * d0 * F0).real, D.DT * (1j * d1 * F1).real
    assert abs(F1 - F0) > 1e-3      # the phase is there
    assert _fig(name, f"{kind}_uniform_fid", np.abs(fid1 - fid0).max()) <= 1e-12
    assert _fig(name, f"{kind}_uniform_grad", np.abs(g1 - g0).max() / (D.DT * dmax)) <= 1e-12
    assert _fig(name, f"{kind}_uniform_H", np.abs(H1 - H0).max() / T.hessian_scale(ref)) <= 1e-12
    e.close()


# ------------------------------------------------------------------------------------------ set and clear
@pytest.mark.parametrize("kind", ["onewave", "general", "hbm"])
def test_set_and_clear(monkeypatch, kind):
    from optimalcontrolmps_amd import native as nat
    name = "T_L5p5Q5"
    u, eps = _controls(name), P.potential(name)
    never = _engine(monkeypatch, name, kind, eps=None)
    H0, d0, F0 = never.hessian(u)
    fast0 = never.info.fast_chain
    never.close()
    e = _engine(monkeypatch, name, kind, eps=None)
    assert np.array_equal(e.potential, np.zeros(e.L))
    e.set_potential(eps)
    assert np.array_equal(e.potential, eps)
    H1, _, F1 = e.hessian(u)
    assert abs(F1 - F0) > 1e-3 and not np.array_equal(H1, H0)
    # stored trajectories are dropped like ocg_set_tstep does
    e.set_potential(eps)
    with pytest.raises(nat.OcgError, match="ESTATE"):
        e.div_t()
    e.set_potential(None)
    assert np.array_equal(e.potential, np.zeros(e.L)) and e.info.fast_chain == fast0
    H2, d2, F2 = e.hessian(u)
    assert np.array_equal(H2, H0) and np.array_equal(d2, d0) and F2 == F0
    # all zeros is the same as NULL
    e.set_potential(eps)
    e.set_potential(np.zeros(e.L))
    assert np.array_equal(e.potential, np.zeros(e.L))
    H3, d3, F3 = e.hessian(u)
    assert np.array_equal(H3, H0) and np.array_equal(d3, d0) and F3 == F0
    # NaN / inf are rejected and change nothing
    e.set_potential(eps)
    for bad in (np.nan, np.inf):
        b = eps.copy()
        b[2] = bad
        with pytest.raises(nat.OcgError, match="EINVAL"):
            e.set_potential(b)
    assert np.array_equal(e.potential, eps)
    e.close()


# ------------------------------------------------------------------------------------------ ground state
GS_TOL = 2e-7       # tests/test_ground_state.py TOL[2.5]


@pytest.mark.parametrize("engine", ["lds", "hbm"])
def test_trapped_ground_state(engine):
    """ocg_ground_state at L = 5, p = 5, Q = 5, U = 2.5 in the trap, against exact diagonalisation with the
    same potential: the infidelity of tests/test_ground_state.py within its TOL, and <n_k> through
    ocg_observe.  A state of infidelity i has |d<n_k>| <= 2 (p - 1) sqrt(i), which sets the density's
    tolerance; the exact density is asymmetric by more than 100 times that, so a potential that is ignored
    (a symmetric density) fails.

    LDS engine: InitializeState's whole tau schedule from the product state (1 s).  On the HBM engine that
    schedule is 3500 host-driven steps and 80 s (measured), so there ocg_ground_state runs the closing
    tau = 5e-4 stage for 100 steps from the exact trapped ground state: the Trotter fixed point of that stage
    lies 3.6e-8 from it (exact state-vector iteration), inside TOL, while weights of another potential move
    the state by tau * steps * (spread of eps) = 0.05 * 4, five orders above TOL."""
    from optimalcontrolmps_amd.native import MPS, Engine
    from optimalcontrolmps_amd.states import ground_state
    L, p, N, J, U = 5, 5, 5, 1.0, 2.5
    eps = P.potential("T_L5p5Q5")
    gs, _ = ed.ground_state_full(L, p, N, J, U, eps)
    g = np.indices((p,) * L).reshape(L, -1)
    n_ex = (g * np.abs(gs) ** 2).sum(axis=1)
    n_tol = 2 * (p - 1) * np.sqrt(GS_TOL)
    assert np.abs(n_ex - n_ex[::-1]).max() > 100 * n_tol
    eng = Engine(L, p, N, J, 0.01, 1e-9, 80, engine=engine)
    eng.set_potential(eps)
    if engine == "lds":
        psi = ground_state(eng, U)
    else:
        start = MPS(L, p, N, *ed.mps_from_full(gs, L, p, N))
        psi, steps = eng.ground_state(start, U, (0.0005,), block=25, tol=1e-13, max_steps=100)
        assert steps == 100
    v = ed.full_from_mps(psi.dims, psi.data, L, p, N)
    infid = 1.0 - abs(np.vdot(gs, v)) ** 2 / (np.vdot(v, v).real * np.vdot(gs, gs).real)
    assert _fig(engine, "trapped_gs_infidelity", infid) < GS_TOL
    o = eng.observe_states([psi], outputs=("norm2", "occ"))
    n_dev = (o["occ"][0] * np.arange(p)).sum(axis=1) / o["norm2"][0]
    assert _fig(engine, "trapped_gs_density", np.abs(n_dev - n_ex).max()) <= n_tol
    if engine == "lds":
        # states.ground_state(eps=...) passes a potential through and puts the engine's own back
        eng.set_potential(None)
        psi2 = ground_state(eng, U, eps=eps)
        assert _same_state(psi2, psi) and np.array_equal(eng.potential, np.zeros(L))
    else:
        # the same 100 steps without the potential leave the trapped ground state by far more than TOL
        eng.set_potential(None)
        off, _ = eng.ground_state(start, U, (0.0005,), block=25, tol=1e-13, max_steps=100)
        w = ed.full_from_mps(off.dims, off.data, L, p, N)
        away = 1.0 - abs(np.vdot(gs, w)) ** 2 / (np.vdot(w, w).real * np.vdot(gs, gs).real)
        assert _fig(engine, "untrapped_steps_infidelity", away) > 100 * GS_TOL
    eng.close()


# ------------------------------------------------------------------------------------------ sensitivities
@pytest.mark.parametrize("name,kind", [("T_L5p5Q5", "onewave"), ("T_L9p3Q9", "hbm")])
def test_sensitivities(monkeypatch, name, kind):
    """native.control_sensitivities from ocg_observe_pairs(xi_t, psi_t) of the trapped trajectories: dEps
    against the dense s[t, k]"""
    from optimalcontrolmps_amd import native as nat
    u, ref = _controls(name), P.pot_reference(name)
    e = _engine(monkeypatch, name, kind)
    e.propagate(u, 3)
    F = e.overlap_factor()
    s = nat.control_sensitivities(e.observe_pairs(1, None, 0, None), F, D.DT)
    assert s["dEps"].shape == ref["sens"].shape
    assert _fig(name, f"{kind}_sens", np.abs(s["dEps"] - ref["sens"]).max() / P.sens_scale(ref)) \
        <= _bound(name, "sens")
    assert _fig(name, f"{kind}_sens_dU", np.abs(s["dU"] - ref["grad"]).max() / (D.DT * np.abs(ref["divT"]).max())) \
        <= _bound(name, "divT") + _bound(name, "F")
    e.close()
