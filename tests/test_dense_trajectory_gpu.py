"""The gradient and Hessian drivers of both engines (ocg_set_states, ocg_propagate, ocg_div_t,
ocg_overlap_factor, ocg_fidelities, ocg_xi_dH, ocg_hessian_rows, ocg_hessian, ocg_hessian_multi,
ocg_gradient, ocg_gradient_multi) against dense state vectors, on complex right-canonical inputs with flat
Schmidt spectra and every sector populated (dense_trajectory.TRAJ_CASES; the inputs and the reference are
pinned on the CPU by test_dense_trajectory_reference.py).  The reference, dense_trajectory.dense_trajectory,
is written from the state vector alone: it shares no convention of conjugation, normiH or index pairing with
the kernels or with the CPU oracle.

Engines: J = 1, dt = 0.01, cutoff 1e-14, Maxm 512 (nothing binds).  LDS engine: the one-wave chain and the
general chain (OCG_NO_FAST); HBM engine: the stored two-phase, the pipelined and the checkpointed getHessian,
the reuse of stored trajectories, the stored and the meet-in-the-middle gradient, the batched gradient_multi.

Bounds.  Every asserted quantity: max(1e-12, 10 x the CPU oracle's own deviation from dense on that case and
quantity, tests/golden/dense_trajectories.json), in the anchor's units: F absolute, divT relative to
max|divT|, fidelities absolute, H relative to S = max|A| + max|B| (the two terms cancel tenfold), stored
states by dense_reference.deviation and the relative norm of xiH.  The gradient dt Re(i divT F) is a
product of two bounded factors (|F| <= 1): its deviation relative to dt max|divT| is held to the sum of the
divT and F bounds.  The factor 10 allows another eigensolver to place rounding-level eigenvalues
differently.  Bond dimensions: the dense psi_{N-1}'s Schmidt ranks above 1e-12.  Equalities between two
device paths of one arithmetic are bit for bit.  Every assertion prints its figure ("FIG ..." lines).

Worst figures observed on an MI355X next to their bounds: see DESIGN.md section 14a."""
import json
import os

import numpy as np
import pytest

import dense_reference as D
import dense_trajectory as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "dense_trajectories.json")) as _f:
    GOLDEN = json.load(_f)

LDS_KINDS = ("onewave", "general")
HBM_ENV = ("OCG_HBM_PIPE", "OCG_HBM_CKPT", "OCG_HBM_CKPT_MID", "OCG_HBM_MID", "OCG_HBM_FASTGAUGE")


def _engine(monkeypatch, name, kind, **env):
    """a context of the case's shape with its target and init set; env: the HBM path switches (all others
    of HBM_ENV unset)"""
    from optimalcontrolmps_amd.native import MPS, Engine
    if kind == "general":
        monkeypatch.setenv("OCG_NO_FAST", "1")
    else:
        monkeypatch.delenv("OCG_NO_FAST", raising=False)
    monkeypatch.delenv("OCG_NO_FAST_OVL", raising=False)
    for var in HBM_ENV:
        if var in env:
            monkeypatch.setenv(var, str(env[var]))
        else:
            monkeypatch.delenv(var, raising=False)
    shape = T.traj_shape(name)
    e = Engine(*shape, D.J, D.DT, D.CUTOFF, D.MAXM, engine="hbm" if kind == "hbm" else "lds")
    assert e.info.fast_chain == (1 if kind == "onewave" else 0)
    (di, xi, _), (dt, xt, _) = T.traj_states(name)
    e.set_states(MPS(*shape, dt, xt), MPS(*shape, di, xi))
    return e


def _fig(case, what, value):
    print(f"FIG {case} {what} {value:.3e}")
    return value


def _bound(name, key):
    return max(1e-12, 10.0 * GOLDEN[name][key])


def _check_scalars(name, tag, ref, F, divT, fid=None):
    """F, divT, the gradient formed from them and (if given) the fidelities against dense"""
    dmax = np.abs(ref["divT"]).max()
    assert _fig(name, f"{tag}_F", abs(F - ref["F"])) <= _bound(name, "F")
    assert _fig(name, f"{tag}_divT", np.abs(divT - ref["divT"]).max() / dmax) <= _bound(name, "divT")
    g = D.DT * (1j * np.asarray(divT) * F).real
    assert _fig(name, f"{tag}_grad", np.abs(g - ref["grad"]).max() / (D.DT * dmax)) \
        <= _bound(name, "divT") + _bound(name, "F")
    if fid is not None:
        assert _fig(name, f"{tag}_fid", np.abs(fid - ref["fid"]).max()) <= _bound(name, "fid")


def _mask(N, rows):
    """the entries of H that the rows write: (i, j >= i) for j <= N-2 and their mirrors"""
    m = np.zeros((N, N), bool)
    for i in rows:
        m[i, i:N - 1] = m[i:N - 1, i] = True
    return m


def _check_H(name, tag, ref, H, rows=None):
    N = len(ref["divT"])
    m = _mask(N, range(1, N - 1) if rows is None else rows)
    assert H.shape == (N, N) and not H[~m].any()
    assert np.array_equal(H, H.T)
    assert _fig(name, f"{tag}_H", np.abs(H - ref["H"])[m].max() / T.hessian_scale(ref)) <= _bound(name, "H")


def _check_states(name, tag, e, ref, ts=None):
    """state(0 / 1 / 2, t) against psi_t, xi_t and dH xi_t (its norm and its direction); t = 0, the middle
    and N-1 unless given"""
    N, shape = len(ref["divT"]), T.traj_shape(name)
    worst = 0.0
    for t in (0, N // 2, N - 1) if ts is None else ts:
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
    assert np.array_equal(e.state(0, N - 1).dims, D.schmidt_ranks(ref["psi"][-1], T.traj_shape(name))[0].reshape(-1))


def _unfused(e, u, rows=None):
    """the explicit driver sequence: (H, divT, F, fid)"""
    N = len(u)
    e.propagate(u, 3)
    divT, F, fid = e.div_t(), e.overlap_factor(), e.fidelities()
    e.xi_dH()
    return e.hessian_rows(u, list(range(1, N - 1)) if rows is None else rows, F, divT), divT, F, fid


def _same_state(a, b):
    return np.array_equal(a.dims, b.dims) and np.array_equal(a.data, b.data)


LDS = [(n, k) for n in T.TRAJ_LDS for k in LDS_KINDS]
LDS_IDS = ["%s-%s" % nk for nk in LDS]


# ------------------------------------------------------------------------------------------ LDS engine
@pytest.mark.parametrize("name,kind", LDS, ids=LDS_IDS)
def test_lds_unfused(monkeypatch, name, kind):
    """set_states, propagate(u, 3), div_t, overlap_factor, fidelities, xi_dH, hessian_rows (k_trajectory,
    k_hessian_rows) and ocg_gradient against dense; psi then xi in two launches bit for bit the same"""
    u, ref = T.traj_controls(name), T.traj_reference(name)
    N, tag = len(u), f"{kind}_unfused"
    e = _engine(monkeypatch, name, kind)
    H, divT, F, fid = _unfused(e, u)
    _check_scalars(name, tag, ref, F, divT, fid)
    _check_H(name, tag, ref, H)
    _check_final_ranks(name, e, ref)
    _check_states(name, tag, e, ref)
    ts = (0, N // 2, N - 1)
    kept = [e.state(w, t) for w in (0, 1) for t in ts]
    e.propagate(u, 1)
    e.propagate(u, 2)
    assert np.array_equal(e.div_t(), divT) and e.overlap_factor() == F and np.array_equal(e.fidelities(), fid)
    assert all(_same_state(a, b) for a, b in zip(kept, [e.state(w, t) for w in (0, 1) for t in ts]))
    d2, F2 = e.gradient(u)
    _check_scalars(name, f"{kind}_gradient", ref, F2, d2)
    e.close()


@pytest.mark.parametrize("name,kind", LDS, ids=LDS_IDS)
def test_lds_fused(monkeypatch, name, kind):
    """ocg_hessian (k_pipeline: psi || xi, the xiH workers and a workgroup per row behind publication flags,
    then k_row_overlaps): all rows, the subset [1, N-2], a shuffled row list"""
    u, ref = T.traj_controls(name), T.traj_reference(name)
    N = len(u)
    e = _engine(monkeypatch, name, kind)
    shuffled = [int(i) for i in np.random.default_rng(5).permutation(np.arange(1, N - 1))]
    assert shuffled != sorted(shuffled)
    for label, rows in (("all", None), ("ends", [1, N - 2]), ("shuffled", shuffled)):
        tag = f"{kind}_fused_{label}"
        H, divT, F = e.hessian(u, rows)
        _check_scalars(name, tag, ref, F, divT, e.fidelities())
        _check_H(name, tag, ref, H, rows)
        _check_states(name, tag, e, ref)
    e.close()


MULTI = [(n, k, K) for n, k in LDS for K in (2, 8)]


@pytest.mark.parametrize("name,kind,K", MULTI, ids=["%s-%s-K%d" % m for m in MULTI])
def test_lds_multi(monkeypatch, name, kind, K):
    """ocg_hessian_multi and ocg_gradient_multi: K distinct control vectors in [2, 10], every member against
    its own dense reference.  K = 2 lays the controls out in full-size slots; K = 8 reaches
    OCG_MULTI_SHARE_K (default 8), from which the row states take the half-size P2() layout.  K = 8 runs at
    N_t = 6 (the case's own N_t or the 6-point prefix of its controls).  The context keeps control 0's
    trajectories."""
    n = 6 if K == 8 else None
    us = np.array([T.traj_controls(name, n, k) for k in range(K)])
    refs = [T.traj_reference(name, n, k) for k in range(K)]
    N = us.shape[1]
    e = _engine(monkeypatch, name, kind)
    H, divT, F = e.hessian_multi(us)
    for k in range(K):
        tag = f"{kind}_multi{K}_hessian_{k}"
        _check_scalars(name, tag, refs[k], F[k], divT[k])
        _check_H(name, tag, refs[k], H[k])
    fid = e.fidelities()
    assert _fig(name, f"{kind}_multi{K}_fid", np.abs(fid - refs[0]["fid"]).max()) <= _bound(name, "fid")
    _check_states(name, f"{kind}_multi{K}_hessian", e, refs[0], (N - 1,))
    # another member first: the kept trajectories follow it
    order = [1, 0] + list(range(2, K))
    dG, FG = e.gradient_multi(us[order])
    for pos, k in enumerate(order):
        _check_scalars(name, f"{kind}_multi{K}_gradient_{k}", refs[k], FG[pos], dG[pos])
    a, b = D.deviation(refs[1]["psi"][-1], D.dense_of(e.state(0, N - 1)))
    assert _fig(name, f"{kind}_multi{K}_gradient_state", max(a, b)) <= _bound(name, "state")
    e.close()


@pytest.mark.parametrize("name,kind", [(n, k) for n in ("T_L5p5Q5", "T_L5p6Q5") for k in LDS_KINDS],
                         ids=["%s-%s" % (n, k) for n in ("T_L5p5Q5", "T_L5p6Q5") for k in LDS_KINDS])
def test_lds_back_to_back(monkeypatch, name, kind):
    """one context: hessian at N_t = 9, at N_t = 6 with other controls, then hessian_multi with K = 2 --
    the flag layout is reset and the slots are reused"""
    e = _engine(monkeypatch, name, kind)
    for label, n, k in (("n9", 9, 0), ("n6", 6, 1)):
        u, ref = T.traj_controls(name, n, k), T.traj_reference(name, n, k)
        H, divT, F = e.hessian(u)
        _check_scalars(name, f"{kind}_b2b_{label}", ref, F, divT, e.fidelities())
        _check_H(name, f"{kind}_b2b_{label}", ref, H)
    us = np.array([T.traj_controls(name, 9, k) for k in (2, 3)])
    H, divT, F = e.hessian_multi(us)
    for i, k in enumerate((2, 3)):
        ref = T.traj_reference(name, 9, k)
        _check_scalars(name, f"{kind}_b2b_multi_{i}", ref, F[i], divT[i])
        _check_H(name, f"{kind}_b2b_multi_{i}", ref, H[i])
    _check_states(name, f"{kind}_b2b_multi", e, T.traj_reference(name, 9, 2))
    e.close()


# ------------------------------------------------------------------------------------------ HBM engine
@pytest.mark.parametrize("name", T.TRAJ_HBM)
def test_hbm_stored(monkeypatch, name):
    """OCG_HBM_PIPE=0: ocg_hessian on the two-phase path, the explicit driver sequence, ocg_hessian again
    (the trajectories of u are on the device: the reuse path), and hessian_rows in two halves"""
    u, ref = T.traj_controls(name), T.traj_reference(name)
    N = len(u)
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_PIPE=0)
    for tag in ("hbm_stored", "hbm_reuse"):
        if tag == "hbm_reuse":
            e.propagate(u, 3)
        H, divT, F = e.hessian(u)
        _check_scalars(name, tag, ref, F, divT, e.fidelities())
        _check_H(name, tag, ref, H)
    st = e.path_stats()
    assert st["pipe_runs"] == 0 and st["ckpt_runs"] == 0
    H, divT, F, fid = _unfused(e, u)
    _check_scalars(name, "hbm_unfused", ref, F, divT, fid)
    _check_H(name, "hbm_unfused", ref, H)
    _check_final_ranks(name, e, ref)
    _check_states(name, "hbm_unfused", e, ref)
    rows = list(range(1, N - 1))
    parts = []
    for label, sub in (("even", rows[0::2]), ("odd", rows[1::2])):
        parts.append(e.hessian_rows(u, sub, F, divT))
        _check_H(name, f"hbm_rows_{label}", ref, parts[-1], sub)
    # rows write disjoint entries ((i, j >= i) and their mirrors): the halves add up exactly
    assert np.array_equal(parts[0] + parts[1], H)
    e.close()


@pytest.mark.parametrize("name", T.TRAJ_HBM)
def test_hbm_pipelined(monkeypatch, name):
    """OCG_HBM_PIPE=1: psi + rows || dH || xi on three streams (hbm_hessian_pipe)"""
    u, ref = T.traj_controls(name), T.traj_reference(name)
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_PIPE=1)
    H, divT, F = e.hessian(u)
    st = e.path_stats()
    assert st["pipe_runs"] == 1 and st["pipe_fallbacks"] == 0 and st["ckpt_runs"] == 0
    _check_scalars(name, "hbm_pipe", ref, F, divT, e.fidelities())
    _check_H(name, "hbm_pipe", ref, H)
    _check_final_ranks(name, e, ref)
    _check_states(name, "hbm_pipe", e, ref)
    sub = [1, len(u) - 2]
    H, divT, F = e.hessian(T.traj_controls(name, None, 1), sub)     # other controls: nothing to reuse
    ref1 = T.traj_reference(name, None, 1)
    assert e.path_stats()["pipe_runs"] == 2
    _check_scalars(name, "hbm_pipe_ends", ref1, F, divT)
    _check_H(name, "hbm_pipe_ends", ref1, H, sub)
    e.close()


@pytest.mark.parametrize("mid", ["1", "0"])
def test_hbm_checkpointed(monkeypatch, mid):
    """OCG_HBM_CKPT=3 at N_t = 7: psi_t / xi_t kept every 3 steps, segments recomputed, with divT from the
    meet-in-the-middle pass (mid 1) and from the first row pass (mid 0).  No trajectories are kept."""
    name = "T_L9p3Q9"
    u, ref = T.traj_controls(name), T.traj_reference(name)
    assert len(u) == 7
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_CKPT=3, OCG_HBM_CKPT_MID=mid)
    H, divT, F = e.hessian(u)
    st = e.path_stats()
    assert st["ckpt_runs"] == 1 and st["ckpt_k"] == 3 and st["pipe_runs"] == 0
    _check_scalars(name, f"hbm_ckpt_mid{mid}", ref, F, divT)
    _check_H(name, f"hbm_ckpt_mid{mid}", ref, H)
    sub = [2, 5]
    H, _, _ = e.hessian(u, sub)
    _check_H(name, f"hbm_ckpt_mid{mid}_sub", ref, H, sub)
    e.close()


GRADIENT = [("T_L9p3Q9", None), ("T_L8p4Q8", None), ("T_L8p4Q8_r15_17", None), ("T_L5p5Q5", None), ("T_L5p5Q5", 6)]


@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("name,n", GRADIENT, ids=["%s-n%s" % (a, b or "t") for a, b in GRADIENT])
def test_hbm_gradient(monkeypatch, name, n, mode):
    """ocg_gradient on the stored path (OCG_HBM_MID=0) and meeting in the middle (OCG_HBM_MID=1, no
    trajectories kept), at odd N_t (7, 9) and even N_t (6)"""
    u, ref = T.traj_controls(name, n), T.traj_reference(name, n)
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_MID=mode)
    divT, F = e.gradient(u)
    _check_scalars(name, f"hbm_gradient_mid{mode}_n{len(u)}", ref, F, divT, e.fidelities() if mode == "0" else None)
    e.close()


def test_hbm_gradient_multi(monkeypatch):
    """ocg_gradient_multi, K = 3: one lockstep batch of 6 chains"""
    name, K = "T_L9p3Q9", 3
    us = np.array([T.traj_controls(name, None, k) for k in range(K)])
    e = _engine(monkeypatch, name, "hbm")
    divT, F = e.gradient_multi(us)
    for k in range(K):
        _check_scalars(name, f"hbm_gradient_multi_{k}", T.traj_reference(name, None, k), F[k], divT[k])
    ref = T.traj_reference(name)
    assert _fig(name, "hbm_gradient_multi_fid", np.abs(e.fidelities() - ref["fid"]).max()) <= _bound(name, "fid")
    a, b = D.deviation(ref["psi"][-1], D.dense_of(e.state(0, len(us[0]) - 1)))
    assert _fig(name, "hbm_gradient_multi_state", max(a, b)) <= _bound(name, "state")
    e.close()


@pytest.mark.parametrize("name", ["T_L8p4Q8", "T_L8p4Q8_r15_17"])
@pytest.mark.parametrize("fast", ["0", "1"])
def test_hbm_gauge_moves(monkeypatch, name, fast):
    """the stored getHessian with the certified gauge moves on (OCG_HBM_FASTGAUGE=1) and off (0: the eigen
    path only).  On full-rank flat spectra every move certifies; with the evolved-init target the early ones
    may not.  (The certified share is not among the path counters, so none is reported.)"""
    u, ref = T.traj_controls(name), T.traj_reference(name)
    e = _engine(monkeypatch, name, "hbm", OCG_HBM_PIPE=0, OCG_HBM_FASTGAUGE=fast)
    H, divT, F = e.hessian(u)
    _check_scalars(name, f"hbm_fastgauge{fast}", ref, F, divT, e.fidelities())
    _check_H(name, f"hbm_fastgauge{fast}", ref, H)
    _check_states(name, f"hbm_fastgauge{fast}", e, ref)
    e.close()
