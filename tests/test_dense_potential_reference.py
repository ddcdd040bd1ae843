"""The references of test_potential_gpu.py, pinned on the CPU (dense_potential.py; no GPU):

* composition: ed.exact_step with eps equals E exact_step E, E = prod_k exp(-i tau eps_k n_k / 2), to 1e-14 on
  (5,5,5) and (4,4,7), forward and backward; eps = None is bit for bit the step without the keyword;
* sensitivities: sum_t w_t s[t, k] (trapezoid weights) against the central difference of the dense cost in
  eps_k at h = 1e-4, within ten times the figure recorded in tests/golden/dense_potential.json ("fd").  The
  recorded figures are 1.5e-4 .. 5.3e-3 of max_k |sum_t w_t s|, far above the stencil's own error (about
  1e-8): xi_t is carried back by BH_tDMRG::step with tau = -dt, which sweeps the bonds in the forward order
  and so is the inverse of the forward step only to the order of the splitting; <xi_t|psi_t> drifts along t
  by the same amount (printed).  The gradient in U has the same property;
* oracle anchor: the oracle-composed reference (the CPU oracle's step, apply_dH and overlaps with exact E
  passes on the compact blocks, getHessian by calcHessianRow) stays within WELL_POSED = 1e-11 of dense on
  every case and quantity, and the recorded figures (make_dense_potential.py), from which the device test
  takes its bounds, are what it gives now;
* the potentials are what they claim: asymmetric, no two sites equal, the steep half-phase argument near 10."""
import importlib.util
import json
import os

import numpy as np
import pytest

import dense_potential as P
import dense_reference as D
import dense_trajectory as T
import oracle_ffi as O
from optimalcontrolmps_amd import ed

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "dense_potential.json")) as _f:
    GOLDEN = json.load(_f)

CASES = list(P.POT_CASES)


@pytest.fixture(scope="module")
def measured():
    spec = importlib.util.spec_from_file_location("make_dense_potential",
                                                  os.path.join(HERE, "golden", "make_dense_potential.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(D, T, P, O)


def _e_dense(v, L, p, eps, tau):
    g = np.indices((p,) * L).reshape(L, -1)
    return v * np.exp(-0.5j * tau * (eps[:, None] * g).sum(axis=0))


@pytest.mark.parametrize("name", ["T_L5p5Q5", "T_L4p4Q7"])
@pytest.mark.parametrize("forward", [True, False])
def test_composition_identity(name, forward):
    L, p, _ = T.traj_shape(name)
    (_, _, psi), _ = T.traj_states(name)
    eps, tau = P.potential(name), D.DT if forward else -D.DT
    a = ed.exact_step(psi, L, p, D.J, D.DT, 3.0, 7.0, forward, eps=eps)
    b = _e_dense(ed.exact_step(_e_dense(psi, L, p, eps, tau), L, p, D.J, D.DT, 3.0, 7.0, forward), L, p, eps, tau)
    dev = np.abs(a - b).max()
    print(f"FIG {name} forward {forward} composition {dev:.3e}")
    assert dev <= 1e-14
    assert np.abs(a - ed.exact_step(psi, L, p, D.J, D.DT, 3.0, 7.0, forward)).max() > 1e-3    # eps is felt
    assert np.array_equal(ed.exact_step(psi, L, p, D.J, D.DT, 3.0, 7.0, forward, eps=None),
                          ed.exact_step(psi, L, p, D.J, D.DT, 3.0, 7.0, forward))


def test_ed_hamiltonian_takes_the_potential():
    L, p, N = 4, 3, 4
    eps = np.array([0.3, -1.1, 0.7, 2.0])
    confs, _ = ed.sector_basis(L, p, N)
    H0, H1 = ed.bh_hamiltonian(L, p, N, 1.0, 2.5), ed.bh_hamiltonian(L, p, N, 1.0, 2.5, eps)
    assert np.array_equal(H0, ed.bh_hamiltonian(L, p, N, 1.0, 2.5, None))
    assert np.allclose(H1 - H0, np.diag([float(np.dot(eps, c)) for c in confs]), rtol=0, atol=1e-15)
    g0, g1 = ed.ground_state_full(L, p, N, 1.0, 2.5), ed.ground_state_full(L, p, N, 1.0, 2.5, eps)
    assert np.array_equal(g0[0], ed.ground_state_full(L, p, N, 1.0, 2.5, None)[0])
    assert abs(np.vdot(g0[0], g1[0])) < 0.99 and g1[1] != g0[1]


def test_e_pass_is_the_dense_e():
    name = "T_L4p4Q7"
    shape = T.traj_shape(name)
    (dims, data, psi), _ = T.traj_states(name)
    eps = P.potential(name)
    w = ed.full_from_mps(dims, P.e_pass(dims, data, shape, eps, -D.DT), *shape)
    assert np.abs(w - _e_dense(psi, shape[0], shape[1], eps, -D.DT)).max() <= 1e-15


@pytest.mark.parametrize("name", CASES)
def test_sensitivities_against_central_difference(measured, name):
    ref = P.pot_reference(name)
    drift = np.abs(np.array([np.vdot(ref["xi"][t], ref["psi"][t]) for t in range(len(ref["divT"]))])
                   - np.conj(ref["F"])).max()
    got, rec = measured["fd"][name], GOLDEN["fd"][name]
    print(f"FIG {name} fd {got:.3e} recorded {rec:.3e} drift of <xi_t|psi_t> {drift:.3e}")
    assert got <= 10.0 * rec


@pytest.mark.parametrize("name", CASES)
def test_oracle_anchor(measured, name):
    assert sorted(measured["cases"][name]) == sorted(GOLDEN["cases"][name]) == P.KEYS
    for key, v in measured["cases"][name].items():
        print(f"FIG {name} composed_vs_dense_{key} {v:.3e} recorded {GOLDEN['cases'][name][key]:.3e}")
        assert v <= D.WELL_POSED
        assert v <= max(1e-13, 3.0 * GOLDEN["cases"][name][key])    # the fixture is not stale


def test_fixture_lists_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(GOLDEN["fd"]) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_potentials_are_what_they_claim(name):
    eps = P.potential(name)
    traj, _, steep = P.POT_CASES[name]
    L, p, _ = T.traj_shape(traj)
    assert eps.shape == (L,)
    assert min(abs(a - b) for i, a in enumerate(eps) for b in eps[:i]) > 1e-3      # no two sites equal
    assert np.abs(eps - eps[::-1]).max() > 0.5                                       # asymmetric
    if steep:
        assert eps[1] == P.STEEP and 0.5 * D.DT * P.STEEP * (p - 1) > 3.0 > np.pi / 4
    # the potential changes the trajectory visibly: F moves by far more than any bound
    assert abs(P.pot_reference(name)["F"] - T.traj_reference(traj)["F"]) > 1e-3
