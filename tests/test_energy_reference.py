"""The numpy restatement of ocg_observe_moments' channel recursion
(energy_reference.moments_ref) against the dense moments from the state vector
and ed.bh_hamiltonian in the sector basis, to 1e-12 (norm2 + max |moment|)."""
import numpy as np
import pytest

import energy_reference as E
import spectrum_reference as S
from conftest import state_key
from optimalcontrolmps_amd import ed


def _check(dims, data, L, p, Q):
    ref = E.moments_ref(dims, data, L, p, Q)
    den = E.moments_of_mps(dims, data, L, p, Q)
    dev = float(np.abs(ref - den).max())
    print(f"moments {np.array2string(den, precision=6)}: max deviation {dev:.3e} "
          f"({dev / E.tol_scale(den):.3e} of the scale)")
    assert dev <= 1e-12 * E.tol_scale(den)
    return ref, den


def test_ed_ground_state(states):
    L, p, Q, J, U = 5, 5, 5, 1.0, 2.5
    k = state_key(L, p, Q, J, U)
    ref, _ = _check(states[k + "/dims"], states[k + "/data"], L, p, Q)
    e0 = ed.ground_state_full(L, p, Q, J, U)[1]
    assert abs(ref[0] - 1) < 1e-12 and abs(E.energy(ref, J, U) - e0) < 1e-12
    assert abs(E.variance(ref, J, U)) < 1e-11
    assert abs(ref[6]) < 1e-12  # d<D>/dt = 0 in an eigenstate


def test_oracle_evolved_truncated_chain():
    import oracle_ffi as O
    L, p, Q, J = 6, 4, 6, 1.0
    ini = O.MPS(L, p, Q, *ed.mps_from_full(ed.ground_state_full(L, p, Q, J, 2.0)[0], L, p, Q))
    m = O.Stepper(L, p, Q, J, 0.02, 1e-12, 12).steps(ini, np.linspace(2.0, 9.0, 12))
    assert m.bond_dims().max() == 12
    ref, _ = _check(m.dims, m.data, L, p, Q)
    assert abs(ref[6]) > 1e-3  # <D> moves along the ramp: the imaginary part of <K D> is there


@pytest.mark.parametrize("seed", [3, 4])
def test_random_complex_states_with_a_zero_padded_sector(seed):
    L, p, Q = 5, 4, 5
    dims, data = S.random_mps(np.random.default_rng(seed), L, p, Q, 1, 3)
    ref, _ = _check(dims, data, L, p, Q)
    assert abs(ref[0] - 1) > 1e-2 and abs(ref[6]) > 1e-6 * ref[0]
    d2, x2 = S.pad_sector(dims, data, L, p, Q, 2, 1)
    r2, _ = _check(d2, x2, L, p, Q)
    assert np.abs(r2 - ref).max() <= 1e-13 * E.tol_scale(ref)


def test_level_cut_below_the_particle_number():
    """p - 1 < Q: a+ hits the level cut, sectors are empty and partners are missing"""
    L, p, Q = 5, 3, 5
    _check(*ed.mps_from_full(ed.ground_state_full(L, p, Q, 1.0, 8.0)[0], L, p, Q), L, p, Q)
    _check(*S.random_mps(np.random.default_rng(5), L, p, Q, 1, 3), L, p, Q)


def test_hard_core():
    L, p, Q = 6, 2, 3
    ref, _ = _check(*S.random_mps(np.random.default_rng(6), L, p, Q, 1, 3), L, p, Q)
    assert ref[2] == 0 and ref[4] == 0 and ref[5] == 0 and ref[6] == 0  # D = 0 at p = 2


def test_mott_product_state():
    import observe_reference as R
    for L, p, kk in ((5, 3, 16.0), (5, 2, 0.0), (4, 5, 12.0)):
        ref, _ = _check(*R.fock(L, p, L, [1] * L), L, p, L)
        assert np.abs(ref - [1.0, 0.0, 0.0, kk, 0.0, 0.0, 0.0]).max() < 1e-14
    ref, _ = _check(*R.fock(4, 3, 4, [2, 0, 1, 1]), 4, 3, 4)
    assert ref[2] == 1.0 and ref[4] == 1.0
