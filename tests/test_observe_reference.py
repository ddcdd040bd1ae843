"""The numpy restatement of ocg_observe's definitions (observe_reference.py)
against the dense state vector, to 1e-12: an ED ground state and an
oracle-evolved, truncated (Maxm 12) L=6, p=4, Q=6 chain whose intermediate
gauge and norm < 1 the gauge-free formulas must not care about."""
import numpy as np

import observe_reference as R
import oracle_ffi as O
from conftest import state_key
from optimalcontrolmps_amd import ed


def _check(dims, data, L, p, Q, rows):
    ref = R.observe_ref(dims, data, L, p, Q, rows)
    den = R.observe_dense(ed.full_from_mps(dims, data, L, p, Q), L, p, rows)
    assert R.max_dev(ref, den) < 1e-12
    assert abs(ref["occ"].sum(-1) - ref["norm2"]).max() < 1e-12
    assert abs((np.arange(p) * ref["occ"]).sum() - Q * ref["norm2"]) < 1e-12
    return ref


def test_reference_on_ed_ground_state(states):
    L, p, Q = 5, 5, 5
    k = state_key(L, p, Q, 1.0, 2.5)
    ref = _check(states[k + "/dims"], states[k + "/data"], L, p, Q, list(range(1, L + 1)))
    assert abs(ref["norm2"] - 1) < 1e-12


def test_reference_on_oracle_evolved_chain():
    L, p, Q = 6, 4, 6
    dims, data = R.fock(L, p, Q, [1] * L)
    orc = O.Stepper(L, p, Q, 1.0, 0.05, 1e-10, 12)
    u = np.linspace(2.0, 5.0, 21)
    m = orc.steps(O.MPS(L, p, Q, dims, data), u, True)
    assert max(m.bond_dims()) == 12
    ref = _check(m.dims, m.data, L, p, Q, [1, 3, 6])
    assert np.abs(ref["ada"].imag).max() > 1e-6        # a complex state: the conjugations matter
    # a state scaled on one site: everything scales with the norm
    d2 = np.array(m.data, np.complex128)
    first = int(np.asarray(m.dims).reshape(L + 1, Q + 1)[1].sum())  # site 1 holds one row per sector of bond 1
    d2[:first] *= 0.5
    r2 = R.observe_ref(m.dims, d2, L, p, Q, [1, 3, 6])
    for key in ("norm2", "occ", "ada", "nn"):
        assert np.abs(np.asarray(r2[key]) - 0.25 * np.asarray(ref[key])).max() < 1e-15
