"""The numpy restatement of ocg_observe_spectrum's block formula
(spectrum_reference.py) against the singular values of the dense state vector:
1e-12 * norm2 on the weights, 1e-12 on the entropies, for an ED ground state
and for a random complex, non-canonical MPS.  On the latter the formula with
the conjugated right environment must miss by more than 1e-3: real states
cannot tell the two apart."""
import numpy as np

import spectrum_reference as S
from conftest import state_key
from optimalcontrolmps_amd import ed


def _devs(ref, den):
    wdev = max(S.weight_dev(a, b) for a, b in zip(ref["weights"], den["weights"]))
    return wdev / den["norm2"], float(np.abs(ref["entropy"] - den["entropy"]).max())


def _check(dims, data, L, p, Q):
    ref = S.spectrum_ref(dims, data, L, p, Q)
    den = S.spectrum_dense(ed.full_from_mps(dims, data, L, p, Q), L, p)
    wdev, sdev = _devs(ref, den)
    print(f"weights {wdev:.3e} of norm2, entropy {sdev:.3e}")
    assert wdev < 1e-12 and sdev < 1e-12
    bond = np.asarray(dims).reshape(L + 1, Q + 1).sum(axis=1)
    for b in range(1, L):
        assert len(ref["weights"][b - 1]) == len(ref["sectors"][b - 1]) == bond[b]
        assert abs(ref["weights"][b - 1].sum() - ref["norm2"]) < 1e-12 * ref["norm2"]
        assert (np.diff(ref["weights"][b - 1]) <= 0).all()
    return ref, den


def test_reference_on_ed_ground_state(states):
    L, p, Q = 5, 5, 5
    k = state_key(L, p, Q, 1.0, 2.5)
    ref, _ = _check(states[k + "/dims"], states[k + "/data"], L, p, Q)
    assert abs(ref["norm2"] - 1) < 1e-12 and ref["entropy"].min() > 0.1


def test_reference_on_random_complex_mps():
    L, p, Q = 5, 4, 5
    dims, data = S.random_mps(np.random.default_rng(11), L, p, Q, 1, 3)
    _, den = _check(dims, data, L, p, Q)
    wrong = S.spectrum_ref(dims, data, L, p, Q, conj_renv=True)
    wdev, _ = _devs(wrong, den)
    print(f"conjugated Renv misses by {wdev:.3e} of norm2")
    assert wdev > 1e-3


def test_zero_padded_sector_adds_one_zero_weight():
    L, p, Q = 4, 2, 1
    psi = np.zeros(p ** L, complex)
    for k in range(L):
        psi[p ** k] = 0.5
    dims, data = ed.mps_from_full(psi, L, p, Q)
    ref = S.spectrum_ref(dims, data, L, p, Q)
    for b in range(1, L):
        assert np.abs(np.sort(ref["weights"][b - 1]) - np.sort([(L - b) / L, b / L])).max() < 1e-14
    d2, x2 = S.pad_sector(dims, data, L, p, Q, 2, 1)
    assert np.abs(ed.full_from_mps(d2, x2, L, p, Q) - psi).max() < 1e-15
    r2 = S.spectrum_ref(d2, x2, L, p, Q)
    assert len(r2["weights"][1]) == len(ref["weights"][1]) + 1 and abs(r2["weights"][1][-1]) <= 1e-15
    assert np.abs(r2["entropy"] - ref["entropy"]).max() < 1e-14
