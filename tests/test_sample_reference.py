"""The numpy restatement of ocg_sample's definition (sample_reference.py) against
the full state vector: the known answers of the counter-based random numbers, and
sample_ref replayed decision by decision against the dense conditionals.

Exemption rule of every replay: a decision whose u lies within 1e-9 of a
normalised dense CDF boundary may fall on either side, the replay continues with
the drawn n, and at most one exempted decision per 1000 shots of a case is
allowed (expected share ~ 2 delta (p-1) L ~ 4e-8 per shot).
"""
import numpy as np
import pytest

import sample_reference as SR
import spectrum_reference as S
from optimalcontrolmps_amd import ed

KNOWN = [
    (0, 0, 0, 1, 0x2a4f111b3be57715, 0.16526896395580137),
    (1, 0, 0, 1, 0x3fa25e1657e024c1, 0.24857128186693034),
    (20261015, 7, 123, 5, 0xd1ee929f7a7b4c49, 0.8200465812064809),
    (2 ** 64 - 1, 200, 999999, 50, 0x3570ae951407bb5c, 0.20875064029317414),
]


@pytest.mark.parametrize("seed,id,shot,k,h,u", KNOWN)
def test_known_answers(seed, id, shot, k, h, u):
    assert SR.hash_of(seed, id, shot, k) == h
    assert SR.uniform_of(h) == u
    if shot < 200 and k <= 8:
        assert SR.uniforms(seed, id, shot + 1, 8)[shot, k - 1] == u


def _replay(dims, data, L, p, Q, nshots, seed, id):
    psi = ed.full_from_mps(dims, data, L, p, Q)
    out = SR.sample_ref(dims, data, L, p, Q, nshots, seed, id)
    assert out["config"].dtype == np.int8 and out["config"].shape == (nshots, L)
    assert (out["config"].sum(axis=1) == Q).all() and out["config"].min() >= 0 and out["config"].max() < p
    assert abs(out["norm2"] - np.vdot(psi, psi).real) <= 1e-12 * out["norm2"]
    r = SR.replay_dense(psi, L, p, out["config"], out["logp"], seed, id)
    print(f"  {nshots} shots: {r}")
    assert r["mismatch"] == 0
    assert r["exempt"] * 1000 <= nshots
    assert r["logp_dev"] <= 1e-12
    return out, psi


def test_ground_state_replay():
    L, p, Q = 5, 5, 5
    psi, _ = ed.ground_state_full(L, p, Q, 1.0, 3.0)
    dims, data = ed.mps_from_full(psi, L, p, Q)
    out, _ = _replay(dims, data, L, p, Q, 1000, 11, 3)
    # the empirical distribution of site 1 against its exact marginal (1000 shots: 5 sigma of a binomial)
    marg = SR.fock_conditionals_dense(psi, [], L, p)
    marg = marg / marg.sum()
    freq = np.bincount(out["config"][:, 0], minlength=p) / 1000.0
    assert (np.abs(freq - marg) <= 5 * np.sqrt(marg * (1 - marg) / 1000.0) + 1e-12).all()


@pytest.mark.parametrize("L,p,Q,lo,hi,nshots", [(5, 5, 5, 1, 3, 2000), (4, 3, 4, 2, 5, 2000), (6, 4, 6, 1, 2, 1000)])
def test_random_complex_mps_replay(L, p, Q, lo, hi, nshots):
    dims, data = S.random_mps(np.random.default_rng(3), L, p, Q, lo, hi)
    _replay(dims, data, L, p, Q, nshots, 20261015, 7)


def test_counter_based_properties_and_amplitudes():
    L, p, Q = 4, 3, 4
    dims, data = S.random_mps(np.random.default_rng(4), L, p, Q, 2, 4)
    a = SR.sample_ref(dims, data, L, p, Q, 60, 5, 2)
    b = SR.sample_ref(dims, data, L, p, Q, 20, 5, 2)
    assert np.array_equal(a["config"][:20], b["config"]) and np.array_equal(a["logp"][:20], b["logp"])
    assert not np.array_equal(a["config"], SR.sample_ref(dims, data, L, p, Q, 60, 6, 2)["config"])
    assert not np.array_equal(a["config"], SR.sample_ref(dims, data, L, p, Q, 60, 5, 3)["config"])
    # amplitudes of every configuration against the state vector; their squares add up to norm2
    psi = ed.full_from_mps(dims, data, L, p, Q)
    cf = SR.all_configs(L, p, Q)
    amp = SR.amplitudes_ref(dims, data, L, p, Q, cf)
    assert np.abs(amp - psi[[SR.flat_index(c, p) for c in cf]]).max() <= 1e-14
    assert abs((np.abs(amp) ** 2).sum() - a["norm2"]) <= 1e-12 * a["norm2"]
    # logp of a shot is ln(|amp|^2 / norm2)
    amps = SR.amplitudes_ref(dims, data, L, p, Q, a["config"])
    assert np.abs(np.log(np.abs(amps) ** 2 / a["norm2"]) - a["logp"]).max() <= 1e-12


def test_zero_state_is_dead():
    L, p, Q = 3, 3, 2
    dims, data = S.random_mps(np.random.default_rng(1), L, p, Q, 1, 2)
    out = SR.sample_ref(dims, 0 * data, L, p, Q, 4, 1, 0)
    assert (out["config"] == -1).all() and np.isneginf(out["logp"]).all()
