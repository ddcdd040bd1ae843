"""The numpy restatement of ocg_observe_strings' block contraction (string_reference.strings_ref) against the
dense state vector, sum over the Fock configurations of |amp|^2 prod_k f[k][n_k], to 1e-12 of the scale
norm2 prod_k max_n |f[k][n]|."""
import numpy as np
import pytest

import observe_reference as R
import spectrum_reference as S
import string_reference as T
from optimalcontrolmps_amd import ed


def random_tables(rng, nops, L, p):
    return rng.normal(size=(nops, L, p)) + 1j * rng.normal(size=(nops, L, p))


def support_variants(rng, L, p):
    """empty, one-site, [1, L], [1, 1], [L, L], an interior support, and a table with zeros"""
    f = T.identity(L, p, 7)
    rnd = random_tables(rng, 7, L, p)
    mid = (L + 1) // 2
    f[1, mid - 1] = rnd[1, mid - 1]
    f[2] = rnd[2]
    f[3, 0] = rnd[3, 0]
    f[4, L - 1] = rnd[4, L - 1]
    lo, hi = (2, L - 1) if L >= 4 else (1, L)
    f[5, lo - 1:hi] = rnd[5, lo - 1:hi]
    f[6] = rnd[6]
    f[6, :, 0] = 0.0
    f[6, L - 1, :] = 0.0
    f[6, L - 1, min(1, p - 1)] = 1.0
    return f


def _check(st, L, p, Q, f):
    ref = T.strings_ref(*st, L, p, Q, f)
    psi = ed.full_from_mps(*st, L, p, Q)
    den = T.strings_dense(psi, L, p, f)
    sc = T.scale(float(np.vdot(psi, psi).real), f)
    dev = float((np.abs(ref - den) / sc).max())
    print(f"{len(f)} operators: deviation {dev:.3e} of the scale")
    assert dev <= 1e-12
    return ref


@pytest.mark.parametrize("seed", [3, 4])
def test_random_complex_states(seed):
    L, p, Q = 5, 4, 5
    rng = np.random.default_rng(seed)
    st = S.random_mps(rng, L, p, Q, 1, 4)
    f = np.concatenate([random_tables(rng, 4, L, p), support_variants(rng, L, p)])
    ref = _check(st, L, p, Q, f)
    assert np.abs(ref.imag).max() > 1e-6 * np.abs(ref).max()
    # a zero-padded sector changes nothing
    pad = S.pad_sector(*st, L, p, Q, 2, 1)
    r2 = _check(pad, L, p, Q, f)
    assert (np.abs(r2 - ref) / T.scale(abs(ref[4]), f)).max() < 1e-13


def test_support_variants():
    L, p, Q = 5, 4, 5
    rng = np.random.default_rng(11)
    st = S.random_mps(rng, L, p, Q, 1, 4)
    f = support_variants(rng, L, p)
    assert [T.support(x) for x in f] == [None, (3, 3), (1, 5), (1, 1), (5, 5), (2, 4), (1, 5)]
    ref = _check(st, L, p, Q, f)
    obs = R.observe_ref(*st, L, p, Q)
    assert abs(ref[0] - obs["norm2"]) <= 1e-12 * obs["norm2"]
    # a one-site support: sum_n f occ
    for m, k in ((1, 3), (3, 1), (4, 5)):
        want = (f[m, k - 1] * obs["occ"][k - 1]).sum()
        assert abs(ref[m] - want) <= 1e-12 * T.scale(obs["norm2"], f)[m]


def test_level_cut_below_the_particle_number():
    rng = np.random.default_rng(5)
    L, p, Q = 5, 3, 5
    _check(S.random_mps(rng, L, p, Q, 1, 3), L, p, Q, support_variants(rng, L, p))
    L, p, Q = 6, 2, 3
    _check(S.random_mps(rng, L, p, Q, 1, 3), L, p, Q, support_variants(rng, L, p))


def test_single_bond():
    L, p, Q = 2, 3, 2
    rng = np.random.default_rng(2)
    _check(S.random_mps(rng, L, p, Q, 1, 1), L, p, Q, support_variants(rng, L, p))


def test_fock_states():
    L, p = 5, 3
    occ = [1, 2, 0, 1, 1]
    st = R.fock(L, p, L, occ)
    rng = np.random.default_rng(9)
    f = random_tables(rng, 3, L, p)
    f[2, 1, 2] = 0.0  # a zero at the occupied level: exactly 0
    ref = _check(st, L, p, L, f)
    want = np.array([np.prod([f[m, k, occ[k]] for k in range(L)]) for m in range(3)])
    assert ref[2] == 0 and np.abs(ref - want).max() <= 1e-15 * np.abs(want).max()


@pytest.fixture(scope="module")
def ed_states():
    L, p, Q, J = 5, 5, 5, 1.0
    return {U: ed.mps_from_full(ed.ground_state_full(L, p, Q, J, U)[0], L, p, Q) for U in (2.5, 50.0)}


def test_ed_ground_states_parity_order(ed_states):
    L, p, Q = 5, 5, 5
    f = T.parity_tables(L, p, 1, 1)
    par = {U: _check(st, L, p, Q, f) for U, st in ed_states.items()}
    for U in par:
        assert np.abs(par[U].imag).max() < 1e-13
    # the Mott insulator's order parameter: larger deep in the insulator, at every distance short of the full chain
    assert (par[50.0].real[:L - 1] > par[2.5].real[:L - 1]).all()
    assert par[50.0].real[L - 2] > 0.9
    # the full chain holds Q = L bosons: (-1)^(Q - L nbar) = 1
    assert abs(par[2.5][L - 1] - 1) < 1e-12


def test_counting_statistics_of_every_block(ed_states):
    L, p, Q = 5, 5, 5
    st = ed_states[2.5]
    obs = R.observe_ref(*st, L, p, Q, rows=tuple(range(1, L + 1)))
    nk = (obs["occ"] * np.arange(p)).sum(1)
    m = np.arange(Q + 1)
    for i in range(1, L + 1):
        for j in range(i, L + 1):
            G = T.strings_ref(*st, L, p, Q, T.counting_tables(L, p, Q, i, j))
            P = T.counting_from(G, obs["norm2"], Q)
            assert P.min() >= -1e-12 and abs(P.sum() - 1) <= 1e-12
            assert abs((m * P).sum() - nk[i - 1:j].sum()) <= 1e-12 * Q
            # <N_A^2> from the nn rows (row k holds <n_k n_l> for l >= k)
            n2 = sum(obs["nn"][k - 1, l - 1] * (1 if l == k else 2)
                     for k in range(i, j + 1) for l in range(k, j + 1))
            assert abs((m * m * P).sum() - n2) <= 1e-12 * Q * Q
