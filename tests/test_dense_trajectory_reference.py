"""The inputs and the reference of test_dense_trajectory_gpu.py, pinned on the CPU (dense_trajectory.py; no
GPU):

* oracle anchor: on every trajectory case the CPU oracle's getHessian at the device test's settings (cutoff
  1e-14, Maxm 512) stays within WELL_POSED = 1e-11 of the state-vector reference in F, divT, the fidelities,
  H (against S = max|A| + max|B|) and the stored states, and the recorded figures
  (tests/golden/dense_trajectories.json, make_dense_trajectories.py), from which the device test takes its
  bounds, are what the oracle gives now;
* the inputs are what they claim: 0.3 <= |F| <= 0.95 (the evolved-init case: >= 0.3 only), both terms of H
  at least a fifth of S, a conjugated F or divT visibly away, full cases at the rank bound md, and a final
  psi whose Schmidt ranks are beyond argument;
* the reference is consistent with itself: H from a second computation that carries the row state
  unnormalised through its own copy of the gate sequence, and symmetry."""
import importlib.util
import json
import os

import numpy as np
import pytest

import dense_reference as D
import dense_trajectory as T
import oracle_ffi as O

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "dense_trajectories.json")) as _f:
    GOLDEN = json.load(_f)

CASES = list(T.TRAJ_CASES)


@pytest.fixture(scope="module")
def measured():
    spec = importlib.util.spec_from_file_location("make_dense_trajectories",
                                                  os.path.join(HERE, "golden", "make_dense_trajectories.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(D, T, O)


@pytest.mark.parametrize("name", CASES)
def test_oracle_anchor(measured, name):
    assert sorted(measured[name]) == sorted(GOLDEN[name]) == ["F", "H", "divT", "fid", "state"]
    for key, v in measured[name].items():
        print(f"FIG {name} oracle_vs_dense_{key} {v:.3e} recorded {GOLDEN[name][key]:.3e}")
        assert v <= D.WELL_POSED
        assert v <= max(1e-13, 3.0 * GOLDEN[name][key])     # the fixture is not stale


def test_fixture_lists_the_cases():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_inputs_are_what_they_claim(name):
    L, p, Q, lo, hi, seed, nt, mix = T.TRAJ_CASES[name]
    shape = (L, p, Q)
    (di, _, init), (dt, _, target) = T.traj_states(name)
    ref = T.traj_reference(name)
    assert len(ref["divT"]) == nt
    assert abs(np.linalg.norm(init) - 1.0) <= 1e-14 and abs(np.linalg.norm(target) - 1.0) <= 1e-14
    F, divT, S = ref["F"], ref["divT"], T.hessian_scale(ref)
    print(f"FIG {name} census widest {D.md_of(*shape).max()} |F| {abs(F):.3f} max|A| {np.abs(ref['A']).max():.3e} "
          f"max|B| {np.abs(ref['B']).max():.3e} max|H| {np.abs(ref['H']).max():.3e}")
    assert abs(F) >= 0.3
    if mix:
        assert abs(F) <= 0.95
    assert np.abs(ref["A"]).max() >= 0.2 * S and np.abs(ref["B"]).max() >= 0.2 * S
    assert abs(F - np.conj(F)) >= 1e-3
    assert np.abs(divT - np.conj(divT)).max() >= 0.1 * np.abs(divT).max()
    md = D.md_of(*shape)
    if name in T.TRAJ_FULL:
        assert np.array_equal(di, md) and np.array_equal(dt, md)
    else:
        assert (di <= np.minimum(md, hi)).all() and (di < md).any() and (dt <= md).all()
        assert dt.sum(axis=1).max() > di.sum(axis=1).max()      # the ranks grow along the trajectory
    # the bond dimensions of the final psi are beyond argument
    ranks, above, below = D.schmidt_ranks(ref["psi"][-1], shape)
    assert above >= D.RANK_ABOVE and below <= D.RANK_BELOW and (ranks >= di).all()


def test_shapes_are_what_the_table_says():
    import fast_shapes
    assert all(T.traj_shape(n) in fast_shapes.ACCEPTED for n in T.TRAJ_LDS)     # one-wave plans exist
    assert fast_shapes.ACCEPTED[T.traj_shape("T_L4p4Q7")][0].startswith("four Gram groups")
    assert D.md_of(8, 4, 8).max() == 31 and D.md_of(9, 3, 9).max() == 19
    assert T.TRAJ_CASES["T_L4p4Q7"][6] == T.TRAJ_CASES["T_L8p4Q8"][6] == 6 and T.TRAJ_CASES["T_L9p3Q9"][6] == 7


@pytest.mark.parametrize("name", CASES)
def test_reference_is_consistent_with_itself(name):
    ref, u = T.traj_reference(name), T.traj_controls(name)
    N, S = len(u), T.hessian_scale(ref)
    H = ref["H"]
    assert np.array_equal(H, H.T) and np.array_equal(H, ref["A"] + ref["B"])
    assert not H[0].any() and not H[N - 1].any() and H[1:N - 1, 1:N - 1].all()
    dev = np.abs(T.dense_hessian_raw(ref, T.traj_shape(name), u) - H).max()
    print(f"FIG {name} second_computation {dev / S:.3e}")
    assert dev <= 1e-13 * S
    assert np.allclose(ref["grad"], D.DT * (1j * ref["divT"] * ref["F"]).real, rtol=0, atol=0)
    assert abs(ref["fid"][-1] - abs(ref["F"]) ** 2) <= 1e-14


def test_a_prefix_of_the_controls_is_another_trajectory():
    """the 6-point prefix used beside K = 8, and the k-th control vectors, are distinct inputs"""
    a, b = T.traj_controls("T_L5p5Q5"), T.traj_controls("T_L5p5Q5", 6)
    assert len(a) == 9 and np.array_equal(a[:6], b)
    us = np.array([T.traj_controls("T_L5p5Q5", 6, k) for k in range(8)])
    assert us.min() >= 2.0 and us.max() <= 10.0
    assert all(np.abs(us[i] - us[j]).max() > 0.5 for i in range(8) for j in range(i))
