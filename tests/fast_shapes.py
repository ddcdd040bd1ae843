"""The chain shapes on which the one-wave padded chain (csrc/fast_chain.hpp, fast_overlap.hpp, host plan
fast_plan.hpp) is tested beyond config 1: one shape per class of plan that build_fast_plan accepts, the
rejected neighbours at the ragged edges of the accepted set, the truncation settings, and well-posed inputs.
Shared by test_fast_shapes_cpu.py (emulator), test_fast_plan_host.py and test_fast_shapes_gpu.py; the class
labels are backed by tests/golden/fast_plan_census.json (test_fast_shapes_cpu.test_table_labels).

Inputs.  An ED ground state is reflection symmetric: its Schmidt weights of bond b, sector q tie with those
of bond L - b, sector Q - q, and whenever Maxm or the cutoff cuts through such a pair the kept set is
arbitrary (two correct implementations then differ by 1e-7 .. 0.16 in the overlap at identical bond
dimensions).  The step inputs are therefore tilted: the ground state at (J, U) = (1, 2) with the amplitude
of configuration n multiplied by exp(-tilt sum_k k n_k), normalised.  tilt = 0.37 unless the table says
otherwise."""
import functools

import numpy as np

from optimalcontrolmps_amd import ed

J, DT, NSTEPS = 1.0, 0.01, 3
TILT = 0.37
U_TILTED, U_TARGET = 2.0, 10.0

# (Maxm, cutoff): nothing binds / Maxm binds / Maxm binds below the order of the Gram blocks with no
# cutoff / the cutoff binds
SETTINGS = [(5000, 1e-8), (3, 1e-8), (2, 0.0), (5000, 1e-3)]

# (L, p, Q): (class, what the census must show for the label to hold, tilt)
ACCEPTED = {
    (2, 3, 2): ("single gate", {"nops": 1, "ns": 0}, TILT),
    (3, 2, 2): ("hard core, odd L", {"nops": 3, "maxr": 0}, TILT),
    (4, 3, 6): ("order-2 Jacobi only", {"maxr": 1}, TILT),
    (5, 2, 3): ("order-2 Jacobi only", {"maxr": 1}, TILT),
    (4, 4, 7): ("four Gram groups, Q > L", {"ngrp": 4}, TILT),
    (5, 3, 8): ("level cut binding (Q = 8 of at most 10), Q > L", {"maxr": 1, "T": 4}, TILT),
    (6, 2, 3): ("9 operations, hard core, Q < L", {"nops": 9}, TILT),
    (6, 6, 3): ("9 operations, p = 6, Q < L", {"nops": 9}, TILT),
    (7, 3, 3): ("11 operations", {"nops": 11}, TILT),
    (8, 2, 5): ("13 operations, hard core", {"nops": 13}, TILT),
    (8, 6, 2): ("13 operations, p = 6", {"nops": 13}, TILT),
    (5, 5, 5): ("anchor: config 1", {"nops": 7, "ngrp": 4, "maxr": 3}, TILT),
    (5, 6, 5): ("anchor: p = 6", {"nops": 7, "ngrp": 4, "maxr": 3}, TILT),
}

# rejected neighbours: the why_not text build_fast_plan must give (the general chain steps them)
REJECTED = {
    (4, 4, 6): "more than four Gram blocks of order >= 2",
    (8, 2, 4): "bond sector bound above the unrolled maximum",
    (5, 5, 6): "bond sector bound above the unrolled maximum",
    (6, 3, 4): "bond sector bound above the unrolled maximum",
    (3, 7, 3): "local dimension above 6",
}

CENSUS_RANGE = [(L, p, Q) for L in range(2, 9) for p in range(2, 8) for Q in range(1, 9) if Q <= L * (p - 1)]


def shape_id(s):
    return "L%dp%dQ%d" % tuple(s)


def tilt_of(shape):
    return ACCEPTED[shape][2] if shape in ACCEPTED else TILT


@functools.lru_cache(maxsize=None)
def _ground_full(L, p, Q, U):
    return ed.ground_state_full(L, p, Q, J, U)[0]


@functools.lru_cache(maxsize=None)
def tilted_state(L, p, Q):
    """(dims, data) of the tilted U = 2 ground state (module docstring)"""
    g = np.indices((p,) * L).reshape(L, -1)
    full = _ground_full(L, p, Q, U_TILTED) * np.exp(-tilt_of((L, p, Q)) * (np.arange(1, L + 1)[:, None] * g).sum(0))
    return ed.mps_from_full(full / np.linalg.norm(full), L, p, Q)


@functools.lru_cache(maxsize=None)
def ground_state(L, p, Q, U=U_TARGET):
    """(dims, data) of the ED ground state at (J, U): overlap operand and getHessian target, never stepped
    under a binding truncation"""
    return ed.mps_from_full(_ground_full(L, p, Q, U), L, p, Q)


def controls(L, p, Q, n=NSTEPS + 1):
    """n controls in [2, 10] (n - 1 steps)"""
    return np.random.default_rng(L * 100 + p * 10 + Q).uniform(2.0, 10.0, n)


STEPPED = (2, 0.0)  # (Maxm, cutoff) of the stepped overlap operand


def overlap_pairs(shape, step):
    """the three (dims, data) pairs of the overlap tests: (tilted, U = 10 ground state), (ground state,
    stepped), (stepped, stepped).  stepped = step(tilted, controls): 3 forward steps at STEPPED, after which
    the bond dimensions sit below the padded bounds wherever a bond is wider than 2"""
    a, b = tilted_state(*shape), ground_state(*shape)
    c = step(a, controls(*shape))
    return [(a, b), (b, c), (c, c)]
