"""Wall time of the device observables (ocg_observe) against the only path there
was before: one ocg_get_state copy per state (a lower bound of that path, which
adds the host contraction of correlations.hpp on top).

    python -m optimalcontrolmps_amd.tools.observe_timing [--config 1|4|s1|s4|p1|p4|e1|e4|pairs|strings|all] [--reps R] [--out DIR]

One process; every shape is warmed up; each timed call ends in a device
synchronise (both entry points return only after their results are on the
host); the two paths alternate and the spread (min / median / max) is
reported.  Config 1: L=5, p=5, chi<=80, N_t=201, the LDS engine.  Config 4
slice: L=20, p=7, chi=256 from the warm state, N_t=33, the HBM engine; also the
old path's cost for one state (copy + host expectationValues).  Writes
observe_config1.json / observe_config4.json into --out (default profiles/).

s1 / s4: the entanglement spectra (ocg_observe_spectrum) at the same two
shapes, entropies only and with the weights, alternating with the copy loop;
the path they replace is that loop plus N_t times the host
entanglementEntropy(sites, psi) of one mid-trajectory state, timed by a small
stand-alone program.  Writes observe_spectrum_config1.json /
observe_spectrum_config4.json.

p1 / p4: Fock-state snapshots (ocg_sample, 1024 shots of every state) and the
Mott-state amplitude (ocg_fock_amplitudes) at the same two shapes, alternating
with the copy loop; the path they replace is that loop plus N_t times the host
sampleFock(psi, 1024, seed, t) of one mid-trajectory state, timed on one thread by
a small stand-alone program.  Writes observe_sample_config1.json /
observe_sample_config4.json.

e1 / e4: the energy moments (ocg_observe_moments) of every state at the same two
shapes, alternating with the copy loop alone, which is the lower bound of the
only other route to <H^2> (copy every state out and contract on the host); at
config 1 the chain kernel also alternates with the forced task-list path
(OCG_OBS_ENERGY_CHAIN=0).  Writes observe_energy_config1.json /
observe_energy_config4.json.

pairs: the transition elements (ocg_observe_pairs) of all (xi_t, psi_t) at config 1,
N_t = 201: the chain kernel, the forced task-list path (OCG_OBS_PAIR_CHAIN=0) and
the host route (ocg_get_state of both trajectories plus the numpy block
contraction of tests/pair_reference.py), alternating.  Writes
observe_pairs_config1.json.

strings: the string-operator expectations (ocg_observe_strings) of every psi_t at config 1,
N_t = 201, for two operator sets, the parity-order row from site 1 (L operators) and the
counting statistics of the sites 2..4 (Q + 1 operators): the chain kernels, the forced
task-list path (OCG_OBS_STRING_CHAIN=0) and the host route (ocg_get_state plus the numpy
block contraction of tests/string_reference.py), alternating, and each device route
back to back.  Writes observe_strings_config1.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import tempfile
import time

import numpy as np

from optimalcontrolmps_amd import native
from optimalcontrolmps_amd.native import MPS, Engine

ROOT = native.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden")


def spread(xs):
    xs = sorted(xs)
    return {"min_ms": 1e3 * xs[0], "median_ms": 1e3 * xs[len(xs) // 2], "max_ms": 1e3 * xs[-1], "reps": len(xs)}


def copy_all(eng, which, n, dims, data):
    """the n ocg_get_state copies alone, into preallocated buffers"""
    got = C.c_size_t(0)
    for t in range(n):
        eng._chk(native.lib().ocg_get_state(eng.h, which, t, dims.ctypes.data_as(native.ip),
                                            data.ctypes.data_as(native.dp), eng.cap, C.byref(got)), "ocg_get_state")


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def config1(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 5, 5, 5, 1.0, 0.01, 1e-8, 80, 201
    z = np.load(os.path.join(GOLDEN, "states.npz"), allow_pickle=False)
    ini = MPS(L, p, Q, z["L5_p5_N5_J1_U2.5/dims"], z["L5_p5_N5_J1_U2.5/data"])
    tgt = MPS(L, p, Q, z["L5_p5_N5_J1_U50/dims"], z["L5_p5_N5_J1_U50/data"])
    eng = Engine(L, p, Q, J, dt, cut, maxm)
    eng.set_states(tgt, ini)
    eng.propagate(np.linspace(2.5, 50.0, Nt), 1)
    dims = np.zeros((L + 1) * (Q + 1), np.int32)
    data = np.zeros(2 * eng.cap)
    rows = list(range(1, L + 1))
    cases = {"occ_only": lambda: eng.observe(0, None, (), outputs=("occ",)),
             "all_rows": lambda: eng.observe(0, None, rows),
             "get_state_copies": lambda: copy_all(eng, 0, Nt, dims, data)}
    for f in cases.values():  # warm up every shape
        f()
        f()
    eng.reset_stats()
    t = {k: [] for k in cases}
    for _ in range(reps):     # alternating
        for k, f in cases.items():
            t[k].append(timed(f))
    res = {"config": "1: L=5 p=5 Q=5 chi<=80 N_t=201, LDS engine", "fast_chain": int(eng.info.fast_chain),
           "bond_max": int(eng.observe(0, None, (), outputs=("bond",))["bond"].max())}
    res.update({k: spread(v) for k, v in t.items()})
    res["kind9"] = eng.stats(9)
    for k in ("occ_only", "all_rows"):
        res[k + "_vs_copies"] = res["get_state_copies"]["median_ms"] / res[k]["median_ms"]
    return res


def host_expectation_seconds(state, tool="host_expectation_timing", args=()):
    """copy-free part of the old path for one state: expectationValues(sites, psi, "N") (or, with
    tool="host_entropy_timing", entanglementEntropy(sites, psi)) on the host"""
    src = os.path.join(native.PKG_DIR, "tools", tool + ".cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, tool)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src])
        path = os.path.join(d, "state.bin")
        with open(path, "wb") as f:
            f.write(np.array([state.L, state.p, state.Q, state.dims.size, state.data.size], np.int32).tobytes())
            f.write(state.dims.tobytes() + state.data.tobytes())
        return json.loads(subprocess.run([exe, path] + [str(a) for a in args], capture_output=True, text=True,
                                         check=True).stdout)


def config4(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 20, 7, 20, 1.0, 0.005, 1e-8, 256, 33
    z = np.load(os.path.join(GOLDEN, "c4_warm256.npz"), allow_pickle=False)
    c4 = np.load(os.path.join(GOLDEN, "c4.npz"), allow_pickle=False)
    u = np.load(os.path.join(GOLDEN, "c4_w256h33.npz"), allow_pickle=False)["u"]
    eng = Engine(L, p, Q, J, dt, cut, maxm, engine="hbm")
    eng.set_states(MPS(L, p, Q, c4["w256h/tgt_dims"], c4["w256h/tgt_data"]), MPS(L, p, Q, z["dims"], z["data"]))
    eng.propagate(u, 1)
    dims = np.zeros((L + 1) * (Q + 1), np.int32)
    data = np.zeros(2 * eng.cap)
    cases = {"observe_rows10": lambda: eng.observe(0, None, [10]),
             "get_state_copies": lambda: copy_all(eng, 0, Nt, dims, data)}
    for f in cases.values():
        f()
    eng.reset_stats()
    t = {k: [] for k in cases}
    for _ in range(reps):
        for k, f in cases.items():
            t[k].append(timed(f))
    k9, k7 = eng.stats(9), eng.stats(7)
    res = {"config": "4 slice: L=20 p=7 Q=20 chi=256 (warm state) N_t=33, HBM engine, rows=[10]"}
    res.update({k: spread(v) for k, v in t.items()})
    res["per_state_ms"] = res["observe_rows10"]["median_ms"] / Nt
    res["kind9_per_call"] = {k: v / reps for k, v in k9.items()}
    res["k_gemm_share_of_kind9_time"] = k7["ms"] / k9["ms"] if k9["ms"] else None
    res["kind9_tflops"] = 1e-9 * k9["alg_flops"] / k9["ms"] if k9["ms"] else None
    res["old_path_one_state"] = {"get_state_ms": res["get_state_copies"]["median_ms"] / Nt,
                                 "host_expectationValues_N": host_expectation_seconds(eng.state(0, Nt // 2))}
    return res


def spectrum_cases(eng, Nt, reps, warm):
    """spectrum (entropies only / with the weights), the environments alone (observe occ) and the copy loop,
    alternating; kind 9 (and kind 7) per case from a pass of its own"""
    dims = np.zeros((eng.L + 1) * (eng.Q + 1), np.int32)
    data = np.zeros(2 * eng.cap)
    cases = {"spectrum_entropy": lambda: eng.spectrum(0, None, outputs=("entropy",)),
             "spectrum_weights": lambda: eng.spectrum(0, None),
             "observe_occ": lambda: eng.observe(0, None, (), outputs=("occ",)),
             "get_state_copies": lambda: copy_all(eng, 0, Nt, dims, data)}
    for f in cases.values():
        for _ in range(warm):
            f()
    t = {k: [] for k in cases}
    for _ in range(reps):
        for k, f in cases.items():
            t[k].append(timed(f))
    res = {k: spread(v) for k, v in t.items()}
    for k in ("spectrum_entropy", "observe_occ"):
        eng.reset_stats()
        cases[k]()
        res[k + "_kind9"] = eng.stats(9)
        res[k + "_kind7_ms"] = eng.stats(7)["ms"]
    host = host_expectation_seconds(eng.state(0, Nt // 2), "host_entropy_timing")
    res["host_entanglementEntropy_one_state"] = host
    old = res["get_state_copies"]["median_ms"] + Nt * 1e3 * host["seconds"]
    res["old_path_ms"] = old
    for k in ("spectrum_entropy", "spectrum_weights"):
        res[k + "_vs_old_path"] = old / res[k]["median_ms"]
        res[k + "_vs_copies"] = res["get_state_copies"]["median_ms"] / res[k]["median_ms"]
    # kind 9 of the entropies-only call: its stream time, the k_gemm time inside (kind 7; HBM engine only) and
    # the rest (eigen stages, entropy reduction, the gaps in which the host builds the next task lists).  The
    # occupations call forms the same environments (plus the X products and a close launch per site instead of
    # the spectrum stages), so the difference of the two rests estimates the eigen stages; it is no clean split.
    a, b = res["spectrum_entropy_kind9"], res["observe_occ_kind9"]
    ga, gb = res["spectrum_entropy_kind7_ms"], res["observe_occ_kind7_ms"]
    res["kind9_split_ms"] = {"total": a["ms"], "k_gemm": ga, "rest": a["ms"] - ga,
                             "occupations_call_total": b["ms"], "occupations_call_k_gemm": gb,
                             "eigen_and_entropy_estimate": (a["ms"] - ga) - (b["ms"] - gb)}
    return res


def spectrum1(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 5, 5, 5, 1.0, 0.01, 1e-8, 80, 201
    z = np.load(os.path.join(GOLDEN, "states.npz"), allow_pickle=False)
    ini = MPS(L, p, Q, z["L5_p5_N5_J1_U2.5/dims"], z["L5_p5_N5_J1_U2.5/data"])
    tgt = MPS(L, p, Q, z["L5_p5_N5_J1_U50/dims"], z["L5_p5_N5_J1_U50/data"])
    eng = Engine(L, p, Q, J, dt, cut, maxm)
    eng.set_states(tgt, ini)
    eng.propagate(np.linspace(2.5, 50.0, Nt), 1)
    res = {"config": "1: L=5 p=5 Q=5 chi<=80 N_t=201, LDS engine (no k_gemm: kind 7 is 0)",
           "bond_max": int(eng.observe(0, None, (), outputs=("bond",))["bond"].max())}
    res.update(spectrum_cases(eng, Nt, reps, 2))
    return res


def spectrum4(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 20, 7, 20, 1.0, 0.005, 1e-8, 256, 33
    z = np.load(os.path.join(GOLDEN, "c4_warm256.npz"), allow_pickle=False)
    c4 = np.load(os.path.join(GOLDEN, "c4.npz"), allow_pickle=False)
    u = np.load(os.path.join(GOLDEN, "c4_w256h33.npz"), allow_pickle=False)["u"]
    eng = Engine(L, p, Q, J, dt, cut, maxm, engine="hbm")
    eng.set_states(MPS(L, p, Q, c4["w256h/tgt_dims"], c4["w256h/tgt_data"]), MPS(L, p, Q, z["dims"], z["data"]))
    eng.propagate(u, 1)
    res = {"config": "4 slice: L=20 p=7 Q=20 chi=256 (warm state) N_t=33, HBM engine",
           "sector_max": int(max(eng.state(0, t).dims.max() for t in (0, Nt // 2, Nt - 1)))}
    res.update(spectrum_cases(eng, Nt, reps, 1))
    return res


def sample_cases(eng, Nt, reps, warm, nshots=1024):
    """snapshots (nshots of every state), the Mott amplitude of every state, the environments alone (observe
    occ) and the copy loop, alternating; kind 9 (and kind 7) of the snapshot call from a pass of its own"""
    dims = np.zeros((eng.L + 1) * (eng.Q + 1), np.int32)
    data = np.zeros(2 * eng.cap)
    mott = [[1] * eng.L]
    cases = {"sample": lambda: eng.sample(0, None, nshots, 1),
             "fock_amplitude_mott": lambda: eng.fock_amplitudes(0, None, mott),
             "observe_occ": lambda: eng.observe(0, None, (), outputs=("occ",)),
             "get_state_copies": lambda: copy_all(eng, 0, Nt, dims, data)}
    for f in cases.values():
        for _ in range(warm):
            f()
    t = {k: [] for k in cases}
    for _ in range(reps):
        for k, f in cases.items():
            t[k].append(timed(f))
    res = {"nshots": nshots}
    res.update({k: spread(v) for k, v in t.items()})
    for k in ("sample", "observe_occ"):
        eng.reset_stats()
        cases[k]()
        res[k + "_kind9"] = eng.stats(9)
        res[k + "_kind7_ms"] = eng.stats(7)["ms"]
    host = host_expectation_seconds(eng.state(0, Nt // 2), "host_sample_timing", (nshots,))
    res["host_sampleFock_one_state"] = host
    old = res["get_state_copies"]["median_ms"] + Nt * 1e3 * host["seconds"]   # (the call forms its environments)
    res["old_path_ms"] = old
    res["sample_vs_old_path"] = old / res["sample"]["median_ms"]
    res["sample_vs_copies"] = res["get_state_copies"]["median_ms"] / res["sample"]["median_ms"]
    res["shots_per_second"] = Nt * nshots / (1e-3 * res["sample"]["median_ms"])
    return res


def sample1(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 5, 5, 5, 1.0, 0.01, 1e-8, 80, 201
    z = np.load(os.path.join(GOLDEN, "states.npz"), allow_pickle=False)
    ini = MPS(L, p, Q, z["L5_p5_N5_J1_U2.5/dims"], z["L5_p5_N5_J1_U2.5/data"])
    tgt = MPS(L, p, Q, z["L5_p5_N5_J1_U50/dims"], z["L5_p5_N5_J1_U50/data"])
    eng = Engine(L, p, Q, J, dt, cut, maxm)
    eng.set_states(tgt, ini)
    eng.propagate(np.linspace(2.5, 50.0, Nt), 1)
    res = {"config": "1: L=5 p=5 Q=5 chi<=80 N_t=201, LDS engine (no k_gemm: kind 7 is 0), 1024 shots per state",
           "sector_max": int(max(eng.state(0, t).dims.max() for t in (0, Nt // 2, Nt - 1)))}
    res.update(sample_cases(eng, Nt, reps, 2))
    return res


def sample4(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 20, 7, 20, 1.0, 0.005, 1e-8, 256, 33
    z = np.load(os.path.join(GOLDEN, "c4_warm256.npz"), allow_pickle=False)
    c4 = np.load(os.path.join(GOLDEN, "c4.npz"), allow_pickle=False)
    u = np.load(os.path.join(GOLDEN, "c4_w256h33.npz"), allow_pickle=False)["u"]
    eng = Engine(L, p, Q, J, dt, cut, maxm, engine="hbm")
    eng.set_states(MPS(L, p, Q, c4["w256h/tgt_dims"], c4["w256h/tgt_data"]), MPS(L, p, Q, z["dims"], z["data"]))
    eng.propagate(u, 1)
    res = {"config": "4 slice: L=20 p=7 Q=20 chi=256 (warm state) N_t=33, HBM engine, 1024 shots per state",
           "sector_max": int(max(eng.state(0, t).dims.max() for t in (0, Nt // 2, Nt - 1)))}
    res.update(sample_cases(eng, Nt, reps, 1))
    return res


def energy_cases(eng, Nt, reps, warm, both_paths):
    """the moments of every state (on the chain kernel where the widths allow, and with the task lists
    forced), and the copy loop, alternating; kind 9 per moments case from a pass of its own"""
    dims = np.zeros((eng.L + 1) * (eng.Q + 1), np.int32)
    data = np.zeros(2 * eng.cap)

    def forced_lists():
        os.environ["OCG_OBS_ENERGY_CHAIN"] = "0"
        try:
            return eng.moments(0)
        finally:
            del os.environ["OCG_OBS_ENERGY_CHAIN"]
    cases = {"moments": lambda: eng.moments(0)}
    if both_paths:
        cases["moments_lists"] = forced_lists
    cases["get_state_copies"] = lambda: copy_all(eng, 0, Nt, dims, data)
    for f in cases.values():
        for _ in range(warm):
            f()
    t = {k: [] for k in cases}
    for _ in range(reps):
        for k, f in cases.items():
            t[k].append(timed(f))
    res = {k: spread(v) for k, v in t.items()}
    for k in cases:
        if k.startswith("moments"):
            eng.reset_stats()
            cases[k]()
            res[k + "_kind9"] = eng.stats(9)
            res[k + "_kind7_ms"] = eng.stats(7)["ms"]
            res[k + "_vs_copies"] = res["get_state_copies"]["median_ms"] / res[k]["median_ms"]
    if both_paths:
        res["chain_vs_lists"] = res["moments_lists"]["median_ms"] / res["moments"]["median_ms"]
        a, b = eng.moments(0), forced_lists()
        res["chain_lists_max_rel_dev"] = float(np.abs(a - b).max() / np.abs(b).max())
    return res


def energy1(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 5, 5, 5, 1.0, 0.01, 1e-8, 80, 201
    z = np.load(os.path.join(GOLDEN, "states.npz"), allow_pickle=False)
    ini = MPS(L, p, Q, z["L5_p5_N5_J1_U2.5/dims"], z["L5_p5_N5_J1_U2.5/data"])
    tgt = MPS(L, p, Q, z["L5_p5_N5_J1_U50/dims"], z["L5_p5_N5_J1_U50/data"])
    eng = Engine(L, p, Q, J, dt, cut, maxm)
    eng.set_states(tgt, ini)
    u = np.linspace(2.5, 50.0, Nt)
    eng.propagate(u, 1)
    res = {"config": "1: L=5 p=5 Q=5 chi<=80 N_t=201, LDS engine (no k_gemm: kind 7 is 0), all t",
           "sector_max": int(max(eng.state(0, t).dims.max() for t in (0, Nt // 2, Nt - 1)))}
    res.update(energy_cases(eng, Nt, reps, 2, True))
    mom = eng.moments(0)
    res["energy_first_last"] = [float(native.energy(mom[0], J, u[0])), float(native.energy(mom[-1], J, u[-1]))]
    res["variance_first_last"] = [float(native.energy_variance(mom[0], J, u[0])),
                                  float(native.energy_variance(mom[-1], J, u[-1]))]
    return res


def energy4(reps):
    L, p, Q, J, dt, cut, maxm, Nt = 20, 7, 20, 1.0, 0.005, 1e-8, 256, 33
    z = np.load(os.path.join(GOLDEN, "c4_warm256.npz"), allow_pickle=False)
    c4 = np.load(os.path.join(GOLDEN, "c4.npz"), allow_pickle=False)
    u = np.load(os.path.join(GOLDEN, "c4_w256h33.npz"), allow_pickle=False)["u"]
    eng = Engine(L, p, Q, J, dt, cut, maxm, engine="hbm")
    eng.set_states(MPS(L, p, Q, c4["w256h/tgt_dims"], c4["w256h/tgt_data"]), MPS(L, p, Q, z["dims"], z["data"]))
    eng.propagate(u, 1)
    res = {"config": "4 slice: L=20 p=7 Q=20 chi=256 (warm state) N_t=33, HBM engine (task-list path)",
           "sector_max": int(max(eng.state(0, t).dims.max() for t in (0, Nt // 2, Nt - 1)))}
    res.update(energy_cases(eng, Nt, reps, 1, False))
    k9 = res["moments_kind9"]
    res["per_state_ms"] = res["moments"]["median_ms"] / Nt
    res["kind9_tflops"] = 1e-9 * k9["alg_flops"] / k9["ms"] if k9["ms"] else None
    res["k_gemm_share_of_kind9_time"] = res["moments_kind7_ms"] / k9["ms"] if k9["ms"] else None
    mom = eng.moments(0)
    res["energy_first_last"] = [float(native.energy(mom[0], J, u[0])), float(native.energy(mom[-1], J, u[-1]))]
    res["variance_first_last"] = [float(native.energy_variance(mom[0], J, u[0])),
                                  float(native.energy_variance(mom[-1], J, u[-1]))]
    return res


def pairs1(reps):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pair_reference as P
    L, p, Q, J, dt, cut, maxm, Nt = 5, 5, 5, 1.0, 0.01, 1e-8, 80, 201
    z = np.load(os.path.join(GOLDEN, "states.npz"), allow_pickle=False)
    ini = MPS(L, p, Q, z["L5_p5_N5_J1_U2.5/dims"], z["L5_p5_N5_J1_U2.5/data"])
    tgt = MPS(L, p, Q, z["L5_p5_N5_J1_U50/dims"], z["L5_p5_N5_J1_U50/data"])
    eng = Engine(L, p, Q, J, dt, cut, maxm)
    eng.set_states(tgt, ini)
    eng.propagate(np.linspace(2.5, 50.0, Nt), 3)

    def forced_lists():
        os.environ["OCG_OBS_PAIR_CHAIN"] = "0"
        try:
            return eng.observe_pairs(1, None, 0, None)
        finally:
            del os.environ["OCG_OBS_PAIR_CHAIN"]

    def host_route():
        out = []
        for t in range(Nt):
            x, y = eng.state(1, t), eng.state(0, t)
            out.append(P.pairs_ref(x.dims, x.data, y.dims, y.data, L, p, Q))
        return out
    cases = {"pairs": lambda: eng.observe_pairs(1, None, 0, None), "pairs_lists": forced_lists}
    for f in cases.values():
        f()
        f()
    t = {k: [] for k in cases}
    for _ in range(reps):
        for k, f in cases.items():
            t[k].append(timed(f))
    res = {"config": "1: L=5 p=5 Q=5 chi<=80 N_t=201, LDS engine, all (xi_t, psi_t)",
           "sector_max": int(max(eng.state(w, t).dims.max() for w in (0, 1) for t in (0, Nt // 2, Nt - 1)))}
    res.update({k: spread(v) for k, v in t.items()})
    host_route()
    res["host_get_state_plus_numpy"] = spread([timed(host_route) for _ in range(max(2, reps // 8))])
    for k in cases:
        eng.reset_stats()
        cases[k]()
        res[k + "_kind9"] = eng.stats(9)
        res[k + "_vs_host"] = res["host_get_state_plus_numpy"]["median_ms"] / res[k]["median_ms"]
    res["chain_vs_lists"] = res["pairs_lists"]["median_ms"] / res["pairs"]["median_ms"]
    a, b, h = cases["pairs"](), forced_lists(), host_route()
    res["chain_lists_max_dev"] = float(max(np.abs(a[k] - b[k]).max() for k in a))
    res["chain_host_max_dev"] = float(max(np.abs(a[k] - np.array([r[k] for r in h])).max() for k in a))
    return res


def strings1(reps):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import string_reference as T
    L, p, Q, J, dt, cut, maxm, Nt = 5, 5, 5, 1.0, 0.01, 1e-8, 80, 201
    z = np.load(os.path.join(GOLDEN, "states.npz"), allow_pickle=False)
    ini = MPS(L, p, Q, z["L5_p5_N5_J1_U2.5/dims"], z["L5_p5_N5_J1_U2.5/data"])
    tgt = MPS(L, p, Q, z["L5_p5_N5_J1_U50/dims"], z["L5_p5_N5_J1_U50/data"])
    eng = Engine(L, p, Q, J, dt, cut, maxm)
    eng.set_states(tgt, ini)
    eng.propagate(np.linspace(2.5, 50.0, Nt), 1)
    sets = {"parity": T.parity_tables(L, p, 1, 1), "counting": T.counting_tables(L, p, Q, 2, 4)}
    res = {"config": "1: L=5 p=5 Q=5 chi<=80 N_t=201, LDS engine, every psi_t",
           "sector_max": int(max(eng.state(0, t).dims.max() for t in (0, Nt // 2, Nt - 1))),
           "operators": {k: len(f) for k, f in sets.items()}}
    norm2 = eng.observe(0, None, outputs=("norm2",))["norm2"]
    for name, f in sets.items():
        def forced_lists():
            os.environ["OCG_OBS_STRING_CHAIN"] = "0"
            try:
                return eng.observe_strings(0, None, f)
            finally:
                del os.environ["OCG_OBS_STRING_CHAIN"]

        def host_route():
            out = []
            for t in range(Nt):
                x = eng.state(0, t)
                out.append(T.strings_ref(x.dims, x.data, L, p, Q, f))
            return np.array(out)
        cases = {"chain": lambda: eng.observe_strings(0, None, f), "lists": forced_lists}
        for c in cases.values():
            c()
            c()
        host_route()
        t = {k: [] for k in cases}
        t["host_get_state_plus_numpy"] = []
        for i in range(reps):  # alternating; the host route joins every eighth round
            for k, c in cases.items():
                t[k].append(timed(c))
            if i % 8 == 0:
                t["host_get_state_plus_numpy"].append(timed(host_route))
        r = {k: spread(v) for k, v in t.items()}
        # each device route on its own as well: a call's host-side cost can surface in the call after it
        for k, c in cases.items():
            r[k + "_back_to_back"] = spread([timed(c) for _ in range(max(8, reps // 2))][2:])
        for k in cases:
            eng.reset_stats()
            cases[k]()
            r[k + "_kind9"] = eng.stats(9)
            r[k + "_vs_host"] = r["host_get_state_plus_numpy"]["median_ms"] / r[k]["median_ms"]
        r["chain_vs_lists"] = r["lists"]["median_ms"] / r["chain"]["median_ms"]
        a, b, h = cases["chain"](), forced_lists(), host_route()
        sc = T.scale(norm2[:, None], f[None])
        r["chain_lists_max_dev_per_state"] = float((np.abs(a - b) / sc).max())
        r["chain_host_max_dev_per_state"] = float((np.abs(a - h) / sc).max())
        res[name] = r
    par = eng.parity_order(0, [0, Nt - 1], 1, 1)
    res["parity_order_first_last"] = [par[0].tolist(), par[1].tolist()]
    res["counting_2_4_last"] = eng.counting_statistics(0, [Nt - 1], 2, 4)[0].tolist()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="all", choices=["1", "4", "s1", "s4", "p1", "p4", "e1", "e4", "pairs", "strings",
                                                       "all"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name, fn, reps in (("1", config1, a.reps), ("4", config4, max(3, a.reps // 4)),
                           ("s1", spectrum1, a.reps), ("s4", spectrum4, max(3, a.reps // 4)),
                           ("p1", sample1, a.reps), ("p4", sample4, max(3, a.reps // 4)),
                           ("e1", energy1, a.reps), ("e4", energy4, max(3, a.reps // 4)),
                           ("pairs", pairs1, a.reps), ("strings", strings1, a.reps)):
        if a.config in (name, "all"):
            res = fn(reps)
            res["command"] = f"python -m optimalcontrolmps_amd.tools.observe_timing --config {name} --reps {a.reps}"
            kind = {"s": "observe_spectrum_config", "p": "observe_sample_config",
                    "e": "observe_energy_config"}.get(name[0], "observe_config")
            out = f"observe_{name}_config1.json" if name in ("pairs", "strings") else f"{kind}{name[-1]}.json"
            with open(os.path.join(a.out, out), "w") as f:
                json.dump(res, f, indent=1)
            print(json.dumps(res))


if __name__ == "__main__":
    main()
