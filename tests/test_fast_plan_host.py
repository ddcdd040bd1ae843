"""The host plans of the one-wave padded chain (csrc/fast_plan.hpp: build_fast_plan, build_overlap_plan) under
a verifier built as a stand-alone program with AddressSanitizer + UndefinedBehaviorSanitizer
(tests/cpp/fast_plan_check.cpp): for every shape of L = 2..8, p = 2..7, Q = 1..8 every packed field decodes
back to a value recomputed from (L, p, Q), every offset lies inside its LDS region or is that region's zero
slot, factor destinations are distinct and cover whole padded sites, eigen slots are a permutation, tables
are 16-byte aligned and the LDS sizes cover the furthest byte a descriptor addresses.  The program's
accept / reject verdicts are those of tests/golden/fast_plan_census.json."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

with open(os.path.join(HERE, "golden", "fast_plan_census.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fast_plan_check") / "fast_plan_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(HERE, "cpp", "fast_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("OCG_FAST_DUMP", None)
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)


def test_plans_verify_under_asan_ubsan(run):
    bad = [m for m in ("ERROR: AddressSanitizer", "runtime error:") if m in run.stderr]
    violations = [ln for ln in run.stdout.splitlines() if ln.startswith("VIOLATION")]
    assert run.returncode == 0 and not bad and not violations, (run.returncode, violations[:20], run.stderr[-3000:])
    assert run.stdout.splitlines()[-1] == "307 shapes, 170 accepted, 0 violations"


def test_verdicts_equal_the_census(run):
    got = {}
    for ln in run.stdout.splitlines()[:-1]:
        L, p, Q, verdict, rest = ln.split(" ", 4)
        got[f"{L},{p},{Q}"] = (verdict == "accepted", "" if verdict == "accepted" else rest)
        if verdict == "accepted":
            f = rest.split()
            assert f[-1] == "ok" and int(f[f.index("np") + 1]) == GOLDEN[f"{L},{p},{Q}"]["np"] \
                and int(f[f.index("ops") + 1]) == GOLDEN[f"{L},{p},{Q}"]["nops"], ln
    assert got == {k: (v["accepted"], v["why_not"]) for k, v in GOLDEN.items()}
