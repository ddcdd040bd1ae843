"""The HBM engine's host drivers issue the batches they were recorded with:
every launch / step counter of Engine.stats(0..5, 7) and Engine.path_stats()
after each driver call on config 1's chain equals
tests/golden/hbm_driver_counts.json (tests/golden/make_hbm_driver_counts.py,
recorded on an MI355X).  The counters are exact integers: a batch split or
merged, or a step added or dropped, changes them.  Not compared: the GEMM
kernel's launch count of the pipelined getHessian (its dH thread joins the rows
that are ready when it looks, which depends on thread timing)."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "hbm_driver_counts.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def replayed(states):
    spec = importlib.util.spec_from_file_location("make_hbm_driver_counts",
                                                  os.path.join(HERE, "golden", "make_hbm_driver_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(states)


def test_same_cases(replayed):
    assert sorted(replayed) == sorted(GOLDEN)


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_driver_counts(replayed, case):
    got, want = replayed[case], GOLDEN[case]
    print(case, got)
    differ = {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}
    assert got == want, differ
