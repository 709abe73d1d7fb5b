"""GPU: every user of LinearPlan — HipLinear, the InfoNCE head, the classifier head, the projection head — computes the bits, and calls
the multiset of library entry points, that the hand-written 1x1x1-convolution code of the commit before LinearPlan did
(tests/golden/linear_sites_parent.json, recorded on an MI355X by tests/golden/make_goldens_linear_sites.py, which also holds the cases).
Two runs of the generator on that commit gave the same record, so every entry is held bit for bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_goldens_linear_sites", os.path.join(HERE, "golden", "make_goldens_linear_sites.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def record(golden_dir):
    with open(os.path.join(golden_dir, "linear_sites_parent.json")) as f:
        rec = json.load(f)
    assert sorted(rec["cases"]) == sorted(gen.CASES)
    return rec["cases"]


@pytest.mark.parametrize("name", gen.CASES)
def test_linear_site_reproduces_the_parent_record(gpu, record, name):
    got, want = gen.run_case(name), record[name]
    assert sorted(got["outputs"]) == sorted(want["outputs"])
    for k, w in want["outputs"].items():
        assert got["outputs"][k] == w, (name, k, got["outputs"][k], w)
    assert got["calls"] == want["calls"], (name, {k: (got["calls"].get(k, 0), want["calls"].get(k, 0))
                                                  for k in set(got["calls"]) | set(want["calls"])
                                                  if got["calls"].get(k, 0) != want["calls"].get(k, 0)})
