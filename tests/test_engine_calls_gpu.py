"""The C entry points one pass of the encoder engine (models/resnet.py::_Engine) calls, in order and with the stream each launch goes to,
against tests/golden/engine_entry_sequence.json — recorded from the resnet.py of the commit that file names by
tests/golden/make_goldens_engine_calls.py (which documents the cases).  The engine is host code around an unchanged library: the same
calls in the same order on the same streams is what "same behaviour" means for it."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_goldens_engine_calls", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_goldens_engine_calls.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_entry_sequence.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", mg.CASES)
def test_entry_point_sequence(gpu, golden, name):
    from video_similarity_search_amd.models import resnet
    assert len(golden["recorded_from_commit"]) == 40
    got = mg.run_case(resnet, name)
    assert got == golden["sequences"][name]
