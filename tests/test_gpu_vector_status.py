"""The calling contract of the vector and matrix families on degenerate calls, against the answers recorded from the
library before these entry points were moved onto one call driver (tests/golden/vector_api_status.json, written by
tools/make_golden_vector_status.py; the rows: tests/vector_status.py)."""
import json
import os

import pytest

import vector_status as vs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vector_api_status.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_every_function(dsp, golden):
    """The fixture lists exactly the drop-ins and _batch forms that the *_ref.py lists and the library's exported
    symbols give now, and holds every row of each: a new function cannot be left out silently."""
    names = vs.function_names(dsp)
    assert golden["functions"] == names
    assert sorted(golden["rows"]) == names
    for model in vs.models(dsp).values():
        for form in model.forms:
            assert list(golden["rows"][form]) == sorted(r for r, _ in vs.rows(model, form)), form


@pytest.mark.gpu
def test_degenerate_calls_answer_as_recorded(dsp, torch_gpu, golden):
    """Status, whether the last error is set, and which buffers changed, row by row."""
    got = vs.replay(dsp, torch_gpu)
    bad = [(f, r, got[f][r], want) for f, rows in golden["rows"].items() for r, want in rows.items()
           if got[f][r] != want]
    assert not bad, f"{len(bad)} rows differ from {golden['commit'][:12]}; the first: {bad[:8]}"
    assert sum(len(r) for r in got.values()) == sum(len(r) for r in golden["rows"].values())
