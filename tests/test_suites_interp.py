"""tests/suite_replay_interp.py on the CPU: the manifest names every `Test` line of the five suites once, the fixture
holds every pattern a line loads and the reference build's words, and the numpy restatements, replayed line by line,
pass the suites' own thresholds and give the reference build's words.  The GPU replay is tests/test_gpu_suites_interp.py."""
import os

import numpy as np
import pytest

import suite_replay as sr
import suite_replay_interp as sri
from f32_classes import assert_same_words

FIX = np.load(sri.FIXTURE)
LINES = sri.manifest()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_line(lib, e):
    """Replays e against lib: no ASSERT_* line fails and every output equals the reference build's words."""
    outs, fails = sri.run_line(lib, e, sri.patterns(FIX, e["suite"]))
    assert not fails, (sri.line_id(e), fails)
    for name, o in outs.items():
        want = FIX[f"{sri.line_id(e)}/ref_{name}"]
        if want.dtype == np.float32:
            assert_same_words(o.words, want, f"{sri.line_id(e)} {name}")
        else:
            assert np.array_equal(o.words, want), (sri.line_id(e), name)
    return outs


def test_manifest_is_complete():
    assert len(LINES) == 19 and " 19 lines" in " ".join(sri.SUMMARY.split())
    assert {e["suite"] for e in LINES} == set(sri.SUITES) and all(e["status"] == "replayed" for e in LINES)
    assert len({sri.line_id(e) for e in LINES}) == len(LINES) and not any(e["disabled"] for e in LINES)
    per = {s: [e for e in LINES if e["suite"] == s] for s in sri.SUITES}
    assert [len(per[s]) for s in sri.SUITES] == [5, 2, 2, 2, 8]
    for s, lines in per.items():
        assert [e["index"] for e in lines] == list(range(1, len(lines) + 1)), s
    methods = {e["method"] for e in LINES}
    assert set(sri.QUATERNION) | set(sri.SPLINES) <= methods
    assert not (set(sri.SUITES) & set(sr.FAMILIES))          # the first replay's table is not extended
    assert os.path.getsize(sri.FIXTURE) < 128 << 10
    text = open(os.path.join(ROOT, "README.md")).read()
    assert " ".join(sri.SUMMARY.split()) in " ".join(text.split())


@pytest.mark.parametrize("e", LINES, ids=sri.line_id)
def test_restatement_passes_every_line(e):
    check_line(sri.Restatement(), e)
