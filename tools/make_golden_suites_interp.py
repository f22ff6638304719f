#!/usr/bin/env python3
"""Writes tests/golden/suites_interp.npz and tests/golden/suites_interp_manifest.json (development machine only).

The replay of the reference's InterpolationTests{F32,Q31,Q15,Q7} and QuaternionTestsF32 (tests/suite_replay_interp.py)
needs the suites' pattern files and, per `Test` line, the words the reference's own scalar build gives.  This script
reads Testing/desc.txt and the pattern files the five suites name, compiles the reference's interpolation and
quaternion sources as tools/make_golden_interp.py and tools/make_golden_quaternion.py do (oracle/ref.mk's flags, a
temporary directory outside the tree), replays every line against that build, asserts that the reference passes its own
suite, and records the patterns and the output words.  Nothing compiled and no reference text is kept.

  <SuiteClass>/<pattern file stem>      the pattern's words, typed by the file's suffix
  <line id>/ref_<output>                what the reference build wrote (output; the spline lines also splineCoefs, buffer)
  manifest: one entry per `Test` line: suite, index, method, label, function, disabled, status ("replayed")

    python tools/make_golden_suites_interp.py [--ref DIR]
"""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd", "cmsisdsp_amd"))
import _abi  # noqa: E402  (the ctypes mirrors only; the product library is not loaded)
import make_golden_interp  # noqa: E402
import make_golden_quaternion  # noqa: E402
import make_golden_suites as mgs  # noqa: E402
import suite_replay as sr  # noqa: E402
import suite_replay_interp as sri  # noqa: E402


class Both:
    """The two reference builds as one ctypes library."""

    def __init__(self, *libs):
        self.libs = libs

    def __getattr__(self, name):
        for lib in self.libs:
            try:
                return getattr(lib, name)
            except AttributeError:
                pass
        raise AttributeError(name)


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    args = ap.parse_args()
    desc = mgs.parse_desc(os.path.join(args.ref, "Testing", "desc.txt"))
    data, entries = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        lib = sri.Ctypes(Both(make_golden_interp.build(args.ref, tmp)[0], make_golden_quaternion.build(args.ref, tmp)), _abi)
        for suite in sri.SUITES:
            s = desc[suite]
            folder = os.path.join(args.ref, "Testing", "Patterns", s["folder"])
            used = set()
            for stem, fname in s["patterns"].items():
                suffix = stem.rsplit("_", 1)[1]
                words = mgs.read_pattern(os.path.join(folder, fname))
                data[f"{suite}/{stem}"] = words.view(sr.DT[sr.SUFFIX[suffix]])
            pats = {k.split("/")[1].rsplit("_", 1)[0]: v for k, v in data.items() if k.startswith(suite + "/")}
            for index, t in enumerate(s["tests"], 1):
                e = {"suite": suite, "index": index, "method": t["method"], "label": t["label"],
                     "function": t["function"], "disabled": t["disabled"], "status": "replayed"}
                assert not t["disabled"], e
                seen = Recording(pats)
                outs, fails = sri.run_line(lib, e, seen)
                assert not fails, (sri.line_id(e), fails)
                used |= seen.used
                for name, o in outs.items():
                    data[f"{sri.line_id(e)}/ref_{name}"] = o.words.copy()
                entries.append(e)
            for key in [k for k in data if k.startswith(suite + "/") and k.count("/") == 1]:
                if key.split("/")[1].rsplit("_", 1)[0] not in used:      # a pattern no replayed line loads
                    del data[key]
    with open(sri.MANIFEST, "w") as f:
        json.dump(entries, f, indent=1)
        f.write("\n")
    np.savez_compressed(sri.FIXTURE, **data)
    print("wrote", len(entries), "lines,", os.path.getsize(sri.FIXTURE), "bytes")


class Recording(dict):
    """The suite's patterns, remembering which ones a line loads."""

    def __init__(self, pats):
        super().__init__(pats)
        self.used = set()

    def __getitem__(self, k):
        self.used.add(k)
        return super().__getitem__(k)


if __name__ == "__main__":
    main()
