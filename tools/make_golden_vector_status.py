#!/usr/bin/env python3
"""Writes tests/golden/vector_api_status.json: what a library answers to the degenerate calls of the vector and matrix
families (tests/vector_status.py lists them; tests/test_gpu_vector_status.py replays them on the built library).

The fixture pins a contract across a change of the entry points, so it is recorded from the library of the commit
BEFORE that change, never from the tree it is committed with.  Needs a GPU.

    python tools/make_golden_vector_status.py [--rev REV]
        exports REV (default HEAD) with git archive into a temporary directory, builds its library there and records
        it in a child process that loads it through CMSISDSP_MI355X_LIB
    python tools/make_golden_vector_status.py --lib PATH --commit ID
        records a library of that commit that was built beforehand (building and recording apart)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "vector_api_status.json")


def record(commit, out):
    sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import cmsisdsp_amd as dsp
    import vector_status as vs

    assert torch.cuda.is_available(), "needs a GPU"
    assert os.path.samefile(dsp.LIB_PATH, os.environ["CMSISDSP_MI355X_LIB"])
    rows = vs.replay(dsp, torch)
    doc = {"commit": commit, "library": dsp.version(), "functions": vs.function_names(dsp), "rows": rows}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rows)} functions, {sum(len(r) for r in rows.values())} rows, from {commit} ({doc['library']})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--lib")
    ap.add_argument("--commit")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if os.environ.get("CMSISDSP_MI355X_LIB") and a.commit and not a.lib:   # the child process
        return record(a.commit, a.out)
    with tempfile.TemporaryDirectory() as tmp:
        if a.lib:
            assert a.commit, "--lib needs --commit: the fixture names the commit it was recorded from"
            lib, commit = os.path.abspath(a.lib), a.commit
        else:
            commit = subprocess.run(["git", "rev-parse", a.rev], cwd=ROOT, check=True, capture_output=True,
                                    text=True).stdout.strip()
            tar = subprocess.run(["git", "archive", commit], cwd=ROOT, check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
            subprocess.run(["make", "-C", os.path.join(tmp, "cmsis-dsp_amd"), "-j", str(min(16, os.cpu_count() or 1))],
                           check=True, stdout=subprocess.DEVNULL)
            lib = os.path.join(tmp, "cmsis-dsp_amd", "lib", "libcmsisdsp_mi355x.so")
        env = dict(os.environ, CMSISDSP_MI355X_LIB=lib)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--commit", commit, "--out", a.out], env=env,
                       check=True)


if __name__ == "__main__":
    main()
