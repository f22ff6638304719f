#!/usr/bin/env python3
"""Writes tests/golden/suites_<family>.npz and tests/golden/suites_manifest.json (development machine only).

The reference ships its own acceptance test: Testing/desc.txt names, per suite, the pattern files and the `Test` lines;
Testing/Patterns/DSP/** holds the inputs and the expected outputs its generators computed in double precision.  This
script extracts the data that the rows of tests/suite_replay.py read, and nothing else:

  suites_<family>.npz     <SuiteClass>/<pattern file stem>: the words of every pattern a replayed row loads, typed by
                          the file's suffix (format: Testing/PatternGeneration/Tools.py:775-790);
                          <SuiteClass>/<NN>_<method>/<label>/ref_words: what the reference build wrote for that row
  suites_manifest.json    one entry per `Test` line of the suites in scope: suite, index (the line's position, which
                          is the test's id), method, function, label (the line's nb= / parameter text), and status:
                          "replayed", or "skipped: <reason>" where the library exports no such function

It compiles the reference's scalar sources of the functions the rows call into a temporary directory outside the tree,
with oracle/ref.mk's own CFLAGS (the filter, convolution, transform and MFCC rows, suite_replay.REF_MK_FAMILIES, run
against oracle/ref.mk's own build instead, oracle/_ref/, which has their tables), replays every row against that
build through suite_replay.run_row and stops at the first row that misses one of the suite's checks: such a row is a
finding about ref.mk's flags or about the row.  The one exception: a threshold that the reference misses itself on an
inverse fixed-point transform is written into the manifest entry as `reference_fails` (check, output,
bound, measured) and not applied to that row, unless it is every check of the row; the row's words are recorded all
the same.  The MFCC rows read the data already committed in tests/golden/mfcc_<t>.npz, which is held to the suites'
pattern files here, and MFCC f32 words are recorded only where the host's logf is the one the device restates
(oracle/_build/liblogfprobe.so).  Nothing compiled and no reference text is kept in the tree's committed files.  The archives are written with fixed timestamps, so a second run gives
the same bytes.

    python tools/make_golden_suites.py [--ref DIR] [--docs]     (DIR: the reference tree, default as oracle/ref.mk)

It prints the sentence with the counts that README.md and DESIGN.md quote (tests/test_suites.py holds them to it);
with --docs it also rewrites that sentence in those two files, and touches nothing else in them.
"""
import argparse
import ctypes as C
import glob
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd", "cmsisdsp_amd"))
import _abi  # noqa: E402  (the ctypes mirrors only; the product library is not loaded)
import suite_replay as sr  # noqa: E402

MAX_BYTES = 1485055                                          # tests/golden/ref_vectors.npz, the largest fixture so far
KIND = {"W": 4, "H": 2, "B": 1, "D": 8}
# what the functions in scope call in turn (arm_rms_q31 / arm_std_q15 ...: the fixed-point square roots and their table)
NEEDED = ("FastMathFunctions/arm_sqrt_q31.c", "FastMathFunctions/arm_sqrt_q15.c", "CommonTables/arm_common_tables.c",
          "DistanceFunctions/arm_boolean_distance.c",      # the boolean distances' shared bit counts
          *(f"SupportFunctions/arm_{a}_sort_f32.c"          # what arm_sort_f32 dispatches to
            for a in ("bitonic", "bubble", "heap", "insertion", "quick", "selection")))

# the two functions whose source file carries another name
FILE_OF = {"arm_biquad_cas_df1_32x64_q31": "arm_biquad_cascade_df1_32x64_q31",
           "arm_biquad_cas_df1_32x64_init_q31": "arm_biquad_cascade_df1_32x64_init_q31"}


def read_pattern(path):
    """Line 1: the word width (W 32, H 16, B 8, D 64 bits); line 2: the count; then a `// value` comment and a hex word
    per sample -> the words as unsigned integers of that width."""
    with open(path) as f:
        lines = [l.strip() for l in f if l.strip()]
    size, count = KIND[lines[0]], int(lines[1])
    words = [int(l, 16) for l in lines[2:] if not l.startswith("//")]
    assert len(words) == count, (path, len(words), count)
    return np.array(words, dtype=np.uint64).astype(f"u{size}")


def parse_desc(path):
    """desc.txt -> {suite class: {"folder": path under Patterns, "patterns": {stem: file}, "tests": [entry]}}; an
    entry is {"label", "function", "method", "disabled"}.  A `Test` line reads `Test <label> [<function>]:<method>`."""
    suites, stack, depth, cur = {}, [], 0, None
    for raw in open(path):
        line = raw.split("//")[0].strip()
        m = re.match(r"(group|suite)\b", line)
        if m:
            stack.append({"kind": m.group(1), "folder": None, "depth": depth})
        m = re.match(r"class\s*=\s*(\w+)", line)
        if m and stack and stack[-1]["kind"] == "suite":
            cur = suites[m.group(1)] = {"patterns": {}, "tests": [], "folder": None}
        m = re.match(r"folder\s*=\s*(\w+)", line)
        if m:
            stack[-1]["folder"] = m.group(1)
            if stack[-1]["kind"] == "suite":
                cur["folder"] = os.path.join(*[s["folder"] for s in stack if s["folder"]])
        m = re.match(r"Pattern\s+\w+\s*:\s*(\S+)\.txt", line)
        if m and cur is not None:
            cur["patterns"][m.group(1)] = m.group(1) + ".txt"
        inside = any(k["kind"] == "functions" for k in stack)
        if re.match(r"Functions\b", line):
            stack.append({"kind": "functions", "folder": None, "depth": depth})
        for dis, body in re.findall(r"(disabled\s*\{)?\s*((?:Test\s+)?[^{}:]*:\s*\w+)", line) if inside else ():
            label, method = re.sub(r"^Test\s+", "", body).rsplit(":", 1)
            fm = re.search(r"\barm_\w+\s*$", label)
            cur["tests"].append({"label": (label[:fm.start()] if fm else label).strip(),
                                 "function": fm.group(0).strip() if fm else None, "method": method.strip(),
                                 "disabled": bool(dis)})
        depth += line.count("{") - line.count("}")
        while stack and depth <= stack[-1]["depth"]:
            if stack.pop()["kind"] == "suite":
                cur = None
    return suites


def cflags():
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    body = re.search(r"^CFLAGS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ")
    return [f for f in body.split() if not f.startswith("-I")]


def build(ref, out, funcs):
    """The reference's own scalar sources of funcs, with ref.mk's flags -> a ctypes library with _abi's signatures."""
    files = []
    for f in sorted(funcs):
        hit = glob.glob(os.path.join(ref, "Source", "*Functions", FILE_OF.get(f, f) + ".c"))
        assert len(hit) == 1, (f, hit)
        files.append(hit[0])
    files += [os.path.join(ref, "Source", f) for f in NEEDED]
    so = os.path.join(out, "libsuites_ref.so")
    inc = ["-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude")]
    subprocess.run(["gcc", *cflags(), "-shared", *inc, *files, "-o", so, "-lm"], check=True)
    lib = C.CDLL(so)
    sigs = {}
    for v in vars(_abi).values():
        if isinstance(v, dict):
            sigs.update({k: s for k, s in v.items() if isinstance(k, str) and k in funcs and isinstance(s, tuple)})
    for f in funcs:
        fn = getattr(lib, f)
        fn.restype, fn.argtypes = sigs[f]
    return sr.CtypesLibrary(lib, _abi)


def build_ref_mk(ref):
    """oracle/ref.mk's own build of the reference (oracle/_ref/libcmsisdsp_ref.so: the transforms, filters and MFCC
    compiled whole, tables included) -> a ctypes library with _abi's signatures."""
    subprocess.run(["make", "-s", "-f", "oracle/ref.mk", f"REF={ref}"], cwd=ROOT, check=True)
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libcmsisdsp_ref.so"))
    for table in (_abi.DROPIN, _abi.PARTIAL_FAST):
        for name, (restype, argtypes) in table.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
    return sr.CtypesLibrary(lib, _abi)


def assert_host_logf_is_the_restated_one():
    """arm_mfcc_f32's words depend on the generating host's logf (arm_vlog_f32.c:110): record them only where it is
    the one the device restates (oracle/src/logf_probe.cpp, built by `make -C oracle`)."""
    subprocess.run(["make", "-s", "-C", "oracle"], cwd=ROOT, check=True)
    probe = C.CDLL(os.path.join(ROOT, "oracle", "_build", "liblogfprobe.so"))
    probe.logf_probe_mismatches.restype = C.c_uint64
    probe.logf_probe_mismatches.argtypes = [C.c_uint32, C.c_uint32]
    bad = int(probe.logf_probe_mismatches(4099, 17))
    assert bad == 0, f"the host's logf differs from the device restatement on {bad} sampled inputs: do not record MFCC f32"


def inverse_fixed_point_transform(row):
    """The rows that may carry a reference_fails entry: arm_cfft_q31 / _q15 and arm_rfft_q31 / _q15 with ifft = 1."""
    return row.func in ("arm_cfft_q31", "arm_cfft_q15", "arm_rfft_q31", "arm_rfft_q15") and row.params.get("ifft") == 1


def save_npz(path, data):
    """np.savez_compressed with fixed member timestamps and order: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(data):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(data[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())


def main():
    ap = argparse.ArgumentParser()
    mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()
    ap.add_argument("--ref", default=re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    ap.add_argument("--docs", action="store_true", help="rewrite the quoted counts in README.md and DESIGN.md")
    args = ap.parse_args()
    desc = parse_desc(os.path.join(args.ref, "Testing", "desc.txt"))
    names = sr.exported_names(_abi)
    entries, by_family, patterns = [], {}, {}
    rows = {(r.suite, r.index): r for r in sr.ROWS}
    for suite, family in sr.FAMILIES.items():
        d = desc[suite]
        index = 0
        for t in d["tests"]:
            index += 1                                       # a disabled line keeps its id (Testing/preprocess.py)
            row = rows.get((suite, index))
            e = {"suite": suite, "index": index, "method": t["method"], "function": t["function"], "label": t["label"]}
            func = t["function"] or (row.func if row else sr.CALLS.get((suite, t["method"])))
            if row is not None:
                assert (row.method, row.label) == (t["method"], t["label"]), (suite, index, t, row.method, row.label)
                assert not t["disabled"], (suite, index, "the table replays a line the reference disables")
                # desc.txt may name the function without its type (arm_biquad_cascade_df1)
                # or under a name of its own (arm_biquad_cascade_df1_32x64 for arm_biquad_cas_df1_32x64_q31)
                if t["function"] not in (None, row.func):
                    e["named"] = t["function"]
                assert row.func in names, (row.func, "is not exported")
                e["function"] = row.func
                e["samples"] = None
                e["status"] = "replayed"
            elif t["disabled"]:
                e["function"] = func
                e["status"] = "skipped: disabled in the reference's own test description"
            else:
                assert func is not None and func not in names, (suite, index, t, "exported but no row replays it")
                e["function"] = func
                e["status"] = "skipped: the library exports no such function"
            entries.append(e)
        for r in sr.ROWS:
            if r.suite == suite and family != "mfcc":
                for stem, _ in r.load.values():
                    words = read_pattern(os.path.join(args.ref, "Testing", "Patterns", d["folder"],
                                                      d["patterns"][stem]))
                    t = sr.SUFFIX[stem.rsplit("_", 1)[1]]
                    assert words.itemsize == np.dtype(sr.DT[t]).itemsize, (suite, stem)
                    patterns[f"{suite}/{stem}"] = words.view(sr.DT[t])
    # the MFCC rows read the data already committed in tests/golden/mfcc_<t>.npz: held to the suites' pattern files here
    committed = sr.mfcc_data()
    for suite, t in sr.MFCC_T.items():
        d = desc[suite]
        for kind in ("Noise", "Sine"):
            for n in (256, 512, 1024):
                for ours, theirs in ((f"input_{kind}_{n}", f"MFCC{kind}Input_{n}_1_{t}"), (f"ref_{kind}_{n}", f"MFCC{kind}Ref_{n}_1_{t}")):
                    words = read_pattern(os.path.join(args.ref, "Testing", "Patterns", d["folder"], d["patterns"][theirs]))
                    have = committed[f"{suite}/{ours}"]
                    assert words.view(have.dtype)[:have.size].tobytes() == have.tobytes(), (suite, ours)
    mfcc_keys = set(committed)
    patterns.update(committed)
    own = [r for r in sr.ROWS if sr.FAMILIES[r.suite] not in sr.REF_MK_FAMILIES]
    whole = build_ref_mk(args.ref)
    assert_host_logf_is_the_restated_one()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(args.ref, tmp, {r.func for r in own} | {r.params["init"] for r in own if "init" in r.params} |
                    {f for r in own for f in r.params.get("needs", ())})
        for r in sr.ROWS:
            outs, failed = sr.run_row(r, whole if sr.FAMILIES[r.suite] in sr.REF_MK_FAMILIES else lib, patterns, exempt=())
            e = next(e for e in entries if (e["suite"], e["index"]) == (r.suite, r.index))
            if failed:
                # the reference misses its own thresholds on some inverse fixed-point transforms: such
                # a check is recorded with what it measured and not applied to that row; anything else is a finding
                checks = {(c[0], c[1]): c for c in r.checks}
                missed = [f for f in failed if len(f) == 3 and (f[0], f[1]) in checks and f[2] == checks[f[0], f[1]][3]]
                if len(missed) != len(failed) or not inverse_fixed_point_transform(r) or len(missed) == len(r.checks):
                    sys.exit(f"the reference build misses {failed} of {r.id} ({r.cite})")
                bufs = sr.load(r, patterns)
                e["reference_fails"] = []
                for form, name, thr in missed:
                    ref = checks[form, name][2]
                    want = outs[ref] if ref in outs else sr.reference(r, bufs, ref)
                    e["reference_fails"].append({"check": form, "output": name, "bound": thr,
                                                 "measured": sr.measure(form, outs[name], want)})
            for name, words in outs.items():
                if name not in sr.SCRATCH:
                    patterns[sr.ref_key(r, name)] = words
            e["samples"] = {k: int(v.size) for k, v in sr.load(r, patterns).items()}
    out = os.path.join(ROOT, "tests", "golden")
    for key, v in patterns.items():
        if key not in mfcc_keys:
            by_family.setdefault(sr.FAMILIES[key.split("/")[0]], {})[key] = v
    for family, data in sorted(by_family.items()):
        path = os.path.join(out, f"suites_{family}.npz")
        save_npz(path, data)
        assert os.path.getsize(path) <= MAX_BYTES, (path, os.path.getsize(path))
        print(f"suites_{family}.npz: {len(data)} arrays, {os.path.getsize(path)} bytes")
    with open(os.path.join(out, "suites_manifest.json"), "w") as f:
        json.dump(entries, f, indent=1, sort_keys=True)
        f.write("\n")
    for suite in sr.FAMILIES:
        mine = [e for e in entries if e["suite"] == suite]
        rep = sum(e["status"] == "replayed" for e in mine)
        print(f"{suite}: {rep} replayed, {len(mine) - rep} skipped")
    # README.md and DESIGN.md quote the counts: written from the manifest, never typed
    quoted = re.compile(r"\d+ test lines of \d+ suites: \d+ replayed, \d+ skipped(?: \([^)]*\))?"
                        r"(?:; \d+ checks of \d+ replayed lines exempted \([^)]*\))?")
    for doc in ("README.md", "DESIGN.md") if args.docs else ():
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert quoted.search(text), (doc, "does not quote the manifest")
        with open(os.path.join(ROOT, doc), "w") as f:
            f.write(quoted.sub(lambda m: sr.summary(), text))
    for e in entries:
        for f in e.get("reference_fails", ()):
            print(f"reference_fails: {e['suite']} {e['index']} {e['label']}: {f['check']} of {f['output']} "
                  f"measures {f['measured']} against {f['bound']}")
    print("the reference build passes every replayed line but for the checks above:", sr.summary())


if __name__ == "__main__":
    main()
