"""The reference's own suites (tests/suite_replay.py) replayed against the numpy restatements, on the CPU.

Every row must pass the suite's thresholds against the double-precision patterns and give the words the reference build
gave (tests/golden/suites_*.npz, <row>/ref_words; the README states these families bit-exact).  The negative controls
plant, in a passing output, a defect just outside each check of each row and a written tail word, and want the row to
fail on that check; they disturb a word behind a FIR call's block, and plant four kernel defects (a dropped state
carry, a late decimator phase, an ignored firstIndex, an inverse RFFT one halving short) that must turn exactly the
rows red that meet them; the manifest tests hold tests/golden/suites_manifest.json against the table and against what the
library exports."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import mfcc_cfg
import suite_replay as sr
from suite_replay import patterns, same_words


@pytest.mark.parametrize("suite,method", sr.methods(), ids=lambda v: v)
def test_restatements_pass_the_suites(suite, method):
    lib = sr.RestatementLibrary()
    # the restatement of arm_mfcc_f32 calls the host's logf as the reference does: its words are the recorded ones
    # where that logf is the one of the generating host (tests/mfcc_cfg.py), the suite's thresholds hold anywhere
    same_libm = suite != "MFCCF32" or mfcc_cfg.host_libm_status()[0]
    for row in (r for r in sr.ROWS if (r.suite, r.method) == (suite, method)):
        pats = patterns(row)
        outs, failed = sr.run_row(row, lib, pats)
        assert not failed, (row.id, row.cite, failed)
        for name, words in outs.items():
            if row.exact and same_libm and name not in sr.SCRATCH:
                same_words(words, pats[sr.ref_key(row, name)], (row.id, name))


# ---------------------------------------------------------------------------------------------------------------------
# negative controls
def _limits(dtype):
    return (np.iinfo(dtype).min, np.iinfo(dtype).max) if dtype.kind in "iu" else (-np.inf, np.inf)


def _plant_snr(words, ref, thr):
    """An error of twice the amplitude the threshold allows (6 dB under it), on as few words as can carry it: each
    moves towards and past zero, the way that never leaves the type's range first."""
    scale = 1.0 if words.dtype.kind == "f" else 2.0 ** (8 * words.itemsize - 1)
    energy = float(np.sum((ref.astype(np.float64) / scale) ** 2))
    assert energy > 0
    lo, hi = _limits(words.dtype)
    order = np.argsort(-np.abs(ref.astype(np.float64)), kind="stable")
    for k in range(1, words.size + 1):
        d = 2.0 * math.sqrt(energy / k) * 10.0 ** (-thr / 20.0) * scale
        d = d if words.dtype.kind == "f" else math.ceil(d)
        idx = order[:k]
        new = np.where(ref[idx] > 0, ref[idx].astype(np.float64) - d, ref[idx].astype(np.float64) + d)
        if new.min() >= lo and new.max() <= hi:
            words[:] = ref
            words[idx] = new.astype(words.dtype)
            return
    raise AssertionError("no planted error fits the type")


def _off(ref, value):
    """value as float32, or the next float32 away from ref where the bound is finer than the format (1e-8)."""
    v = np.float32(value)
    return v if v != ref else np.nextafter(ref, np.float32(np.inf if value >= ref else -np.inf))


def _plant(form, words, ref, thr):
    """Writes the reference pattern with one defect just outside the bound of `form` into words."""
    ref = ref[:words.size] if form == "eq_partial" else ref
    words[:] = ref
    i = int(np.argmax(np.abs(ref.astype(np.float64))))
    lo, hi = _limits(words.dtype)
    if form == "near_eq":                                   # 2 x the absolute bound
        v = int(ref[i]) + 2 * thr
        words[i] = v if v <= hi else int(ref[i]) - 2 * thr
    elif form == "rel":                                     # 2 x the relative bound
        assert ref[i] != 0
        words[i] = _off(ref[i], np.float64(ref[i]) * (1.0 + 2.0 * thr))
    elif form == "eq" and words.size > 1 and (np.roll(ref, 1) != ref).any():         # one index off
        words[:] = np.roll(ref, 1)
    elif form in ("eq", "eq_s16"):                          # (or a constant output, as arm_fill_* gives)                          # a single word (a value, an index): the next one
        if words.dtype.kind == "f":
            words[0] = np.nextafter(ref[0], np.float32(np.inf))
        else:
            words[0] = int(ref[0]) + (1 if int(ref[0]) < hi else -1)
    elif form == "close":                                   # 2 x (abs + rel * |ref|)
        words[i] = np.float32(np.float64(ref[i]) + 2.0 * (thr[0] + thr[1] * abs(np.float64(ref[i]))))
    elif form == "eq_partial":                              # one index off, among the words the output holds
        words[:] = np.roll(ref[:words.size], 1)
        assert (words != ref[:words.size]).any()
    elif form == "near":                                    # 2 x the absolute bound, on float words
        words[i] = _off(ref[i], np.float64(ref[i]) + 2.0 * thr)
    elif form == "within":                                  # 2 x the bound
        words[0] = ref[0] + np.float32(2.0 * thr)
    elif form == "snr":
        _plant_snr(words, ref, thr)
    else:
        raise AssertionError(form)


@pytest.mark.parametrize("suite", list(sr.FAMILIES))
def test_rows_report_planted_defects(suite):
    """Every check of every row, and the tail of every row: the defect must be reported under its own name."""
    lib = sr.RestatementLibrary()
    forms = set()
    for row in (r for r in sr.ROWS if r.suite == suite):
        pats = patterns(row)
        for form, name, ref, thr in row.checks:
            def tamper(outs, form=form, name=name, ref=ref, thr=thr):
                want = outs[ref].words if ref in outs else sr.reference(row, sr.load(row, pats), ref)
                _plant(form, outs[name].words, want, thr)
            _, failed = sr.run_row(row, lib, pats, tamper)
            assert (form, name, thr) in failed, (row.id, form, thr, failed)
            forms.add(form)

        def tail(outs):
            o = outs["output"]
            o.buf[o.n + sr.TAIL - 1] = 0                    # the last tail word, as the framework fills it: zero
        _, failed = sr.run_row(row, lib, pats, tail)
        assert failed == [("tail", "output")], (row.id, failed)

        def first_tail(outs):
            o = outs["output"]
            o.buf[o.n] = o.words[-1]
        _, failed = sr.run_row(row, lib, pats, first_tail)
        assert ("tail", "output") in failed, (row.id, failed)
    assert forms == {c[0] for r in sr.ROWS if r.suite == suite for c in r.checks}


def test_a_changed_input_is_reported():
    row = next(r for r in sr.ROWS if r.suite == "BasicTestsF32")

    class Scribbler(sr.RestatementLibrary):
        def __getattr__(self, name):
            fn = super().__getattr__(name)

            def call(a, *rest):
                fn(a, *rest)
                a[0] = a[0] + a.dtype.type(1)
            return call
    _, failed = sr.run_row(row, Scribbler(), patterns(row))
    assert failed == [("input changed", "input1")]


def test_a_word_written_past_a_call_s_output_is_reported():
    """BIQUADQ31's 32x64 test filters one sample per call and looks behind every call's output (checkInnerTail)."""
    row = next(r for r in sr.ROWS if r.method == "test_biquad_cascade_df1_32x64")

    class Overrun(sr.RestatementLibrary):
        def __getattr__(self, name):
            fn = super().__getattr__(name)
            if name != row.func:
                return fn

            def call(S, src, dst, n):
                fn(S, src, dst, n)
                whole = dst.base
                whole[(dst.ctypes.data - whole.ctypes.data) // dst.itemsize + n] = dst[n - 1]
            return call
    _, failed = sr.run_row(row, Overrun(), patterns(row))
    assert ("inner tail", "output", 1) in failed and ("tail", "output") in failed, failed[:3]
    _, failed = sr.run_row(row, sr.RestatementLibrary(), patterns(row))
    assert not failed


def _with(wraps):
    """The restatements, with the functions named in wraps {name: fn -> defective fn} replaced."""
    class Defective(sr.RestatementLibrary):
        def __getattr__(self, name):
            fn = super().__getattr__(name)
            return wraps[name](fn) if name in wraps else fn
    return Defective()


def _red(lib, families):
    """The ids of the rows of these families that the library fails."""
    return {r.id for r in sr.ROWS if sr.FAMILIES[r.suite] in families and sr.run_row(r, lib, patterns(r))[1]}


@pytest.mark.parametrize("t", ["f32", "q31", "q15", "q7"])
def test_a_disturbed_fir_inner_tail_word_is_reported(t):
    """FIR*'s checkInnerTail: a word written behind a call's block is reported after that call, even where the next
    call overwrites it; only the word behind the last block also breaks the buffer's tail."""
    row = sr.BY_ID[f"FIR{t.upper()}/01_test_fir_{t}/-"]

    def overrun(fn):
        def call(S, src, dst, n):
            fn(S, src, dst, n)
            whole = dst.base
            whole[(dst.ctypes.data - whole.ctypes.data) // dst.itemsize + n] = 1
        return call
    _, failed = sr.run_row(row, _with({row.func: overrun}), patterns(row))
    first_block = int(patterns(row)[f"{row.suite}/FirConfigs1_s16"][0])
    assert ("inner tail", "output", first_block) in failed and ("tail", "output") in failed, failed[:3]
    assert len([f for f in failed if f[0] == "inner tail"]) == patterns(row)[f"{row.suite}/FirConfigs1_s16"].size
    assert not [f for f in failed if f[0] in ("snr", "near_eq", "rel")], failed   # every such word but the last is rewritten


def _fir_without_state_carry(fn):
    def call(S, src, dst, n):
        C.memset(C.cast(S.pState, C.c_void_p), 0, (S.numTaps + n - 1) * src.itemsize)     # as the init left it
        fn(S, src, dst, n)
    return call


def _decimator_one_phase_late(fn):
    def call(S, src, dst, n):
        late = np.concatenate([src[1:n], src[n - 1:n]])     # sample k + 1 where sample k belongs
        fn(S, late, dst, n)
    return call


def _partial_ignoring_first(fn):
    def call(a, la, b, lb, dst, first, num, *scratch):
        head = np.zeros(num, dtype=dst.dtype)
        status = fn(a, la, b, lb, head, 0, num, *scratch)   # outputs 0 ... num - 1, stored where first ... belong
        dst[first:first + num] = head
        return status
    return call


def _inverse_rfft_without_a_halving(fn):
    def call(S, src, dst):
        fn(S, src, dst)
        if S.ifftFlagR:
            dst[:S.fftLenReal] = (dst[:S.fftLenReal].astype(np.int64) << 1).astype(dst.dtype)
    return call


PLANTED = {
    # defect: (the functions it is planted in, the families replayed, the rows that must turn red)
    "the FIR state carry dropped between the two calls":
        ({f"arm_fir_{t}": _fir_without_state_carry for t in ("f32", "q31", "q15", "q7")}, ("fir",),
         lambda r: True),
    "the decimator's phase off by one":
        ({f"arm_fir_decimate_{t}": _decimator_one_phase_late for t in ("f32", "q31", "q15")}, ("decim",),
         lambda r: "decimate" in r.func),
    "first ignored in a partial convolution":
        ({r.func: _partial_ignoring_first for r in sr.ROWS if "first" in r.params}, ("misc",),
         lambda r: "first" in r.params),
    "the RFFT inverse scaling omitted":
        ({"arm_rfft_q31": _inverse_rfft_without_a_halving, "arm_rfft_q15": _inverse_rfft_without_a_halving},
         ("transform_r",), lambda r: r.func != "arm_rfft_fast_f32" and r.params["ifft"] == 1),
}


@pytest.mark.parametrize("defect", list(PLANTED))
def test_a_planted_kernel_defect_turns_its_rows_red(defect):
    """The defects a filter or transform kernel is likeliest to have: exactly the rows that call the defective function
    that way fail, every other row of the family stays green."""
    wraps, families, hit = PLANTED[defect]
    want = {r.id for r in sr.ROWS if sr.FAMILIES[r.suite] in families and hit(r)}
    assert want and _red(_with(wraps), families) == want


# ---------------------------------------------------------------------------------------------------------------------
# the manifest
def test_manifest_lines_are_replayed_or_skipped_for_want_of_the_function(dsp):
    from cmsisdsp_amd import _abi
    exported = sr.exported_names(_abi)
    lines = sr.manifest()
    assert len({(e["suite"], e["index"]) for e in lines}) == len(lines)
    assert {e["suite"] for e in lines} == set(sr.FAMILIES)
    disabled = {(f"Transform{c}{t.upper()}", i) for c, table in (("C", sr.CFFT_DISABLED), ("R", sr.RFFT_DISABLED))
                for t, indexes in table.items() for i in indexes}
    replayed = set()
    for e in lines:
        rid = sr.row_id(e["suite"], e["index"], e["method"], e["label"])
        if e["status"] == "replayed":
            row = sr.BY_ID[rid]                             # a row of the table replays it
            assert row.func == e["function"] and row.func in exported
            assert hasattr(dsp.lib, row.func), row.func
            replayed.add(rid)
        else:
            assert e["status"].startswith("skipped: ") and len(e["status"]) > len("skipped: "), e
            assert rid not in sr.BY_ID, rid
            assert e["function"] is not None, e
            if (e["suite"], e["index"]) in disabled:            # the table names the transform lines desc.txt disables
                assert e["status"] == "skipped: disabled in the reference's own test description", e
                disabled.remove((e["suite"], e["index"]))
                continue
            # a condition, not a judgement: no other skipped line names a function the library has
            assert e["function"] not in exported, e
            assert not hasattr(dsp.lib, e["function"]), e
    assert not disabled, disabled
    assert replayed == set(sr.BY_ID)                        # and the table has no row the manifest does not know


def test_exempted_checks_are_the_ones_the_generator_recorded():
    """A check the reference build misses itself is recorded in the manifest with what it measured (outside the
    bound), only on an inverse fixed-point transform, and never all the checks of a row; the recorded words stay."""
    recorded = {}
    for e in sr.manifest():
        if "reference_fails" in e:
            row = sr.BY_ID[sr.row_id(e["suite"], e["index"], e["method"], e["label"])]
            assert e["status"] == "replayed" and e["reference_fails"], e
            assert row.func in ("arm_cfft_q31", "arm_cfft_q15", "arm_rfft_q31", "arm_rfft_q15") and row.params["ifft"] == 1
            checks = {(c[0], c[1]): c[3] for c in row.checks}
            for f in e["reference_fails"]:
                assert checks[f["check"], f["output"]] == f["bound"], (row.id, f)
                assert f["measured"] < f["bound"] if f["check"] == "snr" else f["measured"] > f["bound"], (row.id, f)
            recorded[row.id] = {(f["check"], f["output"]) for f in e["reference_fails"]}
            assert len(recorded[row.id]) == len(e["reference_fails"]) < len(row.checks), row.id
            assert row.exact and sr.ref_key(row) in patterns(row), row.id
    assert sr.exemptions() == recorded


def test_documents_quote_the_manifest():
    root = os.path.dirname(sr.GOLDEN.rstrip("/").rsplit("/", 1)[0])
    for doc in ("README.md", "DESIGN.md"):
        with open(os.path.join(root, doc)) as f:
            assert sr.summary() in f.read(), (doc, "regenerate the counts: python tools/make_golden_suites.py")


def test_fixture_holds_what_the_rows_read_and_no_more():
    for family in set(sr.FAMILIES.values()):
        pats = sr.patterns_of(family)
        rows = [r for r in sr.ROWS if sr.FAMILIES[r.suite] == family]
        want = {f"{r.suite}/{stem}" for r in rows for stem, _ in r.load.values()}
        assert want <= set(pats) and all(sr.ref_key(r) in pats for r in rows)
        assert all(k in want or k.rsplit("/", 1)[0] in sr.BY_ID for k in pats)
        assert all(v.dtype.kind in "fiu" for v in pats.values())
