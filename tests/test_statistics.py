"""arm_{mean,power,rms,var,std,mse}_*, arm_accumulate_f32, arm_{absmax,absmin}_*, arm_{max,min,absmax,absmin}_no_idx_*
(46 drop-ins and their _batch forms, cmsis-dsp_amd/csrc/statistics.hip), arm_sqrt_q15 and arm_cmplx_mag_fast_q15.

The checker is committed data: tests/golden/statistics.npz holds the reference's own outputs, each in a buffer
pre-filled with a marker word with a guard word either side (tools/make_golden_statistics.py);
tests/statistics_ref.py restates the functions in numpy and Python ints, and the generator asserted it against the
reference case by case.  Every comparison is bit-exact; f32 results follow the rule of tests/test_f32_classes.py
(non-NaN words bit-equal, NaNs at the same positions).

CPU: the fixture index, the restatement against every fixture, the probed facts, arm_sqrt_q15 on every int16
input, the exported symbols, the Python names.  GPU: every function through its _batch form and its drop-in against
every fixture; the shapes at which the kernels change path (the lanes-per-item steps 1 .. 64 lanes, the whole
workgroup past REDUCE_WAVE_MAX loads, 16-B packs or single elements, the two f32 chain kernels: one wave per item
below SUM_LANE_MIN_BATCH items, one lane per item with SUM_CHUNK-word LDS stages from there on, var / std keeping up
to VAR_KEEP words between their two passes); the f32 value classes on long items; the refusals."""
import json
import os

import numpy as np
import pytest

import statistics_ref as sr
from cmsisdsp_amd import _abi
from f32_classes import f32_class_input

cm = sr.cm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "statistics.npz"))
INDEX = [(f, list(c)) for f, c in json.loads(str(GOLD["index"]))]
CASES = dict(INDEX)
GUARD = 8                      # marker words after the end of every device buffer
SUCCESS, ARGUMENT_ERROR = 0, -1
# the constants of statistics.hip / reduce_lanes.hpp that decide a kernel's path
REDUCE_WAVE_MAX = 512          # kRedWaveMax: loads (16-B packs when aligned, else words) a wave takes per item
SUM_LANE_MIN_BATCH = 4096      # kSumLaneMinBatch
SUM_CHUNK = 16                 # kSumChunk
VAR_KEEP = 1024                # kVarKeep
SUMS = [f for f in sr.STAT_FUNCS if sr.split(f)[0] in sr.SUM_OPS]
SEARCHES = [f for f in sr.STAT_FUNCS if f not in SUMS]


def _type_name(a):
    return {np.dtype(v): k for k, v in sr.MDT.items()}[np.asarray(a).dtype]


def unguard(buf):
    """A fixture output buffer -> its words, after checking the guard word either side."""
    m = np.asarray(sr.MARK[_type_name(buf)]).tobytes()
    assert buf[:1].tobytes() == m and buf[-1:].tobytes() == m, "guard words"
    return buf[1:-1]


_OFFSETS = {}


def gold(func, case):
    """{"a", "b"} operands and {"value", "index"} results of one recorded case."""
    names = CASES[func]
    k = names.index(case)
    if sr.stored(case):
        if func not in _OFFSETS:
            per = 2 if func == "cmplx_mag_fast_q15" else 1
            sizes = [per * sr.case_n(c) if sr.stored(c) else 0 for c in names]
            _OFFSETS[func] = np.concatenate([[0], np.cumsum(sizes)])
        lo, hi = _OFFSETS[func][k], _OFFSETS[func][k + 1]
        g = {"a": GOLD[f"{func}/a"][lo:hi]}
        if sr.two_sources(func):
            g["b"] = GOLD[f"{func}/b"][lo:hi]
    else:
        g = sr.operands(func, case)
    assert sr.crc(g) == int(GOLD[f"{func}/crc"][k]), (func, case, "operands differ from the recorded ones")
    if func == "cmplx_mag_fast_q15":
        start = sum(sr.case_n(c) + 2 for c in names[:k])
        g["value"] = unguard(GOLD[f"{func}/dst"][start:start + sr.case_n(case) + 2])
        return g
    g["value"] = unguard(GOLD[f"{func}/value"][k]).reshape(())
    if sr.has_index(func):
        g["index"] = unguard(GOLD[f"{func}/index"][k]).reshape(())
    return g


def check(func, what, got, want):
    for k in ("value", "index"):
        if k in want:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert sr.same_words(g.reshape(w.shape), w, sr.nan_rule(func)), (func, what, k, g, w)


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    """46 statistics functions and arm_cmplx_mag_fast_q15; every case of the case list is inside the reference's
    contract and recorded, every length of the issue among them."""
    assert len(sr.STAT_FUNCS) == 46 and len(set(sr.FUNCS)) == 47
    assert [f for f, _ in INDEX] == list(sr.FUNCS)
    for f, cases in INDEX:
        assert cases == sr.case_names(f), f
        if f != "cmplx_mag_fast_q15":
            assert cases[:20] == [f"rand_{n}" for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 257, 1023,
                                                         1025, 4097, 33000)]
    for t in ("q15",):
        assert "wrap_65537" in CASES[f"var_{t}"] and "wrap_65537" in CASES[f"std_{t}"]


def test_contract_check_rejects_overflowing_items():
    """in_contract(), which decides what the generator records: the 32-bit sums of mean_q7 / q15, var / std_q15,
    power_q7, mse_q7 and sum * sum of var / std_q31."""
    assert sr.in_contract("mean_q15", np.full(65536, -32768, dtype=np.int16))
    assert not sr.in_contract("mean_q15", np.full(65537, -32768, dtype=np.int16))
    assert not sr.in_contract("var_q15", np.full(65537, -32768, dtype=np.int16))
    assert not sr.in_contract("power_q7", np.full(131072, -128, dtype=np.int8))
    assert sr.in_contract("power_q7", np.full(131071, -128, dtype=np.int8))
    assert not sr.in_contract("mse_q7", np.full(2 ** 18, -128, dtype=np.int8), np.full(2 ** 18, 127, dtype=np.int8))
    assert sr.in_contract("var_q31", np.full(256, -2 ** 31, dtype=np.int32))
    assert not sr.in_contract("std_q31", np.full(363, -2 ** 31, dtype=np.int32))
    for f in sr.STAT_FUNCS:
        for c in CASES[f]:
            if sr.case_n(c) <= 300:
                g = sr.operands(f, c)
                assert sr.in_contract(f, g["a"], g.get("b")), (f, c)


def test_restatement_equals_every_fixture():
    for f, cases in INDEX:
        for c in cases:
            g = gold(f, c)
            check(f, c, sr.run(f, g["a"], g.get("b")), g)


def test_probed_facts_hold_in_the_fixtures():
    """The traps the issue lists, read off the reference's own outputs."""
    u32 = lambda x: int(np.asarray(x, dtype=np.float32).reshape(1).view(np.uint32)[0])       # noqa: E731
    # arm_sqrt_f32 of a NaN is +0.0: rms / std of an item with a NaN
    for c in ("nanfirst_9", "nanmid_9", "nanlast_9"):
        assert u32(gold("rms_f32", c)["value"]) == 0 and u32(gold("std_f32", c)["value"]) == 0
        assert np.isnan(gold("mean_f32", c)["value"]) and np.isnan(gold("var_f32", c)["value"])
    assert np.isposinf(gold("power_f32", "overflow_9")["value"]) and np.isposinf(gold("accumulate_f32", "overflow_9")["value"])
    assert u32(gold("var_f32", "rand_1")["value"]) == 0 and u32(gold("std_f32", "rand_1")["value"]) == 0
    # absmax of +0.0 only: -0.0 at index 0; a NaN at 0 stays with its sign flipped, elsewhere it never wins
    g = gold("absmax_f32", "pzero_5")
    assert u32(g["value"]) == 0x80000000 and int(g["index"]) == 0
    for f in ("absmax_f32", "absmin_f32"):
        g = gold(f, "nanfirst_9")
        assert np.isnan(g["value"]) and int(g["index"]) == 0
        g = gold(f, "nanmid_9")
        assert not np.isnan(g["value"]) and int(g["index"]) != 4
    # max_no_idx_f32 starts from -FLT_MAX: all -Inf returns it, a NaN never wins, not even as element 0
    assert gold("max_no_idx_f32", "neginf_6")["value"] == -sr.FLT_MAX
    assert gold("min_no_idx_f32", "posinf_6")["value"] == sr.FLT_MAX
    assert not np.isnan(gold("max_no_idx_f32", "nanfirst_9")["value"])
    assert not np.isnan(gold("min_no_idx_f32", "nanfirst_9")["value"])
    assert np.isnan(gold("absmax_no_idx_f32", "nanfirst_9")["value"])
    # saturating negate; ties keep the lower index
    for t in ("q31", "q15", "q7"):
        i = np.iinfo(sr.DT[t])
        g = gold(f"absmax_{t}", "allmin_255")
        assert g["value"] == i.max and int(g["index"]) == 0
        g = gold(f"absmax_{t}", "abssat_9")
        assert g["value"] == i.max and int(g["index"]) == 2
        assert gold(f"absmax_no_idx_{t}", "allmin_255")["value"] == i.max
    for t in sr.TYPES:
        for f, n_first in ((f"absmax_{t}", 2), (f"absmin_{t}", 2)):
            assert int(gold(f, "abstie_9")["index"]) == n_first
            assert int(gold(f, "abstie2_300")["index"]) == 70
    # the integer mean truncates toward zero: (-13) / 3 = -4, (-5) / 7 = 0
    for t in ("q31", "q15", "q7"):
        assert gold(f"mean_{t}", "negmean_3")["value"] == -4 and gold(f"mean_{t}", "negmean_7")["value"] == 0
        assert gold(f"mse_{t}", "const_9")["value"] == 0
    for t in ("q31", "q15"):
        assert gold(f"var_{t}", "const_9")["value"] == 0 and gold(f"std_{t}", "const_9")["value"] == 0
    # rms_q15 of -32768 only: 32767 goes into arm_sqrt_q15
    assert gold("rms_q15", "allmin_255")["value"] == int(sr.sqrt_q15(np.array([32767]))[0])
    # rms_q31 sums x*x unshifted in an unsigned word: four minima already wrap it to 0
    assert sr.run("rms_q31", np.full(4, -2 ** 31, dtype=np.int32))["value"] == 0
    assert gold("rms_q31", "allmin_255")["value"] == sr.run("rms_q31", np.full(255, -2 ** 31, dtype=np.int32))["value"]
    # var_q15 at 65537 words: the uint32_t divisor 65537 * 65536 wraps to 65536
    g = gold("var_q15", "wrap_65537")
    a = g["a"].astype(np.int64)
    s, sq = int(a.sum()), int((a * a).sum())
    wrapped = ((sq // 65536) - (s * s) // 65536) >> 15
    exact = ((sq // 65536) - (s * s) // (65537 * 65536)) >> 15
    assert wrapped != exact and int(g["value"]) == sr._wrap(wrapped, 16)


def test_sqrt_q15_table_rule_and_whole_domain(dsp):
    """The 16 start words follow round(2^13 / sqrt(1 + k / 4)) and equal the reference's table; arm_sqrt_q15 (computed
    on the host) equals the reference on every int16 input, status included."""
    assert GOLD["sqrt_q15/lut"].tolist() == sr.SQRT_Q15_LUT.tolist()
    assert GOLD["sqrt_q15/lut"].tolist() == [8192, 7327, 6689, 6193, 5793, 5461, 5181, 4940, 4730, 4544, 4379, 4230,
                                             4096, 3974, 3862, 3759]
    xs = np.arange(-32768, 32768)
    want, status = GOLD["sqrt_q15/out"], GOLD["sqrt_q15/status"]
    assert want.tobytes() == sr.sqrt_q15(xs).astype(np.int16).tobytes()
    out = np.full(3, sr.MARK["q15"], dtype=np.int16)
    for i in range(0, xs.size, 7):                          # every seventh input and both ends through the C ABI
        out[1] = sr.MARK["q15"]
        assert dsp.lib.arm_sqrt_q15(int(xs[i]), out.ctypes.data + 2) == status[i], xs[i]
        assert out[1] == want[i] and out[0] == out[2] == sr.MARK["q15"], xs[i]
    for x in (-32768, -1, 0, 1, 32767):
        st, v = dsp.arm_sqrt_q15(x)
        assert (st, v) == (status[x + 32768], want[x + 32768])
    assert dsp.lib.arm_sqrt_q15(5, None) == ARGUMENT_ERROR


def test_library_exports_the_symbols(dsp):
    names = [f"arm_{f}{suffix}" for f in sr.FUNCS for suffix in ("", "_batch")] + ["arm_sqrt_q15"]
    assert len(set(names)) == 95 and set(names) == set(_abi.STATISTICS)
    for n in names:
        assert callable(getattr(dsp.lib, n)), n
    for header, suffix in (("arm_math.h", ""), ("arm_math_mi355x.h", "_batch")):
        text = open(os.path.join(ROOT, "include", header)).read()
        for f in ("mean", "power", "rms", "var", "std", "mse", "absmax", "absmin", "max_no_idx", "min_no_idx",
                  "absmax_no_idx", "absmin_no_idx"):
            assert f"arm_{f}_##SUF{'##' + suffix if suffix else ''}(" in text, (header, f)
        assert f"arm_accumulate_f32{suffix}(" in text and f"arm_cmplx_mag_fast_q15{suffix}(" in text


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for f in sr.FUNCS:
        fn = getattr(d, "arm_" + f)
        assert callable(fn) and "cmsis_arm_" + f in fn.__doc__, f
    assert callable(d.arm_sqrt_q15)
    for n in ("arm_stat", "arm_absmax", "arm_absmin", "arm_sqrt_q15", "arm_cmplx_mag_fast_q15", "mean_batch",
              "power_batch", "rms_batch", "var_batch", "std_batch", "mse_batch", "accumulate_batch", "absmax_batch",
              "absmin_batch", "max_no_idx_batch", "min_no_idx_batch", "absmax_no_idx_batch", "absmin_no_idx_batch",
              "cmplx_mag_fast_batch"):
        assert callable(getattr(dsp, n)), n


# ------------------------------------------------------------------ GPU helpers
class Dev:
    """A device copy of x whose first word sits `off` elements into a marker-filled allocation, GUARD marker words
    after its end."""

    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.t = _type_name(x)
        self.off, self.n, self.shape, self.dtype = off, x.size, x.shape, x.dtype
        raw = cm.marked(self.t, off + x.size + GUARD)
        raw[off:off + x.size] = x.reshape(-1)
        self.buf = torch.from_numpy(raw.view(np.uint8)).cuda()
        self.ptr = self.buf.data_ptr() + off * x.itemsize

    def get(self):
        """The words, after checking that nothing around them changed."""
        b = self.buf.cpu().numpy().view(self.dtype)
        m = cm.marked(self.t, 1).tobytes()
        assert b[:self.off].tobytes() == m * self.off and b[self.off + self.n:].tobytes() == m * GUARD, "guard words"
        return b[self.off:self.off + self.n].reshape(self.shape)


class Host:
    def __init__(self, x):
        self.a = np.ascontiguousarray(x).copy()
        self.ptr = self.a.ctypes.data

    def get(self):
        return self.a


def run_on(dsp, torch, func, g, where, off=0, batch=None):
    """arm_<func> (batch None: one item) or arm_<func>_batch on host arrays or device buffers at element offset off,
    the outputs pre-filled with the marker.  g["a"] (g["b"]): [n] or [batch, n].  -> (status, the outputs)."""
    put = (lambda x: Host(x)) if where == "host" else (lambda x: Dev(torch, x, off))
    a = np.asarray(g["a"])
    items = 1 if batch is None else batch
    src = [put(a)] + ([put(g["b"])] if sr.two_sources(func) else [])
    fn = getattr(dsp.lib, f"arm_{func}" + ("" if batch is None else "_batch"))
    tail = [] if batch is None else [batch, None]
    if func == "cmplx_mag_fast_q15":
        n = a.shape[-1] // 2
        out = {"value": put(cm.marked("q15", items * n))}
        st = fn(src[0].ptr, out["value"].ptr, n, *tail)
    else:
        n = a.shape[-1]
        out = {"value": put(cm.marked(sr.result_type(func), items))}
        if sr.has_index(func):
            out["index"] = put(cm.marked("u32", items))
        st = fn(*[s.ptr for s in src], n, *[o.ptr for o in out.values()], *tail)
    if where != "host":
        torch.cuda.synchronize()
    for s, k in zip(src, ("a", "b")):
        assert s.get().tobytes() == np.ascontiguousarray(g[k]).tobytes(), (func, k)
    return (0 if st is None else st), {k: o.get() for k, o in out.items()}


def rand_operands(func, shape, rng):
    """Random operands of `shape` = (..., n) inside the reference's contract."""
    if func == "cmplx_mag_fast_q15":
        return {"a": sr.rand("q15", shape[:-1] + (2 * shape[-1],), rng)}
    t = sr.split(func)[1]
    sh = sr.amp_shift(func, shape[-1])
    g = {"a": sr.rand(t, shape, rng, sh)}
    if sr.two_sources(func):
        g["b"] = sr.rand(t, shape, rng, sh)
    return g


# ------------------------------------------------------------------ GPU: every function against the fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("func", sr.FUNCS)
def test_batch_form_and_dropin_equal_fixtures(dsp, torch_gpu, func):
    """Every recorded case through the _batch form on device pointers (one item) and through the drop-in on host
    pointers; the short cases through the drop-in on device pointers too."""
    for case in CASES[func]:
        g = gold(func, case)
        st, got = run_on(dsp, torch_gpu, func, g, "device", batch=1)
        assert st == SUCCESS, (func, case, dsp.last_error())
        check(func, (case, "batch"), got, g)
        st, got = run_on(dsp, torch_gpu, func, g, "host")
        assert dsp.last_error()[0] == 0, (func, case, dsp.last_error())
        check(func, (case, "host"), got, g)
        if sr.case_n(case) <= 17:
            st, got = run_on(dsp, torch_gpu, func, g, "device")
            assert dsp.last_error()[0] == 0
            check(func, (case, "device"), got, g)


# ------------------------------------------------------------------ GPU: shapes
SHAPE_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 257, 1023, 1025, 4097)


@pytest.mark.gpu
@pytest.mark.parametrize("func", sr.STAT_FUNCS)
def test_item_lengths_batches_and_offsets(dsp, torch_gpu, func):
    """Batches of 3 items at every length with the source 16-B aligned and at element offsets 1, 2 and 3 (the
    one-element-per-load path; with an odd length the items after the first are unaligned anyway), 257 items at the
    lengths around a wave, and two items of 520 16-B packs of every type (the whole workgroup on whole packs)."""
    rng = np.random.default_rng(31)
    per_pack = 16 // np.dtype(sr.DT[sr.split(func)[1]]).itemsize
    shapes = [(3, n) for n in SHAPE_LENGTHS] + [(257, n) for n in (5, 64, 65, 300)] + \
        [(2, (REDUCE_WAVE_MAX + 8) * per_pack), (1, VAR_KEEP), (1, VAR_KEEP + 64)]
    for batch, n in shapes:
        g = rand_operands(func, (batch, n), rng)
        want = sr.run(func, g["a"], g.get("b"))
        for off in (0, 1, 2, 3) if batch == 3 else (0, 1):
            st, got = run_on(dsp, torch_gpu, func, g, "device", off=off, batch=batch)
            assert st == SUCCESS, (func, batch, n, off, dsp.last_error())
            check(func, (batch, n, off), got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", [f for f in SUMS if f.endswith("f32")])
def test_f32_lane_per_item_kernel(dsp, torch_gpu, func):
    """SUM_LANE_MIN_BATCH items and one more (the last workgroup holds one item) of short items: below, at and past
    one LDS stage of SUM_CHUNK words, and 4095 items (still one wave per item) for the same words."""
    rng = np.random.default_rng(37)
    for n in (1, 5, SUM_CHUNK, SUM_CHUNK + 1, 2 * SUM_CHUNK + 3):
        g = rand_operands(func, (SUM_LANE_MIN_BATCH + 1, n), rng)
        want = sr.run(func, g["a"], g.get("b"))
        for off in (0, 1):
            st, got = run_on(dsp, torch_gpu, func, g, "device", off=off, batch=SUM_LANE_MIN_BATCH + 1)
            assert st == SUCCESS
            check(func, ("lane", n, off), got, want)
        few = {k: v[:SUM_LANE_MIN_BATCH - 1] for k, v in g.items()}
        st, got = run_on(dsp, torch_gpu, func, few, "device", batch=SUM_LANE_MIN_BATCH - 1)
        check(func, ("wave", n), got, {"value": want["value"][:SUM_LANE_MIN_BATCH - 1]})


@pytest.mark.gpu
def test_cmplx_mag_fast_q15_shapes(dsp, torch_gpu):
    rng = np.random.default_rng(41)
    for n in (1, 2, 7, 8, 9, 63, 65, 1025):
        g = rand_operands("cmplx_mag_fast_q15", (n,), rng)
        want = sr.run("cmplx_mag_fast_q15", g["a"])
        for off in (0, 1, 3):
            st, got = run_on(dsp, torch_gpu, "cmplx_mag_fast_q15", g, "device", off=off)
            assert dsp.last_error()[0] == 0
            check("cmplx_mag_fast_q15", (n, off), got, want)
    g = rand_operands("cmplx_mag_fast_q15", (257, 5), rng)
    st, got = run_on(dsp, torch_gpu, "cmplx_mag_fast_q15", g, "device", batch=257)
    assert st == SUCCESS
    check("cmplx_mag_fast_q15", "batch", {"value": got["value"].reshape(257, 5)}, sr.run("cmplx_mag_fast_q15", g["a"]))


# ------------------------------------------------------------------ GPU: values
@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["subnormal", "negzero", "signzero", "mixed", "overflow", "nonfinite"])
def test_f32_classes_on_long_items(dsp, torch_gpu, cls):
    """Subnormals, signed zeros, sums that overflow and +-Inf / NaN at the first, a middle and the last position of
    items of 200 words (three full 64-lane steps and a ragged one), through the wave-per-item kernels (3 items) and
    the lane-per-item kernels (SUM_LANE_MIN_BATCH items of 40 words), and through every f32 search."""
    n = 200
    a = np.stack([f32_class_input(cls, n, 50 + i, scale=3.0e38, positions=p)
                  for i, p in enumerate(((0, 100, 199), (199, 0, 100), (100, 199, 0)))])
    b = np.stack([f32_class_input(cls, n, 60 + i, scale=3.0e38, positions=(1, 101, 198)) for i in range(3)])
    for func in [f for f in sr.STAT_FUNCS if f.endswith("f32")]:
        g = {"a": a, "b": b} if sr.two_sources(func) else {"a": a}
        st, got = run_on(dsp, torch_gpu, func, g, "device", batch=3)
        assert st == SUCCESS
        check(func, cls, got, sr.run(func, g["a"], g.get("b")))
    m = 40
    a = f32_class_input(cls, SUM_LANE_MIN_BATCH * m, 70, scale=3.0e38, positions=(0, 39, 20 + 40 * 5))
    a = a.reshape(SUM_LANE_MIN_BATCH, m)
    b = f32_class_input(cls, SUM_LANE_MIN_BATCH * m, 71, scale=3.0e38, positions=(1, 38, 21 + 40 * 5))
    b = b.reshape(SUM_LANE_MIN_BATCH, m)
    for func in [f for f in SUMS if f.endswith("f32")]:
        g = {"a": a, "b": b} if sr.two_sources(func) else {"a": a}
        st, got = run_on(dsp, torch_gpu, func, g, "device", batch=SUM_LANE_MIN_BATCH)
        assert st == SUCCESS
        check(func, (cls, "lane"), got, sr.run(func, g["a"], g.get("b")))


@pytest.mark.gpu
def test_fixed_point_extremes_on_vector_path(dsp, torch_gpu):
    """All-minimum, all-maximum and mixed extreme words at 256 words (whole 16-B packs, several lanes per item) and
    at 133 (single elements), two items each; a = -b at the extremes for mse."""
    rng = np.random.default_rng(43)
    for func in [f for f in sr.STAT_FUNCS if not f.endswith("f32")]:
        t = sr.split(func)[1]
        i = np.iinfo(sr.DT[t])
        for n in (256, 133):
            for fill in (i.min, i.max, None):
                a = np.full((2, n), fill, dtype=sr.DT[t]) if fill is not None else cm.extremes(t, (2, n), rng)
                g = {"a": a}
                if sr.two_sources(func):
                    g["b"] = np.where(a == i.min, i.max, np.where(a == i.max, i.min, a)).astype(sr.DT[t])
                assert all(sr.in_contract(func, g["a"][r], g["b"][r] if "b" in g else None) for r in range(2))
                st, got = run_on(dsp, torch_gpu, func, g, "device", batch=2)
                assert st == SUCCESS
                check(func, (n, fill), got, sr.run(func, g["a"], g.get("b")))


@pytest.mark.gpu
@pytest.mark.parametrize("func", SEARCHES)
def test_search_ties_across_lanes_waves_and_packs(dsp, torch_gpu, func):
    """|x| (or x) equal at two indices, with opposite signs for the abs searches, straddling a lane's loads, a wave
    and the workgroup's four waves: the lower index wins and its value is returned."""
    rng = np.random.default_rng(47)
    op, t = sr.split(func)
    is_max, is_abs = "max" in op, op.startswith("abs")
    dt = sr.DT[t]
    if t == "f32":
        field = lambda shape: (rng.uniform(0.25, 0.75, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)  # noqa: E731
        peak = np.float32(3.0 if is_max else (2.0 ** -10 if is_abs else -3.0))
    else:
        i = np.iinfo(dt)
        field = lambda shape: (rng.integers(i.max // 4, i.max // 2, shape) * rng.choice([-1, 1], shape)).astype(dt)  # noqa: E731
        peak = dt(i.max - 1 if is_max else (1 if is_abs else i.min + 1))
    per_pack = 16 // np.dtype(dt).itemsize
    n = 70000 // per_pack * per_pack
    for first, second in ((63 * per_pack + 1, 64 * per_pack), (255 * per_pack + 2, 256 * per_pack), (7, n - 1)):
        a = field(n)
        a[first], a[second] = (-peak if is_abs else peak), peak
        want = sr.run(func, a)
        for off in (0, 1):
            st, got = run_on(dsp, torch_gpu, func, {"a": a}, "device", off=off, batch=1)
            check(func, (first, second, off), got, want)
            if sr.has_index(func):
                assert int(got["index"][0]) == first
    c = field((4, 300))
    for row, (first, second) in enumerate(((3, 4), (17, 17 + 64), (0, 299), (150, 151))):
        c[row, first], c[row, second] = (-peak if is_abs else peak), peak
    for off in (0, 1):
        st, got = run_on(dsp, torch_gpu, func, {"a": c}, "device", off=off, batch=4)
        check(func, ("rows", off), got, sr.run(func, c))
        if sr.has_index(func):
            assert got["index"].tolist() == [3, 17, 0, 150]


# ------------------------------------------------------------------ GPU: refusals and the empty item
@pytest.mark.gpu
def test_refusals_and_block_size_zero(dsp, torch_gpu):
    """Null pointers and a result (or index) inside a source are refused and nothing is written; blockSize == 0
    stores what the reference's empty sums give, and is refused where the reference would divide an integer by zero
    or read pSrc[0]."""
    torch, lib = torch_gpu, dsp.lib
    rng = np.random.default_rng(53)
    for func in sr.STAT_FUNCS:
        op, t = sr.split(func)
        rt = sr.result_type(func)
        a = Dev(torch, sr.rand(t, 4 * 10, rng, 2))
        b = Dev(torch, sr.rand(t, 4 * 10, rng, 2))
        res, idx = Dev(torch, cm.marked(rt, 4)), Dev(torch, cm.marked("u32", 4))
        name = "arm_" + func
        fb, fd = getattr(lib, name + "_batch"), getattr(lib, name)

        def args(src, n, r, i=idx.ptr, other=b.ptr):
            return ([src, other] if op == "mse" else [src]) + [n, r] + ([i] if sr.has_index(func) else [])

        def void(*call, fails):
            fd(*call)
            code, msg = dsp.last_error()
            assert (code != 0) == fails and (not fails or name in msg), (name, call, code, msg)
            lib.arm_mi355x_clear_error()

        # null pointers
        assert fb(*args(None, 10, res.ptr), 4, None) == ARGUMENT_ERROR
        assert fb(*args(a.ptr, 10, None), 4, None) == ARGUMENT_ERROR
        void(*args(None, 10, res.ptr), fails=True)
        void(*args(a.ptr, 10, None), fails=True)
        if op == "mse":
            assert fb(*args(a.ptr, 10, res.ptr, other=None), 4, None) == ARGUMENT_ERROR
            void(*args(a.ptr, 10, res.ptr, other=None), fails=True)
        if sr.has_index(func):
            assert fb(*args(a.ptr, 10, res.ptr, i=None), 4, None) == ARGUMENT_ERROR
            void(*args(a.ptr, 10, res.ptr, i=None), fails=True)
        assert fb(*args(a.ptr, 10, res.ptr), 0, None) == SUCCESS                     # batch == 0
        # a result inside a source (not run to see what happens: refused before any launch)
        item = np.dtype(sr.MDT[rt]).itemsize
        inside = a.ptr // item * item + item
        assert fb(*args(a.ptr, 10, inside), 4, None) == ARGUMENT_ERROR
        void(*args(a.ptr, 10, inside), fails=True)
        if op == "mse":
            inside_b = b.ptr // item * item + item
            assert fb(*args(a.ptr, 10, inside_b), 4, None) == ARGUMENT_ERROR
        if sr.has_index(func):
            assert fb(*args(a.ptr, 10, res.ptr, i=a.ptr // 4 * 4 + 8), 4, None) == ARGUMENT_ERROR
            assert fb(*args(a.ptr, 10, idx.ptr, i=idx.ptr), 4, None) == ARGUMENT_ERROR
        lib.arm_mi355x_clear_error()
        torch.cuda.synchronize()
        assert res.get().tobytes() == cm.marked(rt, 4).tobytes() and idx.get().tobytes() == cm.marked("u32", 4).tobytes()
        a.get(), b.get()
        # blockSize == 0
        f32 = t == "f32"
        if op in ("power", "accumulate", "var", "std") or (f32 and op in ("mean", "mse", "rms")) or \
                (f32 and op in ("max_no_idx", "min_no_idx")):
            assert fb(*args(a.ptr, 0, res.ptr), 3, None) == SUCCESS
            void(*args(a.ptr, 0, res.ptr + 3 * item), fails=False)
            torch.cuda.synchronize()
            got = res.get()
            if f32 and op in ("mean", "mse"):
                assert np.isnan(got).all()
            elif op == "max_no_idx":
                assert (got == -sr.FLT_MAX).all()
            elif op == "min_no_idx":
                assert (got == sr.FLT_MAX).all()
            else:
                assert got.tobytes() == bytes(4 * item), (func, got)                 # +0.0 / 0
        else:
            assert fb(*args(a.ptr, 0, res.ptr), 3, None) == ARGUMENT_ERROR
            void(*args(a.ptr, 0, res.ptr), fails=True)
            torch.cuda.synchronize()
            assert res.get().tobytes() == cm.marked(rt, 4).tobytes()
        lib.arm_mi355x_clear_error()
    assert lib.arm_mi355x_last_error() == 0


# ------------------------------------------------------------------ GPU: the Python layers
@pytest.mark.gpu
def test_python_wrappers(dsp, torch_gpu):
    """cmsisdsp's names with the reference binding's return shapes, and cmsisdsp_amd's batched forms on tensors."""
    import cmsisdsp as d
    torch = torch_gpu
    for func in sr.FUNCS:
        g = gold(func, "rand_65" if func != "cmplx_mag_fast_q15" else "rand_67")
        got = getattr(d, "arm_" + func)(*[g[k] for k in ("a", "b") if k in g])
        if func == "cmplx_mag_fast_q15":
            assert isinstance(got, np.ndarray) and got.tobytes() == g["value"].tobytes()
            continue
        t = sr.split(func)[1]
        val = got[0] if sr.has_index(func) else got
        assert isinstance(val, float if sr.result_type(func) == "f32" else int), func
        assert sr.MDT[sr.result_type(func)](val) == g["value"], func
        if sr.has_index(func):
            assert isinstance(got, tuple) and got[1] == int(g["index"]), func
    assert d.arm_sqrt_q15(16384) == (0, int(sr.sqrt_q15(np.array([16384]))[0])) and d.arm_sqrt_q15(-5) == (-1, 0)
    rng = np.random.default_rng(59)
    dev = lambda x: torch.from_numpy(x).cuda()                                   # noqa: E731
    for t in sr.TYPES:
        a, b = sr.rand(t, (6, 35), rng), sr.rand(t, (6, 35), rng)
        ta, tb = dev(a), dev(b)
        ops = ["mean", "power", "max_no_idx", "min_no_idx", "absmax_no_idx", "absmin_no_idx"]
        ops += ["rms", "var", "std"] if t != "q7" else []
        ops += ["accumulate"] if t == "f32" else []
        for op in ops:
            rt = sr.result_type(f"{op}_{t}")
            res = dev(cm.marked(rt, 6))
            getattr(dsp, op + "_batch")(ta, res)
            assert sr.same_words(res.cpu().numpy(), sr.run(f"{op}_{t}", a)["value"], rt == "f32"), (op, t)
        res = dev(cm.marked(t, 6))
        dsp.mse_batch(ta, tb, res)
        assert sr.same_words(res.cpu().numpy(), sr.run(f"mse_{t}", a, b)["value"], t == "f32")
        for op in ("absmax", "absmin"):
            res, idx = dev(cm.marked(t, 6)), dev(cm.marked("u32", 6).view(np.int32))
            getattr(dsp, op + "_batch")(ta, res, idx)
            want = sr.run(f"{op}_{t}", a)
            assert res.cpu().numpy().tobytes() == want["value"].tobytes()
            assert idx.cpu().numpy().view(np.uint32).tolist() == want["index"].tolist()
        with pytest.raises(RuntimeError):
            dsp.mean_batch(ta, ta[0])
        dsp.lib.arm_mi355x_clear_error()
    z = sr.rand("q15", (4, 2 * 19), rng)
    out = dev(cm.marked("q15", (4, 19)))
    dsp.cmplx_mag_fast_batch(dev(z), out)
    assert out.cpu().numpy().tobytes() == sr.cmplx_mag_fast_q15(z).tobytes()
