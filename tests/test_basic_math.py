"""arm_{add,sub,mult,offset,scale,clip,abs,negate,dot_prod}_{f32,q31,q15,q7}, arm_shift_{q31,q15,q7} and
arm_{and,or,xor,not}_{u32,u16,u8}: 51 drop-ins and their _batch forms (cmsis-dsp_amd/csrc/basic_math.hip; the dot
products are operations of the sum kernels of statistics.hip).

The checker is committed data: tests/golden/basic_math.npz holds the reference's own outputs, each in a buffer
pre-filled with a marker word with a guard word either side (tools/make_golden_basic_math.py);
tests/basic_math_ref.py restates the functions in numpy and Python ints, and the generator asserted it against the
reference case by case.  Every comparison is bit-exact; f32 outputs follow the rule of tests/test_f32_classes.py
(non-NaN words bit-equal, NaNs at the same positions).

CPU: the fixture index, the restatement against every fixture, the probed facts, in_contract, the exported symbols,
the Python names.  GPU: every function through its _batch form and its drop-in against every fixture (batch 1 and a
batch of several items cut from the fixture list); every pointer in turn one element off 16-byte alignment (the
one-element-per-lane path), guard words after every device buffer; dst == srcA and dst == srcB; the dot products at
the item counts either side of the chain kernels' switch, at the lanes-per-item steps and with bStride 0, ==
blockSize and > blockSize; every refusal."""
import json
import os

import numpy as np
import pytest

import basic_math_ref as br
from cmsisdsp_amd import _abi
from f32_classes import f32_class_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "basic_math.npz"))
INDEX = [(f, list(c)) for f, c in json.loads(str(GOLD["index"]))]
CASES = dict(INDEX)
GUARD = 8                      # marker words after the end of every device buffer
SUCCESS, ARGUMENT_ERROR = 0, -1
# the constants of basic_math.hip, statistics.hip and reduce_lanes.hpp that decide a kernel's path
BLOCK = 256                    # kBlock: lanes of a workgroup
EW_UNROLL = 4                  # kBmUnroll: 16-B packs a lane has in flight; a tile is BLOCK * EW_UNROLL packs
REDUCE_WAVE_MAX = 512          # kRedWaveMax: loads (16-B packs when aligned, else words) a wave takes per item
SUM_LANE_MIN_BATCH = 4096      # kSumLaneMinBatch: from here on dot_prod_f32 runs one lane per item
SUM_CHUNK = 16                 # kSumChunk: words per item and LDS stage of the lane-per-item kernel
EW = [f for f in br.FUNCS if not br.is_dot(f)]
DOTS = [f for f in br.FUNCS if br.is_dot(f)]


def _type_name(a):
    return {np.dtype(v): k for k, v in br.MDT.items()}[np.asarray(a).dtype]


def unguard(buf):
    """A fixture output buffer -> its words, after checking the guard word either side."""
    m = np.asarray(br.MARK[_type_name(buf)]).tobytes()
    assert buf[:1].tobytes() == m and buf[-1:].tobytes() == m, "guard words"
    return buf[1:-1]


_OFFSETS = {}


def gold(func, case):
    """{"a", "b", "scalars"} of one recorded case and its reference output: "dst" (None for a case longer than
    STORE_MAX words, whose output is pinned by "dcrc") or "value"."""
    names = CASES[func]
    k = names.index(case)
    g = br.operands(func, case)
    if func not in _OFFSETS:
        sizes = [br.case_n(c) if br.stored(c) else 0 for c in names]
        _OFFSETS[func] = (np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum([s + 2 if s else 0 for s in sizes])]))
    if br.stored(case):
        lo, hi = _OFFSETS[func][0][k], _OFFSETS[func][0][k + 1]
        for key in ("a", "b"):
            if key in g:
                g[key] = GOLD[f"{func}/{key}"][lo:hi]
    assert br.crc(g) == int(GOLD[f"{func}/crc"][k]), (func, case, "operands differ from the recorded ones")
    g["dcrc"] = int(GOLD[f"{func}/dcrc"][k])
    if br.is_dot(func):
        g["value"] = unguard(GOLD[f"{func}/value"][k]).reshape(())
        assert br.out_crc(g["value"]) == g["dcrc"]
    elif br.stored(case):
        lo, hi = _OFFSETS[func][1][k], _OFFSETS[func][1][k + 1]
        g["dst"] = unguard(GOLD[f"{func}/dst"][lo:hi])
        assert br.out_crc(g["dst"]) == g["dcrc"]
    else:
        g["dst"] = None
    return g


def restated(func, g):
    return br.run(func, g["a"], g.get("b"), g["scalars"])


def expected(func, g):
    """The reference's output of a recorded case: the recorded words, or for a long case the restatement's after
    checking their CRC against the reference's."""
    key = "value" if br.is_dot(func) else "dst"
    if g[key] is not None:
        return g[key]
    want = restated(func, g)[key]
    assert br.out_crc(want) == g["dcrc"], (func, "the restatement differs from the reference's output")
    return want


def check(func, what, got, want):
    g, w = np.asarray(got), np.asarray(want)
    assert br.same_words(g.reshape(w.shape), w, br.nan_rule(func)), (func, what, g.reshape(-1)[:8], w.reshape(-1)[:8])


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    """51 functions; every case of the case list is recorded, every length, extreme, count and clip case of the
    issue among them."""
    assert len(br.FUNCS) == 51 and len(set(br.FUNCS)) == 51
    assert [f for f, _ in INDEX] == list(br.FUNCS)
    lengths = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257, 1023, 1025, 4097, 33000)
    for f, cases in INDEX:
        op, t = br.split(f)
        assert cases == br.case_names(f), f
        assert cases[:22] == [f"rand_{n}" for n in lengths], f
        if t == "f32":
            assert set(br.F32_CASES) <= set(cases), f
        else:
            assert {"allmin_255", "allmax_255", "minmax_257", "alt_1025"} <= set(cases), f
        if op == "clip":
            assert {"clipeq_17", "clipinv_17", "clipext_17"} <= set(cases), f
    for f, (lo, hi) in br.SHIFT_RANGE.items():
        for c in range(lo, hi + 1):
            assert f"cnt{c}_17" in CASES[f], (f, c)
        assert f"cnt{lo - 1}_17" not in CASES[f] and f"cnt{hi + 1}_17" not in CASES[f]
    assert br.SHIFT_RANGE == {"shift_q31": (-31, 31), "shift_q15": (-31, 31), "shift_q7": (-31, 31),
                              "scale_q31": (-32, 30), "scale_q15": (-16, 15), "scale_q7": (-24, 7)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "basic_math.npz")) < 1 << 20


def test_restatement_equals_every_fixture():
    for f, cases in INDEX:
        key = "value" if br.is_dot(f) else "dst"
        for c in cases:
            g = gold(f, c)
            check(f, c, restated(f, g)[key], expected(f, g))


def _one(func, a, case):
    """The recorded output word of `case` at the first position that holds the operand word a."""
    g = gold(func, case)
    pos = int(np.flatnonzero(g["a"] == a)[0])
    return int(g["dst"][pos])


def test_probed_facts_hold_in_the_fixtures():
    """The traps the issue lists, read off the reference's own outputs."""
    i31, i15, i7 = (np.iinfo(br.DT[t]) for t in ("q31", "q15", "q7"))
    # shift_q31 by 31: 1 -> INT32_MAX, -1 -> INT32_MIN, INT32_MIN -> INT32_MIN
    assert _one("shift_q31", 1, "cnt31_17") == i31.max
    assert _one("shift_q31", -1, "cnt31_17") == i31.min
    assert _one("shift_q31", i31.min, "cnt31_17") == i31.min
    # scale_q31(x, 0x40000000, -32): 0 for x >= 0, -1 for x < 0
    g = gold("scale_q31", "cnt-32_17")
    assert g["scalars"] == (0x40000000, -32)
    assert g["dst"].tolist() == np.where(g["a"] >= 0, 0, -1).tolist()
    # shift_q15 by 17 shows the 32-bit wrap: 16384 -> -32768, -32768 -> 0, 1 -> 32767
    assert _one("shift_q15", 16384, "cnt17_17") == -32768
    assert _one("shift_q15", -32768, "cnt17_17") == 0
    assert _one("shift_q15", 1, "cnt17_17") == 32767
    assert _one("shift_q15", 16384, "cnt16_17") == 32767           # exact up to 16
    assert _one("shift_q7", 64, "cnt25_17") == -128                # the same shape on an int, 8 bits: 64 << 25 = 2^31
    # mult_q31: the low bit is always 0, min * min saturates to 0x7FFFFFFE
    for c in ("rand_257", "ext_67", "allmin_255"):
        assert not (gold("mult_q31", c)["dst"] & 1).any()
    assert set(gold("mult_q31", "allmin_255")["dst"].tolist()) == {0x7FFFFFFE}
    assert set(gold("mult_q15", "allmin_255")["dst"].tolist()) == {32767}
    assert set(gold("mult_q7", "allmin_255")["dst"].tolist()) == {127}
    # add / sub saturate
    for t, i in (("q31", i31), ("q15", i15), ("q7", i7)):
        assert set(gold(f"add_{t}", "allmin_255")["dst"].tolist()) == {i.min}
        assert set(gold(f"add_{t}", "allmax_255")["dst"].tolist()) == {i.max}
        assert set(gold(f"sub_{t}", "minmax_257")["dst"].tolist()) == {i.min}
        # abs / negate of the most negative word
        assert set(gold(f"abs_{t}", "allmin_255")["dst"].tolist()) == {i.max}
        assert set(gold(f"negate_{t}", "allmin_255")["dst"].tolist()) == {i.max}
        # clip: low == high gives that word everywhere; low > high: the first comparison wins
        g = gold(f"clip_{t}", "clipeq_17")
        assert set(g["dst"].tolist()) == {g["scalars"][0]}
        g = gold(f"clip_{t}", "clipinv_17")
        low, high = g["scalars"]
        assert low > high
        assert g["dst"].tolist() == [high if x > high else (low if x < low else x) for x in g["a"].tolist()]
        assert set(g["dst"].tolist()) <= {low, high}
    # f32: abs clears the sign of -0.0, negate flips it; a NaN passes through clip
    g = gold("abs_f32", "signzero_9")
    assert np.signbit(g["a"]).any() and not g["dst"].view(np.uint32).any()
    g = gold("negate_f32", "signzero_9")
    assert (g["dst"].view(np.uint32) == (g["a"].view(np.uint32) ^ 0x80000000)).all()
    g = gold("clip_f32", "clipnan_9")
    assert np.isnan(g["dst"][[0, 4, 8]]).all() and not np.isnan(np.delete(g["dst"], [0, 4, 8])).any()
    # dot_prod_f32 is one ordered chain without FMA: the restatement's plain loop is bit-equal on 33000 words
    g = gold("dot_prod_f32", "rand_33000")
    acc = np.float32(0.0)
    for p in (g["a"] * g["b"]).tolist():
        acc = np.float32(acc + np.float32(p))
    assert acc.tobytes() == g["value"].tobytes()
    # dot_prod_q31 adds (a*b) >> 14; q15 the exact products; q7 into 32 bits
    assert int(gold("dot_prod_q31", "allmin_255")["value"]) == 255 * (2 ** 62 >> 14)
    assert int(gold("dot_prod_q15", "allmin_255")["value"]) == 255 * 2 ** 30
    assert int(gold("dot_prod_q7", "allmin_255")["value"]) == 255 * 2 ** 14
    assert gold("dot_prod_q7", "allmin_255")["value"].dtype == np.int32
    assert gold("dot_prod_q15", "allmin_255")["value"].dtype == np.int64


def test_contract_check_rejects_what_it_should():
    """in_contract(): the shift counts either side of every range, and the dot products' sums."""
    for f, (lo, hi) in br.SHIFT_RANGE.items():
        pre = (1,) if f.startswith("scale") else ()
        assert br.in_contract(f, scalars=pre + (lo,)) and br.in_contract(f, scalars=pre + (hi,))
        assert not br.in_contract(f, scalars=pre + (lo - 1,)) and not br.in_contract(f, scalars=pre + (hi + 1,))
    m7 = np.full(131072, -128, dtype=np.int8)
    assert br.in_contract("dot_prod_q7", m7[:131071], m7[:131071]) and not br.in_contract("dot_prod_q7", m7, m7)
    m31 = np.full(32768, -2 ** 31, dtype=np.int32)
    assert br.in_contract("dot_prod_q31", m31[:32767], m31[:32767]) and not br.in_contract("dot_prod_q31", m31, m31)
    for f, cases in INDEX:
        for c in cases:
            if br.case_n(c) <= 300:
                g = br.operands(f, c)
                assert br.in_contract(f, g["a"], g.get("b"), g["scalars"]), (f, c)


def test_library_exports_the_symbols(dsp):
    names = [f"arm_{f}{suffix}" for f in br.FUNCS for suffix in ("", "_batch")]
    assert len(set(names)) == 102 and set(names) == set(_abi.BASIC_MATH)
    for n in names:
        assert callable(getattr(dsp.lib, n)), n
    for header, suffix in (("arm_math.h", ""), ("arm_math_mi355x.h", "_batch")):
        text = open(os.path.join(ROOT, "include", header)).read()
        for op in ("add", "sub", "mult", "offset", "scale", "shift", "clip", "abs", "negate", "dot_prod", "and", "or",
                   "xor", "not"):
            assert f"arm_{op}_##SUF{'##' + suffix if suffix else ''}(" in text, (header, op)
        assert f"arm_scale_f32{suffix}(" in text


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for f in br.FUNCS:
        fn = getattr(d, "arm_" + f)
        assert callable(fn) and "cmsis_arm_" + f in fn.__doc__, f
    for n in ("arm_basic1", "arm_basic2", "arm_dot_prod", "add_batch", "sub_batch", "mult_batch", "offset_batch",
              "scale_batch", "shift_batch", "clip_batch", "abs_batch", "negate_batch", "and_batch", "or_batch",
              "xor_batch", "not_batch", "dot_prod_batch"):
        assert callable(getattr(dsp, n)), n


# ------------------------------------------------------------------ GPU helpers
class Dev:
    """A device copy of x whose first word sits `off` elements into a marker-filled allocation (which is 16-byte
    aligned), GUARD marker words after its end."""

    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.t = _type_name(x)
        self.off, self.n, self.shape, self.dtype = off, x.size, x.shape, x.dtype
        raw = br.marked(self.t, off + x.size + GUARD)
        raw[off:off + x.size] = x.reshape(-1)
        self.buf = torch.from_numpy(raw.view(np.uint8)).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + off * x.itemsize

    def get(self):
        """The words, after checking that nothing around them changed."""
        b = self.buf.cpu().numpy().view(self.dtype)
        m = br.marked(self.t, 1).tobytes()
        assert b[:self.off].tobytes() == m * self.off and b[self.off + self.n:].tobytes() == m * GUARD, "guard words"
        return b[self.off:self.off + self.n].reshape(self.shape)


class Host:
    def __init__(self, x):
        self.a = np.ascontiguousarray(x).copy()
        self.ptr = self.a.ctypes.data

    def get(self):
        return self.a


def call_args(func, srcs, out, scalars, n):
    """The C argument list of arm_<func> up to the length (dot products: the length, then the result)."""
    if br.is_dot(func):
        return [*srcs, n, out]
    if br.split(func)[0] == "clip":
        return [*srcs, out, *scalars, n]
    return [*srcs, *scalars, out, n]


def run_on(dsp, torch, func, g, where, offs=(0, 0, 0), batch=None, b_stride=None, alias=None):
    """arm_<func> (batch None: one item) or arm_<func>_batch on host arrays or device buffers whose a, b and output
    start offs elements into their allocations, the output pre-filled with the marker.  g["a"] (g["b"]): [n] or
    [batch, n]; b_stride (dot products): words between the items' b vectors, g["b"] holding them as the call sees
    them.  alias "a" / "b": the output is that source's buffer.  -> (status, the output words)."""
    put = (lambda x, off: Host(x)) if where == "host" else (lambda x, off: Dev(torch, x, off))
    a = np.asarray(g["a"])
    n = a.shape[-1]
    items = 1 if batch is None else batch
    src = {"a": put(a, offs[0])}
    if br.two_sources(func):
        src["b"] = put(g["b"], offs[1])
    rt = br.result_type(func)
    out = src[alias] if alias else put(br.marked(rt, items if br.is_dot(func) else a.shape), offs[2])
    fn = getattr(dsp.lib, f"arm_{func}" + ("" if batch is None else "_batch"))
    ptrs = [s.ptr for s in src.values()]
    if br.is_dot(func) and batch is not None:
        args = [*ptrs, n if b_stride is None else b_stride, n, out.ptr, batch, None]
    else:
        args = call_args(func, ptrs, out.ptr, g["scalars"], n) + ([] if batch is None else [batch, None])
    st = fn(*args)
    if where != "host":
        torch.cuda.synchronize()
    got = out.get()
    for k, s in src.items():
        if k != alias:
            assert s.get().tobytes() == np.ascontiguousarray(g[k]).tobytes(), (func, k, "a source changed")
    return (0 if st is None else st), got


def rand_operands(func, shape, rng):
    t = br.split(func)[1]
    g = {"a": br.rand(t, shape, rng), "scalars": br.rand_scalars(func, rng)}
    if br.two_sources(func):
        g["b"] = br.rand(t, shape, rng)
    return g


# ------------------------------------------------------------------ GPU: every function against the fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("func", br.FUNCS)
def test_batch_form_and_dropin_equal_fixtures(dsp, torch_gpu, func):
    """Every recorded case through the _batch form on device pointers (one item) and through the drop-in on host
    pointers; the short cases through the drop-in on device pointers too."""
    key = "value" if br.is_dot(func) else "dst"
    for case in CASES[func]:
        g = gold(func, case)
        want = expected(func, g)
        st, got = run_on(dsp, torch_gpu, func, g, "device", batch=1)
        assert st == SUCCESS, (func, case, dsp.last_error())
        check(func, (case, "batch"), got, want)
        st, got = run_on(dsp, torch_gpu, func, g, "host")
        assert dsp.last_error()[0] == 0, (func, case, dsp.last_error())
        check(func, (case, "host"), got, want)
        if br.case_n(case) <= 17:
            st, got = run_on(dsp, torch_gpu, func, g, "device")
            assert dsp.last_error()[0] == 0
            check(func, (case, "device"), got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", br.FUNCS)
def test_batches_cut_from_the_fixture_list(dsp, torch_gpu, func):
    """Several items in one call: the fixture cases of one length that share their scalars, stacked ([items, n]), and
    the rand_33000 case cut into 8 items of 4125 words."""
    key = "value" if br.is_dot(func) else "dst"
    groups = {}
    for case in CASES[func]:
        if br.stored(case):
            g = gold(func, case)
            groups.setdefault((br.case_n(case), g["scalars"]), []).append(g)
    stacked = [v for v in groups.values() if len(v) > 1]
    assert stacked or func in br.SHIFT_RANGE or br.n_scalars(func), func
    for items in stacked:
        g = {k: np.stack([it[k] for it in items]) for k in ("a", "b") if k in items[0]}
        g["scalars"] = items[0]["scalars"]
        st, got = run_on(dsp, torch_gpu, func, g, "device", batch=len(items))
        assert st == SUCCESS
        check(func, ("stacked", len(items)), got, np.stack([it[key] for it in items]))
    g = gold(func, "rand_33000")
    cut = {k: g[k].reshape(8, 4125) for k in ("a", "b") if k in g}
    cut["scalars"] = g["scalars"]
    st, got = run_on(dsp, torch_gpu, func, cut, "device", batch=8)
    assert st == SUCCESS
    if br.is_dot(func):
        check(func, "cut", got, restated(func, cut)["value"])
    else:
        check(func, "cut", got.reshape(-1), expected(func, g))


# ------------------------------------------------------------------ GPU: alignment, aliasing, tiles
EW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257, 1023, 1025, 4097)


@pytest.mark.gpu
@pytest.mark.parametrize("func", EW)
def test_pointer_offsets_and_guard_words(dsp, torch_gpu, func):
    """a, b and d in turn one element off 16-byte alignment (the whole call then runs one element per lane), all
    aligned (16-byte packs and the ragged end), at every length and for 3 items; one call of more than two tiles of
    the pack path with a ragged end.  Every device buffer ends in guard words."""
    rng = np.random.default_rng(61)
    t = br.split(func)[1]
    per_pack = 16 // np.dtype(br.DT[t]).itemsize
    shapes = [(n,) for n in EW_LENGTHS] + [(3, n) for n in (5, 16, 33, 257)] + \
        [(2 * BLOCK * EW_UNROLL * per_pack + BLOCK * per_pack + 3,)]
    for shape in shapes:
        g = rand_operands(func, shape, rng)
        want = restated(func, g)["dst"]
        offsets = [(0, 0, 0), (1, 0, 0), (0, 0, 1)] + ([(0, 1, 0)] if br.two_sources(func) else [])
        for offs in offsets:
            st, got = run_on(dsp, torch_gpu, func, g, "device", offs=offs, batch=shape[0] if len(shape) == 2 else 1)
            assert st == SUCCESS, (func, shape, offs, dsp.last_error())
            check(func, (shape, offs), got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", EW)
def test_dst_may_be_a_source(dsp, torch_gpu, func):
    """dst == srcA and dst == srcB, on the pack path and on the one-element path, through the _batch form and the
    drop-in on device pointers."""
    rng = np.random.default_rng(67)
    for shape, off in (((4, 1031), 0), ((4, 1031), 1), ((70,), 0)):
        g = rand_operands(func, shape, rng)
        want = restated(func, g)["dst"]
        for alias in ("a", "b") if br.two_sources(func) else ("a",):
            batch = shape[0] if len(shape) == 2 else None
            st, got = run_on(dsp, torch_gpu, func, g, "device", offs=(off, off, off), batch=batch, alias=alias)
            assert st == SUCCESS and dsp.last_error()[0] == 0, (func, shape, alias, dsp.last_error())
            check(func, (shape, off, alias), got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["subnormal", "negzero", "signzero", "mixed", "overflow", "nonfinite"])
def test_f32_classes(dsp, torch_gpu, cls):
    """Subnormals, signed zeros, overflow to +-Inf and Inf / NaN inputs through every f32 function, on the pack path
    (1027 words) and through the dot product's two chain kernels."""
    n = 1027
    a = f32_class_input(cls, n, 80, scale=3.0e38, positions=(0, 500, 1026))
    b = f32_class_input(cls, n, 81, scale=3.0e38, positions=(1, 500, 1025))
    for func in [f for f in EW if f.endswith("f32")]:
        op = br.split(func)[0]
        scalars = {"offset": (float(a[3]),), "scale": (float(b[7]) if np.isfinite(b[7]) else 2.0,),
                   "clip": (-0.5, 0.5)}.get(op, ())
        g = {"a": a, "b": b, "scalars": scalars} if br.two_sources(func) else {"a": a, "scalars": scalars}
        st, got = run_on(dsp, torch_gpu, func, g, "device", batch=1)
        assert st == SUCCESS
        check(func, cls, got, restated(func, g)["dst"])
    m = 40
    for items in (3, SUM_LANE_MIN_BATCH):
        a = f32_class_input(cls, items * m, 82, scale=3.0e38, positions=(0, 39, 20 + 40 * 2)).reshape(items, m)
        b = f32_class_input(cls, items * m, 83, scale=3.0e38, positions=(1, 38, 21 + 40 * 2)).reshape(items, m)
        g = {"a": a, "b": b, "scalars": ()}
        st, got = run_on(dsp, torch_gpu, "dot_prod_f32", g, "device", batch=items)
        assert st == SUCCESS
        check("dot_prod_f32", (cls, items), got, restated("dot_prod_f32", g)["value"])


# ------------------------------------------------------------------ GPU: the dot products' paths
@pytest.mark.gpu
@pytest.mark.parametrize("func", DOTS)
def test_dot_prod_paths_and_strides(dsp, torch_gpu, func):
    """bStride == 0 (one shared b), == blockSize and > blockSize, at the lanes-per-item steps (1 .. 64 lanes, the
    whole workgroup past REDUCE_WAVE_MAX loads, 16-byte packs or single elements) for 3 and 257 items, and for
    dot_prod_f32 at SUM_LANE_MIN_BATCH - 1 items (one wave per item) and SUM_LANE_MIN_BATCH + 1 (one lane per item,
    below, at and past one LDS stage of SUM_CHUNK words)."""
    rng = np.random.default_rng(71)
    t = br.split(func)[1]
    per_pack = 16 // np.dtype(br.DT[t]).itemsize
    lengths = sorted({1, 2, 3, 5, 8, 17, 64, 65, 2 * per_pack, 4 * per_pack, 8 * per_pack + 1, 64 * per_pack,
                      128 * per_pack, (REDUCE_WAVE_MAX + 8) * per_pack, REDUCE_WAVE_MAX + 9})
    shapes = [(3, n) for n in lengths] + [(257, n) for n in (5, 64, 8 * per_pack)]
    if t == "f32":
        shapes += [(SUM_LANE_MIN_BATCH - 1, 5), (SUM_LANE_MIN_BATCH - 1, SUM_CHUNK + 1)]
        shapes += [(SUM_LANE_MIN_BATCH + 1, n) for n in (1, 5, SUM_CHUNK, SUM_CHUNK + 1, 2 * SUM_CHUNK + 3)]
    for batch, n in shapes:
        a = br.rand(t, (batch, n), rng)
        for stride in (0, n, n + 3, n + per_pack):
            rows = br.rand(t, (1 if stride == 0 else batch, max(stride, n)), rng)
            b_seen = np.broadcast_to(rows[:, :n], (batch, n))
            # the buffer handed over ends with the last item's n words
            flat = rows.reshape(-1)[:(batch - 1) * stride + n]
            want = br.run(func, a, b_seen)["value"]
            for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0)) if batch <= 257 else ((0, 0, 0),):
                g = {"a": a, "b": flat, "scalars": ()}
                st, got = run_on(dsp, torch_gpu, func, g, "device", offs=offs, batch=batch, b_stride=stride)
                assert st == SUCCESS, (func, batch, n, stride, offs, dsp.last_error())
                check(func, (batch, n, stride, offs), got, want)


@pytest.mark.gpu
def test_fixed_point_extremes_on_both_paths(dsp, torch_gpu):
    """All-minimum, all-maximum, min x max and mixed extreme words at 4 x 256 words (whole 16-byte packs) and 133
    (single elements) through every fixed-point and bitwise function, with the scalars at the extremes too."""
    rng = np.random.default_rng(73)
    for func in [f for f in br.FUNCS if not f.endswith("f32")]:
        op, t = br.split(func)
        i = np.iinfo(br.DT[t])
        for shape in ((4, 256), (133,)):
            for fa, fb in ((i.min, i.min), (i.max, i.max), (i.min, i.max), (None, None)):
                a = np.full(shape, fa, dtype=br.DT[t]) if fa is not None else br.extremes(t, shape, rng)
                b = np.full(shape, fb, dtype=br.DT[t]) if fb is not None else br.extremes(t, shape, rng)
                scalars = {"offset": (int(i.min if fa == i.min else i.max),), "scale": (int(i.min), 0),
                           "shift": (3,), "clip": (int(i.min), int(i.max))}.get(op, ())
                g = {"a": a, "scalars": scalars}
                if br.two_sources(func):
                    g["b"] = b
                batch = shape[0] if len(shape) == 2 else 1
                st, got = run_on(dsp, torch_gpu, func, g, "device", batch=batch)
                assert st == SUCCESS
                check(func, (shape, fa, fb), got, restated(func, g)["value" if br.is_dot(func) else "dst"])


# ------------------------------------------------------------------ GPU: refusals
@pytest.mark.gpu
def test_refusals(dsp, torch_gpu):
    """Null pointers, an output that partly overlaps a source, a shift outside the range and bStride < blockSize
    are refused and nothing is written; batch == 0 and blockSize == 0 succeed (the dot products store zeros)."""
    torch, lib = torch_gpu, dsp.lib
    rng = np.random.default_rng(79)
    for func in br.FUNCS:
        op, t = br.split(func)
        rt = br.result_type(func)
        dot = br.is_dot(func)
        a, b = Dev(torch, br.rand(t, 4 * 12, rng)), Dev(torch, br.rand(t, 4 * 12, rng))
        out = Dev(torch, br.marked(rt, 4 if dot else 4 * 12))
        scalars = br.rand_scalars(func, rng)
        name = "arm_" + func
        fb, fd = getattr(lib, name + "_batch"), getattr(lib, name)

        def batch_call(pa, pb, po, n=12, sc=scalars, batch=4, stride=None):
            srcs = [pa, pb] if br.two_sources(func) else [pa]
            if dot:
                return fb(*srcs, n if stride is None else stride, n, po, batch, None)
            return fb(*call_args(func, srcs, po, sc, n), batch, None)

        def void(pa, pb, po, fails, n=12, sc=scalars):
            srcs = [pa, pb] if br.two_sources(func) else [pa]
            fd(*call_args(func, srcs, po, sc, n))
            code, msg = dsp.last_error()
            assert (code != 0) == fails and (not fails or name in msg), (name, code, msg)
            lib.arm_mi355x_clear_error()

        # null pointers
        assert batch_call(None, b.ptr, out.ptr) == ARGUMENT_ERROR
        assert batch_call(a.ptr, b.ptr, None) == ARGUMENT_ERROR
        void(None, b.ptr, out.ptr, True)
        void(a.ptr, b.ptr, None, True)
        if br.two_sources(func):
            assert batch_call(a.ptr, None, out.ptr) == ARGUMENT_ERROR
            void(a.ptr, None, out.ptr, True)
        assert batch_call(a.ptr, b.ptr, out.ptr, batch=0) == SUCCESS
        # an output that overlaps a source without being it (not run to see what happens: refused before a launch)
        item = np.dtype(br.MDT[rt]).itemsize
        inside = a.ptr // item * item + item
        assert batch_call(a.ptr, b.ptr, inside) == ARGUMENT_ERROR
        void(a.ptr, b.ptr, inside, True)
        if br.two_sources(func):
            assert batch_call(a.ptr, b.ptr, b.ptr // item * item + item) == ARGUMENT_ERROR
        if dot:
            assert batch_call(a.ptr, b.ptr, a.ptr) == ARGUMENT_ERROR          # no exact alias for a result
            assert batch_call(a.ptr, b.ptr, out.ptr, stride=11) == ARGUMENT_ERROR
            assert batch_call(a.ptr, b.ptr, out.ptr, stride=1) == ARGUMENT_ERROR
        # shift counts: both out-of-range neighbours
        if func in br.SHIFT_RANGE:
            lo, hi = br.SHIFT_RANGE[func]
            for c in (lo - 1, hi + 1):
                sc = scalars[:-1] + (c,)
                assert batch_call(a.ptr, b.ptr, out.ptr, sc=sc) == ARGUMENT_ERROR, (func, c)
                void(a.ptr, b.ptr, out.ptr, True, sc=sc)
        lib.arm_mi355x_clear_error()
        torch.cuda.synchronize()
        assert out.get().tobytes() == br.marked(rt, out.n).tobytes(), func
        a.get(), b.get()
        # blockSize == 0
        assert batch_call(a.ptr, b.ptr, out.ptr, n=0, batch=3, stride=0) == SUCCESS
        void(a.ptr, b.ptr, out.ptr + (3 * item if dot else 0), False, n=0)
        torch.cuda.synchronize()
        if dot:
            assert out.get().tobytes() == bytes(4 * item), func
        else:
            assert out.get().tobytes() == br.marked(rt, out.n).tobytes(), func
    assert lib.arm_mi355x_last_error() == 0


# ------------------------------------------------------------------ GPU: the Python layers
@pytest.mark.gpu
def test_python_wrappers(dsp, torch_gpu):
    """cmsisdsp's names with the reference binding's argument order and return shapes, and cmsisdsp_amd's batched
    forms on tensors."""
    import cmsisdsp as d
    torch = torch_gpu
    for func in br.FUNCS:
        g = gold(func, "rand_65")
        got = getattr(d, "arm_" + func)(*[g[k] for k in ("a", "b") if k in g], *g["scalars"])
        if br.is_dot(func):
            assert isinstance(got, float if func.endswith("f32") else int), func
            assert br.MDT[br.result_type(func)](got) == g["value"], func
        else:
            assert isinstance(got, np.ndarray) and got.dtype == g["dst"].dtype, func
            check(func, "cmsisdsp", got, g["dst"])
    rng = np.random.default_rng(83)
    dev = lambda x: torch.from_numpy(x).cuda()                                   # noqa: E731
    for t in br.TYPES:
        a, b = br.rand(t, (6, 35), rng), br.rand(t, (6, 35), rng)
        ta, tb = dev(a), dev(b)
        calls = [("add", (ta, tb), ()), ("sub", (ta, tb), ()), ("mult", (ta, tb), ()), ("abs", (ta,), ()),
                 ("negate", (ta,), ()), ("offset", (ta,), br.rand_scalars(f"offset_{t}", rng)),
                 ("clip", (ta,), br.rand_scalars(f"clip_{t}", rng)), ("scale", (ta,), br.rand_scalars(f"scale_{t}", rng))]
        if t != "f32":
            calls += [("shift", (ta,), (2,))]
        for op, srcs, sc in calls:
            dst = dev(br.marked(t, (6, 35)))
            fn = getattr(dsp, op + "_batch")
            if op == "scale":
                fn(ta, sc[0], dst, *sc[1:])
            else:
                fn(*srcs, *sc, dst)
            want = br.run(f"{op}_{t}", a, b if len(srcs) == 2 else None, sc)["dst"]
            assert br.same_words(dst.cpu().numpy(), want, t == "f32"), (op, t)
        rt = br.DOT_OUT[t]
        res = dev(br.marked(rt, 6))
        dsp.dot_prod_batch(ta, tb, res)
        assert br.same_words(res.cpu().numpy(), br.run(f"dot_prod_{t}", a, b)["value"], t == "f32")
        res = dev(br.marked(rt, 6))
        dsp.dot_prod_batch(ta, tb[2], res)
        assert br.same_words(res.cpu().numpy(), br.run(f"dot_prod_{t}", a, b[2])["value"], t == "f32")
        with pytest.raises(RuntimeError):
            dsp.dot_prod_batch(ta, tb, res, b_stride=3)
        dsp.lib.arm_mi355x_clear_error()
    for t, width in (("u32", np.int32), ("u16", np.int16), ("u8", np.uint8)):
        a, b = br.rand(t, (5, 21), rng), br.rand(t, (5, 21), rng)
        ta, tb = dev(a.view(width)), dev(b.view(width))
        for op in ("and", "or", "xor", "not"):
            dst = dev(br.marked(t, (5, 21)).view(width))
            getattr(dsp, op + "_batch")(*((ta, tb) if op != "not" else (ta,)), dst)
            want = br.run(f"{op}_{t}", a, b)["dst"]
            assert dst.cpu().numpy().view(br.DT[t]).tobytes() == want.tobytes(), (op, t)
