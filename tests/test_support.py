"""The support functions: 12 conversions, arm_copy_* / arm_fill_* for f32 / q31 / q15 / q7, arm_sort_f32,
arm_merge_sort_f32, arm_weighted_average_f32, arm_barycenter_f32, each as a drop-in and as a _batch form
(cmsis-dsp_amd/csrc/support.hip, sort.hip; the weighted average is an operation of the chain kernels of statistics.hip).

The checker is committed data: tests/golden/support.npz holds the reference's own outputs between guard words
(tools/make_golden_support.py); tests/support_ref.py restates the functions in numpy, and the generator asserted it
against the reference case by case.  Every comparison is bit-exact; the f32 arithmetic (weighted average, barycenter,
q -> float) follows the rule of tests/test_f32_classes.py (non-NaN words bit-equal, NaNs at the same positions).  The
sorts are compared with the restatement's total order; the fixture says where the reference agrees with it.

CPU: the fixture index, the restatement against every fixture, the probed facts, the exported symbols, the Python
names, the struct layouts.  GPU: every function through its _batch form and its drop-in against every fixture;
batches of several items, every pointer in turn one element off 16-byte alignment, guard words after every device
buffer, lengths either side of a pack and a tile, dst == src where allowed, every refusal, fill of 0 and 1 words, the
sort's tier edges in both directions in place and out of place, every alg, the bitonic quirks, mixed zeros and NaNs,
the float inputs outside the conversion bounds, the f32 value classes, the weights strides."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import support_ref as sr
from cmsisdsp_amd import _abi
from f32_classes import CLASSES, f32_class_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "support.npz"))
_IDX = json.loads(str(GOLD["index"]))
INDEX = [(f, list(c)) for f, c in _IDX["cases"]]
CASES = dict(INDEX)
UNSORTED = [tuple(u) for u in _IDX["unsorted"]]
GUARD = 8                      # marker words after the end of every device buffer
SUCCESS, ARGUMENT_ERROR = 0, -1
BLOCK, UNROLL = 256, 4         # kBlock, kSpUnroll of support.hip: a tile is BLOCK * UNROLL units
WAVE_ITEMS = 4                 # items per workgroup of the one-wave sort tier
SUM_LANE_MIN_BATCH = 4096      # kSumLaneMinBatch of statistics.hip: from here on one lane per item
EW = sr.CONVERSIONS + sr.COPIES


def _type_name(a):
    return {np.dtype(v): k for k, v in sr.DT.items()}[np.asarray(a).dtype]


def unguard(buf):
    m = np.asarray(sr.MARK[_type_name(buf)]).tobytes()
    assert buf[:1].tobytes() == m and buf[-1:].tobytes() == m, "guard words"
    return buf[1:-1]


_LAYOUT = {}


def _layout(func):
    """Per recorded case: (operands, stored, offsets of a, b and the guarded output in the fixture's arrays)."""
    if func not in _LAYOUT:
        pos, table = {"a": 0, "b": 0, "dst": 0}, {}
        for case in CASES[func]:
            g = sr.operands(func, case)
            st = sr.is_stored(func, g)
            table[case] = (g, st, dict(pos))
            if st:
                for k in ("a", "b"):
                    if k in g:
                        pos[k] += g[k].size
                pos["dst"] += sr.out_len(func, g) + 2
        _LAYOUT[func] = table
    return _LAYOUT[func]


def gold(func, case):
    """The operands of one recorded case with the reference's output: "dst" (sorts: ascending, "dst0" descending;
    None for a case the fixture keeps as CRCs) or "value", and "dcrc"."""
    g, st, pos = _layout(func)[case]
    g = dict(g)
    k = CASES[func].index(case)
    if st:
        for key in ("a", "b"):
            if key in g:
                g[key] = GOLD[f"{func}/{key}"][pos[key]:pos[key] + g[key].size]
    assert sr.crc(g) == int(GOLD[f"{func}/crc"][k]), (func, case, "operands differ from the recorded ones")
    g["dcrc"] = GOLD[f"{func}/dcrc"][k]
    n = sr.out_len(func, g)
    if func == "weighted_average_f32":
        g["value"] = unguard(GOLD[f"{func}/value"][k])
        return g
    for key in ("dst", "dst0") if func in sr.SORTS else ("dst",):
        g[key] = unguard(GOLD[f"{func}/{key}"][pos["dst"]:pos["dst"] + n + 2]) if st else None
    return g


def expected(func, g, ascending=True):
    """The reference's output of a recorded case: the recorded words, or for a long case the restatement's after
    checking their CRC against the reference's."""
    key = "value" if func == "weighted_average_f32" else ("dst" if ascending else "dst0")
    crc = int(g["dcrc"][int(ascending)]) if func in sr.SORTS else int(g["dcrc"])
    if g[key] is not None:
        assert sr.out_crc(g[key]) == crc
        return g[key]
    want = sr.run(func, g, ascending)
    assert sr.out_crc(want) == crc, (func, "the restatement differs from the reference's output")
    return want


def check(func, what, got, want):
    g, w = np.asarray(got), np.asarray(want)
    assert sr.same_words(g.reshape(w.shape), w, sr.nan_rule(func)), (func, what, g.reshape(-1)[:8], w.reshape(-1)[:8])


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert len(sr.FUNCS) == 24 and len(set(sr.FUNCS)) == 24 and len(sr.CONVERSIONS) == 12
    assert [f for f, _ in INDEX] == list(sr.FUNCS)
    lengths = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257, 1023, 1025, 4097, 33000)
    assert sr.LENGTHS == lengths
    for f, cases in INDEX:
        want = [c for c in sr.case_names(f) if f not in sr.SORTS or sr.reference_sorts(c)]
        assert cases == want, f
        if f in EW + sr.FILLS:
            assert cases[:22] == [f"rand_{n}" for n in lengths], f
        if f in EW:
            assert "ext_64" in cases, f
        if f in sr.CONVERSIONS and f.startswith("float_"):
            assert {"trunc_33", "subnormal_9", "edge_16"} <= set(cases), f
    for f in sr.SORTS:
        assert {f"len_{n}" for n in range(1, 71)} <= set(CASES[f])
        assert {f"rand_{n}" for n in (255, 256, 257, 16383, 16384, 16385, 3 * 16384 + 5)} <= set(CASES[f])
        for kind in ("sorted", "reversed", "equal", "dups", "inf", "subnormal", "mixedzero"):
            assert f"{kind}_257" in CASES[f], (f, kind)
        assert not any(c.startswith("nan_") for c in CASES[f])          # never given to the reference
    sizes = (1, 2, 3, 5, 64, 65, 257)
    assert {f"v{a}_{b}" for a in sizes for b in sizes} | {"zerosum_5"} <= set(CASES["barycenter_f32"])
    assert {"empty_0", "zerosum_16"} <= set(CASES["weighted_average_f32"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "support.npz")) < 1 << 20


def test_restatement_equals_every_fixture():
    for f, cases in INDEX:
        for c in cases:
            g = gold(f, c)
            if f in sr.SORTS:
                for asc in (False, True):
                    got, want = sr.run(f, g, asc), expected(f, g, asc)
                    if sr.sort_exact(g):
                        assert got.tobytes() == want.tobytes(), (f, c, asc)
                    else:                                   # both signs of zero: equal values, equal multisets of words
                        assert np.array_equal(got, want), (f, c, asc)
                        assert np.array_equal(np.sort(got.view(np.uint32)), np.sort(want.view(np.uint32))), (f, c, asc)
            else:
                check(f, c, sr.run(f, g), expected(f, g))


def test_probed_facts_hold_in_the_fixtures():
    """The traps the issue lists, read off the reference's own outputs."""
    # the reference's sorts fail only as ARM_SORT_BITONIC with dir == 0 or a length that is no power of two
    assert UNSORTED and all(f == "sort_f32" and alg == 0 for f, _, alg, _ in UNSORTED)
    assert all(d == 0 or sr.case_n(c) & (sr.case_n(c) - 1) for _, c, _, d in UNSORTED)
    assert any(d == 0 and sr.case_n(c) & (sr.case_n(c) - 1) == 0 for _, c, _, d in UNSORTED)
    assert any(d == 1 for _, _, _, d in UNSORTED)
    # truncation toward zero: -0.7 / 2^k -> 0, 1.7 / 2^k -> 1, -1.7 / 2^k -> -1
    for d, bits in (("q31", 31), ("q15", 15), ("q7", 7)):
        g = gold(f"float_to_{d}", "ext_64")
        at = lambda v: int(g["dst"][np.flatnonzero(g["a"] == np.float32(v))[0]])      # noqa: E731
        assert at(-0.7 / 2 ** bits) == 0 and at(0.7 / 2 ** bits) == 0
        assert at(1.7 / 2 ** bits) == 1 and at(-1.7 / 2 ** bits) == -1
        i = np.iinfo(sr.DT[d])
        assert at(1.0) == i.max and at(-1.0) == i.min and at(2.0) == i.max and at(-2.0) == i.min
        assert at(2.0 ** -149) == 0 and int(g["dst"][3]) == 0          # a subnormal, -0.0
        assert at(np.nextafter(np.float32(sr.FLOAT_BOUND[d]), np.float32(0))) == i.max
    # q31_to_float rounds to nearest even above 2^24, and 0x7FFFFFFF gives 1.0f
    g = gold("q31_to_float", "ext_64")
    at = lambda v: g["dst"][np.flatnonzero(g["a"] == v)[0]]                          # noqa: E731
    assert at(0x7FFFFFFF) == np.float32(1.0) and at(-0x7FFFFFFF) == np.float32(-1.0)
    assert at(0x01000001) == np.float32(2.0 ** -7) and at(0x01000003) == np.float32((2 ** 24 + 4) / 2.0 ** 31)
    assert at(0x7FFFFF40) == np.float32((2 ** 31 - 256) / 2.0 ** 31)               # a tie: to even
    # the empty weighted average is 0 / 0
    assert np.isnan(gold("weighted_average_f32", "empty_0")["value"]).all()
    assert not np.isfinite(gold("weighted_average_f32", "zerosum_16")["value"]).any()
    assert not np.isfinite(gold("barycenter_f32", "zerosum_5")["dst"]).any()


def test_contract_and_order_of_the_restatement():
    for d in ("q31", "q15", "q7"):
        b = np.float32(sr.FLOAT_BOUND[d])
        assert sr.in_contract(f"float_to_{d}", {"a": np.array([np.nextafter(b, np.float32(0))], dtype=np.float32)})
        assert not sr.in_contract(f"float_to_{d}", {"a": np.array([b], dtype=np.float32)})
        assert not sr.in_contract(f"float_to_{d}", {"a": np.array([np.nan], dtype=np.float32)})
        i = np.iinfo(sr.DT[d])
        got = sr.float_to_q(sr.out_of_contract_input(), d).tolist()
        assert got[:11] == [i.max, i.min, 0, 0, i.max, i.min, i.max, i.min, i.max, i.min, i.max]
    words = np.array([0x7FC00000, 0x7F800000, 0x3F800000, 1, 0, 0x80000000, 0x80000001, 0xBF800000, 0xFF800000,
                      0xFF800001, 0xFFFFFFFF], dtype=np.uint32)
    rng = np.random.default_rng(5)
    got = sr.total_order_sort(rng.permutation(words).view(np.float32), False).view(np.uint32)
    assert got.tolist() == words.tolist()
    assert sr.total_order_sort(words.view(np.float32)).view(np.uint32).tolist() == words[::-1].tolist()


def test_library_exports_the_symbols(dsp):
    names = [f"arm_{f}{suffix}" for f in sr.FUNCS for suffix in ("", "_batch")] + ["arm_sort_init_f32",
                                                                                  "arm_merge_sort_init_f32"]
    assert len(set(names)) == 50 and set(names) == set(_abi.SUPPORT)
    out = subprocess.run(["nm", "-D", "--defined-only", dsp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(names) <= exported
    support = {s for s in exported if s.startswith(("arm_copy_", "arm_fill_", "arm_sort_", "arm_merge_sort_",
                                                    "arm_weighted_average_", "arm_barycenter_"))
               or ("_to_" in s and s.startswith(("arm_float_", "arm_q31_to", "arm_q15_to", "arm_q7_to")))}
    assert support == set(names)
    for header, suffix in (("arm_math.h", ""), ("arm_math_mi355x.h", "_batch")):
        text = open(os.path.join(ROOT, "include", header)).read()
        for n in ("arm_sort_f32", "arm_merge_sort_f32", "arm_weighted_average_f32", "arm_barycenter_f32"):
            assert f"{n}{suffix}(" in text, (header, n)
        for n in ("arm_##SN##_to_##DN", "arm_copy_##SUF", "arm_fill_##SUF"):
            assert n + ("##" + suffix if suffix else "") + "(" in text, (header, n)


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for f in sr.FUNCS:
        if f != "merge_sort_f32":                           # the reference's wrapper has no merge sort
            fn = getattr(d, "arm_" + f)
            assert callable(fn) and "cmsis_arm_" + f in fn.__doc__, f
    assert callable(d.arm_sort_init_f32)
    S = d.arm_sort_instance_f32(alg=4, dir=1)
    assert (S.alg(), S.dir()) == (4, 1)
    d.arm_sort_init_f32(S, 2, 0)
    assert (S.alg(), S.dir()) == (2, 0)
    for n in ("arm_copy_f64", "arm_fill_f64", "arm_div_int64_to_int32"):      # left out
        assert not hasattr(d, n), n
    for n in ("arm_convert", "arm_fill", "arm_sort_f32", "arm_merge_sort_f32", "arm_weighted_average_f32",
              "arm_barycenter_f32", "convert_batch", "copy_batch", "fill_batch", "sort_batch", "weighted_average_batch",
              "barycenter_batch", "arm_sort_init_f32", "arm_merge_sort_init_f32"):
        assert callable(getattr(dsp, n)), n


def test_struct_layout_matches_reference(tmp_path):
    """tools/abi_layout_support.c compiled against include/ prints what it printed when compiled against the
    reference's headers (tests/golden/abi_layout_support.json); the ctypes mirrors agree."""
    exe = str(tmp_path / "abi_layout_support")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "abi_layout_support.c"),
                    "-o", exe], check=True)
    ours = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_layout_support.json")))
    assert ours == ref and len(ref) == 4
    for name in ("arm_sort_instance_f32", "arm_merge_sort_instance_f32"):
        st, lay = getattr(_abi, name), ref[name]
        assert C.sizeof(st) == lay["size"], name
        assert {f for f, _ in st._fields_} == set(lay) - {"size"}, name
        for fname, _ in st._fields_:
            assert getattr(st, fname).offset == lay[fname], (name, fname)
    assert ref["arm_sort_alg"]["size"] == ref["arm_sort_dir"]["size"] == C.sizeof(C.c_int)


# ------------------------------------------------------------------ GPU helpers
class Dev:
    """A device copy of x whose first word sits `off` elements into a marker-filled allocation (which is 16-byte
    aligned), GUARD marker words after its end."""

    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.t = _type_name(x)
        self.off, self.n, self.shape, self.dtype = off, x.size, x.shape, x.dtype
        raw = sr.marked(self.t, off + x.size + GUARD)
        raw[off:off + x.size] = x.reshape(-1)
        self.buf = torch.from_numpy(raw.view(np.uint8)).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + off * x.itemsize

    def get(self):
        b = self.buf.cpu().numpy().view(self.dtype)
        m = sr.marked(self.t, 1).tobytes()
        assert b[:self.off].tobytes() == m * self.off and b[self.off + self.n:].tobytes() == m * GUARD, "guard words"
        return b[self.off:self.off + self.n].reshape(self.shape)


class Host:
    def __init__(self, x, off=0):
        self.a = np.ascontiguousarray(x).copy()
        self.ptr = self.a.ctypes.data

    def get(self):
        return self.a


def sort_instance(func, dirv, alg=4, buffer=None):
    if func == "sort_f32":
        return _abi.arm_sort_instance_f32(alg, dirv)
    return _abi.arm_merge_sort_instance_f32(dirv, buffer)


def run_on(dsp, torch, func, g, where, offs=(0, 0, 0), batch=None, dirv=1, alg=4, w_stride=None, alias=False):
    """arm_<func> (batch None: one item on host arrays or device buffers) or arm_<func>_batch on device buffers whose
    a, b and output start offs elements into their allocations, the output pre-filled with the marker.  g["a"] /
    g["b"]: the operands as the call sees them ([batch, ...] for a batch).  alias: the output is the source's buffer.
    -> (status, the output words)."""
    put = Host if where == "host" else (lambda x, off=0: Dev(torch, x, off))
    s, d = sr.types(func)
    items = 1 if batch is None else batch
    src = {k: put(np.asarray(g[k]), offs[i]) for i, k in enumerate(("a", "b")) if k in g}
    tail = [] if batch is None else [batch, None]
    fn = getattr(dsp.lib, f"arm_{func}" + ("" if batch is None else "_batch"))
    if func in sr.FILLS:
        value, n = g["scalars"]
        out = put(sr.marked(d, (items, n)), offs[2])
        st = fn(value, out.ptr, n, *tail)
    elif func in sr.SORTS:
        n = np.shape(g["a"])[-1]
        out = src["a"] if alias else put(sr.marked(d, np.shape(g["a"])), offs[2])
        if batch is None:
            S = sort_instance(func, dirv, alg)
            st = fn(C.byref(S), src["a"].ptr, out.ptr, n)
        else:
            st = fn(src["a"].ptr, out.ptr, n, dirv, *tail)
    elif func == "weighted_average_f32":
        n = np.shape(g["a"])[-1]
        if batch is None:
            out = Host(np.array([fn(src["a"].ptr, src["b"].ptr, n)], dtype=np.float32))
            st = None
        else:
            out = put(sr.marked(d, items), offs[2])
            st = fn(src["a"].ptr, src["b"].ptr, n if w_stride is None else w_stride, n, out.ptr, *tail)
    elif func == "barycenter_f32":
        nv, dim = g["scalars"]
        out = put(sr.marked(d, (items, dim)), offs[2])
        if batch is None:
            st = fn(src["a"].ptr, src["b"].ptr, out.ptr, nv, dim)
        else:
            st = fn(src["a"].ptr, src["b"].ptr, nv if w_stride is None else w_stride, out.ptr, nv, dim, *tail)
    else:
        n = np.shape(g["a"])[-1]
        out = src["a"] if alias else put(sr.marked(d, np.shape(g["a"])), offs[2])
        st = fn(src["a"].ptr, out.ptr, n, *tail)
    if where != "host":
        torch.cuda.synchronize()
    got = out.get()
    if alias and func in sr.CONVERSIONS:                    # equal widths: the source's buffer read as the output type
        got = got.view(sr.DT[d])
    for k, v in src.items():
        if not (alias and k == "a"):
            assert v.get().tobytes() == np.ascontiguousarray(g[k]).tobytes(), (func, k, "a source changed")
    assert dsp.last_error()[0] == 0 or st not in (None, SUCCESS), (func, dsp.last_error())
    return (0 if st is None else st), got


def rand_source(func, shape, rng):
    s, _ = sr.types(func)
    if s == "f32":
        return rng.uniform(-1.25, 1.25, shape).astype(np.float32)
    return sr.bm.rand(s, shape, rng)


# ------------------------------------------------------------------ GPU: every function against the fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("func", sr.FUNCS)
def test_batch_form_and_dropin_equal_fixtures(dsp, torch_gpu, func):
    """Every recorded case through the _batch form on device pointers (one item) and through the drop-in on host
    pointers; the sorts in both directions."""
    for case in CASES[func]:
        g = gold(func, case)
        for asc in ((False, True) if func in sr.SORTS else (True,)):
            want = np.asarray(expected(func, g, asc)) if func not in sr.SORTS or sr.sort_exact(g) else \
                sr.run(func, g, asc)
            for where, batch in (("dev", 1), ("host", None)):
                st, got = run_on(dsp, torch_gpu, func, g, where, batch=batch, dirv=int(asc))
                assert st == SUCCESS, (func, case, where)
                check(func, (case, where, asc), got.reshape(-1), want.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("func", EW)
def test_conversion_lengths_offsets_and_batches(dsp, torch_gpu, func):
    """Lengths either side of one pack and one tile of the narrower type, each pointer in turn one element off 16-byte
    alignment (the one-element-per-lane path), as one item and as a batch of three."""
    s, d = sr.types(func)
    v = 16 // min(np.dtype(sr.DT[s]).itemsize, np.dtype(sr.DT[d]).itemsize)
    tile = BLOCK * UNROLL * v
    rng = np.random.default_rng(11)
    for n in (v - 1, v, v + 1, tile - 1, tile, tile + 1):
        a = rand_source(func, n, rng)
        want = sr.convert(s, d, a)
        for offs in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)):
            st, got = run_on(dsp, torch_gpu, func, {"a": a}, "dev", offs=offs, batch=1)
            assert st == SUCCESS
            check(func, (n, offs), got, want)
    a = rand_source(func, (3, 2 * v + 3), rng)
    for where_off in ((0, 0, 0), (0, 0, 1)):
        st, got = run_on(dsp, torch_gpu, func, {"a": a}, "dev", offs=where_off, batch=3)
        assert st == SUCCESS
        check(func, "batch 3", got, sr.convert(s, d, a))
    st, got = run_on(dsp, torch_gpu, func, {"a": a[0]}, "dev", batch=None)       # the drop-in on device pointers
    check(func, "drop-in, device", got, sr.convert(s, d, a[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("func", sr.FILLS)
def test_fill_lengths_offsets_and_batches(dsp, torch_gpu, func):
    d = sr.types(func)[1]
    v = 16 // np.dtype(sr.DT[d]).itemsize
    value = sr.DT[d](-3).item()
    for n in (0, 1, v - 1, v + 1, BLOCK * UNROLL * v + 1):
        for off in (0, 1):
            for batch in (1, 3):
                st, got = run_on(dsp, torch_gpu, func, {"scalars": (value, n)}, "dev", offs=(0, 0, off), batch=batch)
                assert st == SUCCESS and got.shape == (batch, n) and (got == value).all(), (n, off, batch)
    for n in (0, 1):
        st, got = run_on(dsp, torch_gpu, func, {"scalars": (value, n)}, "host")
        assert st == SUCCESS and (got == value).all()


@pytest.mark.gpu
def test_aliasing_and_refusals(dsp, torch_gpu):
    """dst == src exactly where both element widths are equal; every other overlap, a null pointer, an unknown dir
    and a weights stride below the weight count are refused, and nothing is written."""
    rng = np.random.default_rng(3)
    lib = dsp.lib
    for func in EW:
        s, d = sr.types(func)
        a = rand_source(func, 70, rng)
        same = np.dtype(sr.DT[s]).itemsize == np.dtype(sr.DT[d]).itemsize
        if same:
            st, got = run_on(dsp, torch_gpu, func, {"a": a}, "dev", batch=1, alias=True)
            assert st == SUCCESS
            check(func, "in place", got, sr.convert(s, d, a))
            st, got = run_on(dsp, torch_gpu, func, {"a": a}, "dev", offs=(1, 0, 0), batch=1, alias=True)
            check(func, "in place, off alignment", got, sr.convert(s, d, a))
        src = Dev(torch_gpu, a)
        big = Dev(torch_gpu, np.zeros(4 * 80, dtype=np.uint8).view(sr.DT[d])[:80])
        fn = getattr(lib, f"arm_{func}_batch")
        if not same:                                        # the same address, different widths
            assert fn(src.ptr, src.ptr, 70, 1, None) == ARGUMENT_ERROR, func
        isz, osz = a.itemsize, np.dtype(sr.DT[d]).itemsize
        assert fn(src.ptr, src.ptr + osz, 60, 1, None) == ARGUMENT_ERROR, func          # shifted by one word
        assert fn(src.ptr + isz, src.ptr, 60, 1, None) == ARGUMENT_ERROR, func
        assert fn(None, big.ptr, 70, 1, None) == ARGUMENT_ERROR and fn(src.ptr, None, 70, 1, None) == ARGUMENT_ERROR
        assert fn(src.ptr, big.ptr, 70, 0, None) == SUCCESS and fn(src.ptr, big.ptr, 0, 1, None) == SUCCESS
        torch_gpu.cuda.synchronize()
        assert src.get().tobytes() == a.tobytes() and not big.get().view(np.uint8).any(), func
        dsp.lib.arm_mi355x_clear_error()
        getattr(lib, f"arm_{func}")(None, big.ptr, 70)      # the void drop-in reports through the last error
        assert dsp.last_error()[0] != 0, func
        dsp.lib.arm_mi355x_clear_error()
    for func in sr.FILLS:
        assert getattr(lib, f"arm_{func}_batch")(0, None, 4, 1, None) == ARGUMENT_ERROR
    x = Dev(torch_gpu, rng.uniform(-1, 1, 300).astype(np.float32))
    y = Dev(torch_gpu, sr.marked("f32", 300))
    for name in ("arm_sort_f32_batch", "arm_merge_sort_f32_batch"):
        fn = getattr(lib, name)
        assert fn(x.ptr, y.ptr, 100, 2, 3, None) == ARGUMENT_ERROR          # dir
        assert fn(x.ptr, y.ptr, 100, -1, 3, None) == ARGUMENT_ERROR
        assert fn(x.ptr, x.ptr + 4, 100, 1, 2, None) == ARGUMENT_ERROR      # overlap
        assert fn(None, y.ptr, 100, 1, 3, None) == ARGUMENT_ERROR and fn(x.ptr, None, 100, 1, 3, None) == ARGUMENT_ERROR
        assert fn(x.ptr, y.ptr, 100, 1, 0, None) == SUCCESS and fn(x.ptr, y.ptr, 0, 1, 3, None) == SUCCESS
    r = Dev(torch_gpu, sr.marked("f32", 3))
    wa, ba = lib.arm_weighted_average_f32_batch, lib.arm_barycenter_f32_batch
    assert wa(x.ptr, x.ptr, 99, 100, r.ptr, 3, None) == ARGUMENT_ERROR      # stride below the length
    assert wa(x.ptr, x.ptr, 100, 100, x.ptr + 8, 3, None) == ARGUMENT_ERROR  # the result inside a source
    assert wa(None, x.ptr, 100, 100, r.ptr, 3, None) == ARGUMENT_ERROR
    assert wa(x.ptr, None, 100, 100, r.ptr, 3, None) == ARGUMENT_ERROR
    assert wa(x.ptr, x.ptr, 100, 100, None, 3, None) == ARGUMENT_ERROR
    assert ba(x.ptr, x.ptr, 9, y.ptr, 10, 10, 3, None) == ARGUMENT_ERROR     # stride below nbVectors
    assert ba(x.ptr, y.ptr, 0, x.ptr + 40, 10, 10, 3, None) == ARGUMENT_ERROR   # out inside in
    assert ba(None, x.ptr, 0, y.ptr, 10, 10, 3, None) == ARGUMENT_ERROR
    assert ba(x.ptr, x.ptr, 0, None, 10, 10, 3, None) == ARGUMENT_ERROR
    torch_gpu.cuda.synchronize()
    assert (y.get().view(np.uint32) == 0x5A5A5A5A).all() and (r.get().view(np.uint32) == 0x5A5A5A5A).all()
    dsp.lib.arm_mi355x_clear_error()


# ------------------------------------------------------------------ GPU: the sorts
SORT_LENGTHS = (63, 64, 65, 127, 129, sr.SORT_WAVE_MAX - 1, sr.SORT_WAVE_MAX, sr.SORT_WAVE_MAX + 1, 511, 513,
                sr.SORT_LDS_MAX - 1, sr.SORT_LDS_MAX, sr.SORT_LDS_MAX + 1, 3 * sr.SORT_LDS_MAX + 5)


def _sort_input(n, items, rng):
    a = rng.uniform(-1.0, 1.0, (items, n)).astype(np.float32)
    a[:, ::7] = np.float32(0.25)                            # duplicates
    a[0, :3] = [np.inf, -np.inf, -0.0][:min(3, n)]
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("n", SORT_LENGTHS)
def test_sort_tier_edges(dsp, torch_gpu, n):
    """Either side of the one-wave limit and of kSortLdsMax, and 3 * kSortLdsMax + 5 (global passes with a ragged
    end): both directions, in place and out of place, a batch that is no multiple of the items per workgroup, a
    source off 16-byte alignment; the source is unchanged out of place (run_on checks it)."""
    rng = np.random.default_rng(n)
    items = WAVE_ITEMS + 1 if n <= sr.SORT_LDS_MAX + 1 else 2
    a = _sort_input(n, items, rng)
    for func in sr.SORTS:
        for dirv in (0, 1):
            want = sr.total_order_sort(a, dirv == 1)
            for alias, offs in ((False, (0, 0, 0)), (True, (0, 0, 0)), (False, (1, 0, 3))):
                if func == "merge_sort_f32" and offs[0]:
                    continue
                st, got = run_on(dsp, torch_gpu, func, {"a": a}, "dev", offs=offs, batch=items, dirv=dirv, alias=alias)
                assert st == SUCCESS and got.tobytes() == want.tobytes(), (func, n, dirv, alias, offs)
    st, got = run_on(dsp, torch_gpu, "sort_f32", {"a": a[0]}, "host", dirv=0)
    assert got.tobytes() == sr.total_order_sort(a[0], False).tobytes()


@pytest.mark.gpu
def test_sort_instance_fields(dsp, torch_gpu):
    """Every alg gives the same words, also where the reference's bitonic sort does not sort (no power of two;
    dir 0); an unknown alg is a no-op; arm_merge_sort_f32 leaves S->buffer alone; in place on host pointers."""
    lib = dsp.lib
    odd = next(u for u in UNSORTED if u[3] == 1)                                   # not a power of two
    assert sr.case_n(odd[1]) & (sr.case_n(odd[1]) - 1)
    pow2 = next(u for u in UNSORTED if u[3] == 0 and sr.case_n(u[1]) & (sr.case_n(u[1]) - 1) == 0)
    for g, dirs in ((gold("sort_f32", odd[1]), (0, 1)), (gold("sort_f32", pow2[1]), (0,)),
                    (gold("sort_f32", "dups_257"), (0, 1))):
        for d in dirs:
            want = sr.total_order_sort(g["a"], d == 1)
            for alg in range(6):
                st, got = run_on(dsp, torch_gpu, "sort_f32", g, "host", dirv=d, alg=alg)
                assert got.tobytes() == want.tobytes(), (alg, d)
    a = gold("sort_f32", "dups_257")["a"].copy()
    for alg in (6, -1, 1000):
        st, got = run_on(dsp, torch_gpu, "sort_f32", {"a": a}, "host", alg=alg)
        assert (got.view(np.uint32) == 0x5A5A5A5A).all(), alg
    work = sr.marked("f32", a.size + 2)
    S = _abi.arm_merge_sort_instance_f32()
    lib.arm_merge_sort_init_f32(C.byref(S), 1, work.ctypes.data + 4)
    assert S.dir == 1 and S.buffer == work.ctypes.data + 4
    x = a.copy()
    lib.arm_merge_sort_f32(C.byref(S), x.ctypes.data, x.ctypes.data, x.size)        # in place
    assert x.tobytes() == sr.total_order_sort(a).tobytes()
    assert (work.view(np.uint32) == 0x5A5A5A5A).all()
    S2 = _abi.arm_sort_instance_f32()
    lib.arm_sort_init_f32(C.byref(S2), 3, 0)
    assert (S2.alg, S2.dir) == (3, 0)
    y = a.copy()
    lib.arm_sort_f32(C.byref(S2), y.ctypes.data, y.ctypes.data, y.size)
    assert y.tobytes() == sr.total_order_sort(a, False).tobytes() and dsp.last_error()[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixedzero", "nan"])
def test_sort_total_order_of_zeros_and_nans(dsp, torch_gpu, kind):
    for func in sr.SORTS:
        for n in (5, 64, 257, 1025):
            g = sr.operands(func, f"{kind}_{n}")
            for dirv in (0, 1):
                want = sr.total_order_sort(g["a"], dirv == 1)
                st, got = run_on(dsp, torch_gpu, func, g, "dev", batch=1, dirv=dirv)
                assert st == SUCCESS and got.reshape(-1).tobytes() == want.tobytes(), (func, n, dirv)
    if kind == "mixedzero":
        st, got = run_on(dsp, torch_gpu, "sort_f32", {"a": np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32)}, "host")
        assert got.view(np.uint32).tolist() == [0x80000000, 0x80000000, 0, 0]


# ------------------------------------------------------------------ GPU: float inputs, f32 classes
@pytest.mark.gpu
@pytest.mark.parametrize("d", ["q31", "q15", "q7"])
def test_float_inputs_outside_the_bounds_saturate(dsp, torch_gpu, d):
    """+-Inf, NaN, +-2^40 and the bound itself: saturation by sign, NaN -> 0 (the restatement's rule)."""
    a = sr.out_of_contract_input()
    func = f"float_to_{d}"
    assert not sr.in_contract(func, {"a": a})
    want = sr.float_to_q(a, d)
    for where, batch in (("dev", 1), ("host", None)):
        st, got = run_on(dsp, torch_gpu, func, {"a": a}, where, batch=batch)
        assert got.reshape(-1).tobytes() == want.tobytes(), (where, got, want)
    big = np.tile(a, 40)                                    # the 16-byte path
    st, got = run_on(dsp, torch_gpu, func, {"a": big}, "dev", batch=1)
    assert got.reshape(-1).tobytes() == sr.float_to_q(big, d).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
def test_f32_value_classes(dsp, torch_gpu, cls):
    """Subnormals, signed zeros, words near overflow, infinities and NaNs through every function with f32 operands
    (float -> q against the restatement, which holds our rule outside the reference's bounds)."""
    n = 67
    x = f32_class_input(cls, (3, n), 21, scale=3.0e38, positions=(1, n + 5, 3 * n - 1))
    w = f32_class_input(cls, (3, n), 22, scale=1.0e38, positions=(2, n + 6, 3 * n - 2))
    for d in ("q31", "q15", "q7"):
        st, got = run_on(dsp, torch_gpu, f"float_to_{d}", {"a": x}, "dev", batch=3)
        assert got.tobytes() == sr.float_to_q(x, d).tobytes(), d
    st, got = run_on(dsp, torch_gpu, "copy_f32", {"a": x}, "dev", batch=3)
    assert got.tobytes() == x.tobytes()
    for dirv in (0, 1):
        st, got = run_on(dsp, torch_gpu, "sort_f32", {"a": x}, "dev", batch=3, dirv=dirv)
        assert got.tobytes() == sr.total_order_sort(x, dirv == 1).tobytes()
    st, got = run_on(dsp, torch_gpu, "weighted_average_f32", {"a": x, "b": w}, "dev", batch=3)
    check("weighted_average_f32", cls, got, sr.weighted_average(x, w))
    st, got = run_on(dsp, torch_gpu, "barycenter_f32", {"a": x.reshape(1, 3, n), "b": w[:1, :3], "scalars": (3, n)},
                     "dev", batch=1)
    check("barycenter_f32", cls, got, sr.barycenter(x.reshape(1, 3, n), w[:1, :3]))


# ------------------------------------------------------------------ GPU: weighted average, barycenter
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 5, SUM_LANE_MIN_BATCH - 1, SUM_LANE_MIN_BATCH + 3])
def test_weighted_average_batches_and_strides(dsp, torch_gpu, batch):
    """Both chain kernels (one wave per item below kSumLaneMinBatch items, one lane per item from there on) with
    the weights stride 0, == n and > n, the operands off 16-byte alignment."""
    rng = np.random.default_rng(batch)
    for n in (1, 33, 64, 130):
        a = rng.uniform(-1.0, 1.0, (batch, n)).astype(np.float32)
        for stride in (0, n, n + 3):
            w = rng.uniform(0.0, 1.0, (batch, max(stride, n)) if stride else (1, n)).astype(np.float32)
            want = sr.weighted_average(a, w[:, :n])
            offs = (1, 0, 0) if stride == n else (0, 1, 1)
            st, got = run_on(dsp, torch_gpu, "weighted_average_f32", {"a": a, "b": w}, "dev", offs=offs, batch=batch,
                             w_stride=stride)
            assert st == SUCCESS
            check("weighted_average_f32", (batch, n, stride), got, want)


@pytest.mark.gpu
def test_barycenter_batches_and_strides(dsp, torch_gpu):
    rng = np.random.default_rng(8)
    for batch, nv, dim in ((1, 5, 3), (3, 4, 65), (7, 64, 5), (2, 3, 257), (300, 2, 3)):
        a = rng.uniform(-1.0, 1.0, (batch, nv, dim)).astype(np.float32)
        for stride in (0, nv, nv + 2):
            w = rng.uniform(0.1, 1.0, (batch, max(stride, nv)) if stride else (1, nv)).astype(np.float32)
            want = sr.barycenter(a, w[:, :nv])
            for offs in ((0, 0, 0), (1, 1, 1)):
                st, got = run_on(dsp, torch_gpu, "barycenter_f32", {"a": a, "b": w, "scalars": (nv, dim)}, "dev",
                                 offs=offs, batch=batch, w_stride=stride)
                assert st == SUCCESS
                check("barycenter_f32", (batch, nv, dim, stride), got, want)
    a = rng.uniform(-1.0, 1.0, (4, 6)).astype(np.float32)                       # the drop-in on device pointers
    w = rng.uniform(0.1, 1.0, 4).astype(np.float32)
    st, got = run_on(dsp, torch_gpu, "barycenter_f32", {"a": a, "b": w, "scalars": (4, 6)}, "dev")
    check("barycenter_f32", "drop-in, device", got.reshape(-1), sr.barycenter(a[None], w[None])[0])


@pytest.mark.gpu
def test_python_wrappers(dsp, torch_gpu):
    """The numpy drop-ins of cmsisdsp and the tensor forms of cmsisdsp_amd."""
    import cmsisdsp as d
    torch = torch_gpu
    rng = np.random.default_rng(2)
    x = rng.uniform(-1.0, 1.0, 300).astype(np.float32)
    q15 = sr.float_to_q(x, "q15")
    assert d.arm_float_to_q15(x).tobytes() == q15.tobytes()
    assert d.arm_q15_to_float(q15).tobytes() == sr.convert("q15", "f32", q15).tobytes()
    assert d.arm_copy_q7(np.arange(-5, 5)).tolist() == list(range(-5, 5))
    assert d.arm_fill_q31(7, 5).tolist() == [7] * 5 and d.arm_fill_f32(0.5, 3).dtype == np.float32
    S = d.arm_sort_instance_f32(alg=0, dir=0)
    assert d.arm_sort_f32(S, x).tobytes() == sr.total_order_sort(x, False).tobytes()
    w = rng.uniform(0.1, 1.0, 300).astype(np.float32)
    assert np.float32(d.arm_weighted_average_f32(x, w)).tobytes() == sr.weighted_average(x[None], w[None]).tobytes()
    assert d.arm_barycenter_f32(x, w[:3], 3, 100).tobytes() == sr.barycenter(x.reshape(1, 3, 100), w[None, :3]).tobytes()
    t = torch.from_numpy(x.reshape(3, 100)).cuda()
    q = torch.zeros((3, 100), dtype=torch.int16, device="cuda")
    dsp.convert_batch(t, q)
    out = torch.empty_like(t)
    dsp.sort_batch(t, out, dsp.ARM_SORT_DESCENDING)
    f = torch.empty_like(t)
    dsp.fill_batch(1.5, f)
    c = torch.empty_like(t)
    dsp.copy_batch(t, c)
    r = torch.empty(3, dtype=torch.float32, device="cuda")
    dsp.weighted_average_batch(t, torch.from_numpy(w[:100]).cuda(), r)
    b = torch.empty((1, 100), dtype=torch.float32, device="cuda")
    dsp.barycenter_batch(t.reshape(1, 3, 100), torch.from_numpy(w[:3]).cuda(), b)
    torch.cuda.synchronize()
    assert q.cpu().numpy().tobytes() == q15.tobytes()
    assert out.cpu().numpy().tobytes() == sr.total_order_sort(x.reshape(3, 100), False).tobytes()
    assert (f.cpu().numpy() == 1.5).all() and c.cpu().numpy().tobytes() == x.tobytes()
    assert r.cpu().numpy().tobytes() == sr.weighted_average(x.reshape(3, 100), w[:100]).tobytes()
    assert b.cpu().numpy().tobytes() == sr.barycenter(x.reshape(1, 3, 100), w[None, :3]).tobytes()
