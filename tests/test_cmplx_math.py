"""arm_cmplx_{mag,mag_squared,conj,mult_cmplx,mult_real,dot_prod}_{f32,q31,q15} and arm_{max,min}_{f32,q31,q15,q7}:
the 26 drop-ins and their _batch forms (cmsis-dsp_amd/csrc/cmplx_math.hip).

The checker is committed data: tests/golden/cmplx_math.npz holds the reference's own outputs, every output buffer
pre-filled with a marker word (tools/make_golden_cmplx_math.py); tests/cmplx_math_ref.py restates the 26 functions
in numpy, and the generator asserted it against the reference case by case.  Every comparison is bit-exact; f32
cases with NaN follow the rule of tests/test_f32_classes.py (non-NaN words bit-equal, NaNs at the same positions).

CPU: the fixture index, the restatement against every fixture, the probed facts, the 52 exported symbols, the
Python names.  GPU: the drop-ins on host and device pointers against every fixture, the in-place aliases and the
refused overlap, the status cases, and the shapes at which the kernels change path: the 16-B / scalar split of
the element-wise kernel, the lanes-per-item steps of the reductions (1 .. 64 lanes, then the whole workgroup past
REDUCE_WAVE_MAX loads), the two dot_prod_f32 kernels (one wave per item below DOT_LANE_MIN_BATCH items, one lane
per item with DOT_CHUNK-sample LDS stages from there on)."""
import json
import os

import numpy as np
import pytest

import cmplx_math_ref as cm
from cmsisdsp_amd import _abi
from f32_classes import assert_same_words, f32_class_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cmplx_math.npz"))
INDEX = [tuple(x) for x in json.loads(str(GOLD["index"]))]
EW_OPS = ("mag", "mag_squared", "conj", "mult_cmplx", "mult_real")
EW = [f"cmplx_{op}_{t}" for op in EW_OPS for t in cm.CTYPES]
DOT = [f"cmplx_dot_prod_{t}" for t in cm.CTYPES]
SEARCH = [f"{op}_{t}" for op in ("max", "min") for t in ("f32", "q31", "q15", "q7")]
GUARD = 8                      # marker words after the end of every device buffer
SUCCESS, ARGUMENT_ERROR = 0, -1
# the constants of cmplx_math.hip that decide a kernel's path
REDUCE_WAVE_MAX = 512          # kRedWaveMax: loads (16-B packs when aligned, else words) a wave takes per item
DOT_LANE_MIN_BATCH = 4096      # kDotLaneMinBatch
DOT_CHUNK = 8                  # kDotChunk


def gold(func, case):
    pre = f"{func}/{case}/"
    return {k[len(pre):]: GOLD[k] for k in GOLD.files if k.startswith(pre)}


def out_names(func):
    op = cm.split(func)[0]
    return ("re", "im") if op == "dot_prod" else ("value", "index") if op in ("max", "min") else ("dst",)


def check(func, case, got, want):
    for k in out_names(func):
        assert cm.same_words(np.asarray(got[k]).reshape(np.shape(want[k])), np.asarray(want[k]), cm.nan_rule(case)), \
            (func, case, k, got[k], want[k])


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert len(cm.FUNCS) == 26 and len(set(cm.FUNCS)) == 26
    assert INDEX == [(f, c) for f in cm.FUNCS for c in cm.case_names(f)]
    for f, c in INDEX:
        g = gold(f, c)
        assert set(cm.out_spec(f, g)) <= set(g), (f, c)
    for f in cm.FUNCS:
        names = cm.case_names(f)
        assert [f"rand_{n}" for n in (1, 3, 4, 5, 8, 67)] == names[:6]


def test_restatement_equals_every_fixture():
    for f, c in INDEX:
        g = gold(f, c)
        check(f, c, cm.run(f, g), g)


def test_probed_facts_hold_in_the_fixtures():
    """A NaN input to mag_f32 gives +0.0; conj maps the minimum to the maximum; a NaN at 0 gives index 0; and the
    other facts the issue pins."""
    g = gold("cmplx_mag_f32", "nonfinite_8")
    nan_at = np.flatnonzero(np.isnan(g["a"]))
    assert nan_at.size == 1
    assert g["dst"].view(np.uint32)[nan_at[0] // 2] == 0                       # +0.0, not NaN
    assert np.isposinf(g["dst"][np.flatnonzero(np.isinf(g["a"])) // 2]).all()
    g = gold("cmplx_mag_f32", "overflow_8")
    assert np.isposinf(g["dst"]).any() and np.isfinite(g["a"]).all()
    for t in ("q31", "q15"):
        i = np.iinfo(cm.DT[t])
        d = gold(f"cmplx_conj_{t}", "min_5")["dst"]
        assert (d[0::2] == i.min).all() and (d[1::2] == i.max).all()
    d = gold("cmplx_conj_f32", "signzero_8")
    assert (d["dst"].view(np.uint32)[1::2] == d["a"].view(np.uint32)[1::2] ^ 0x80000000).all()
    # (-32768, -32768): the unsigned sum 2^31, >> 1 = 2^30 (0.5 in q31), whose root >> 16 is 0x5A82 = 23170
    assert (gold("cmplx_mag_q15", "min_5")["dst"] == 23170).all()
    assert (gold("cmplx_mult_real_q15", "min_5")["dst"] == 32767).all()        # -32768 * -32768 saturates
    assert (gold("cmplx_mult_real_q31", "min_5")["dst"] == 2**31 - 1).all()
    d = gold("cmplx_mult_cmplx_q15", "edge_4")["dst"]
    assert d.max() == 16384 and d.min() == -16384                              # the widest a difference / sum gets
    for op in ("max", "min"):
        g = gold(f"{op}_f32", "nan0_6")
        assert np.isnan(g["value"]) and int(g["index"]) == 0
        g = gold(f"{op}_f32", "nanmid_6")
        assert not np.isnan(g["value"]) and int(g["index"]) != 3
        for t in ("f32", "q31", "q15", "q7"):
            assert int(gold(f"{op}_{t}", "first_9")["index"]) == 0
            assert int(gold(f"{op}_{t}", "last_9")["index"]) == 8
            assert int(gold(f"{op}_{t}", "tail_8")["index"]) == 6
            assert int(gold(f"{op}_{t}", "tie_9")["index"]) == 2
            assert int(gold(f"{op}_{t}", "equal_6")["index"]) == 0
    # +0.0 before -0.0 and after it: the earlier one wins with its own sign bit
    assert gold("max_f32", "pznz_5")["value"].view(np.uint32) == 0 and int(gold("max_f32", "pznz_5")["index"]) == 1
    assert gold("max_f32", "nzpz_5")["value"].view(np.uint32) == 0x80000000
    assert int(gold("max_f32", "nzpz_5")["index"]) == 1


def test_library_exports_the_52_symbols(dsp):
    names = [f"arm_{f}{suffix}" for f in cm.FUNCS for suffix in ("", "_batch")]
    assert len(set(names)) == 52 and set(names) == set(_abi.CMPLX_MATH)
    for n in names:
        assert callable(getattr(dsp.lib, n)), n


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for f in cm.FUNCS:
        fn = getattr(d, "arm_" + f)
        assert callable(fn) and "cmsis_arm_" + f in fn.__doc__, f
    for n in ("arm_cmplx_mag", "arm_cmplx_mag_squared", "arm_cmplx_conj", "arm_cmplx_mult_cmplx", "arm_cmplx_mult_real",
              "arm_cmplx_dot_prod", "arm_max", "arm_min", "cmplx_mag_batch", "cmplx_mag_squared_batch",
              "cmplx_conj_batch", "cmplx_mult_cmplx_batch", "cmplx_mult_real_batch", "cmplx_dot_prod_batch",
              "max_batch", "min_batch"):
        assert callable(getattr(dsp, n)), n


# ------------------------------------------------------------------ GPU helpers
class Dev:
    """A device copy of x whose first word sits `off` elements into a marker-filled allocation, GUARD marker words
    after its end."""

    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.t = {np.dtype(v): k for k, v in cm.MDT.items() if k != "u32"}.get(x.dtype, "u32")
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


def call(dsp, func, ptrs, n, batch=None, stride=None):
    """arm_<func> (batch None) or arm_<func>_batch on raw addresses in the C order; n: numSamples / blockSize."""
    op, t = cm.split(func)
    name = f"arm_{func}" + ("" if batch is None else "_batch")
    fn = getattr(dsp.lib, name)
    tail = [] if batch is None else [batch, None]
    if op in ("max", "min"):
        args = [ptrs[0], n, ptrs[1], ptrs[2]]
    elif op == "dot_prod":
        args = [ptrs[0], ptrs[1]] + ([] if batch is None else [n if stride is None else stride]) + [n, ptrs[2], ptrs[3]]
    else:
        args = list(ptrs) + [n]
    st = fn(*args, *tail)
    return 0 if st is None else st


def in_names(func):
    op = cm.split(func)[0]
    return {"mult_cmplx": ("a", "b"), "dot_prod": ("a", "b"), "mult_real": ("a", "r")}.get(op, ("a",))


def n_of(func, g):
    return g["a"].shape[-1] // (1 if cm.split(func)[0] in ("max", "min") else 2)


def run_on(dsp, torch, func, g, where, off=0, alias=None, batch=None, stride=None):
    """The drop-in (batch None) or the batched form on host arrays or device buffers (at element offset off), the
    outputs pre-filled with the marker; alias: dst is that source's buffer.  -> (status, the outputs)."""
    put = (lambda x: Host(x)) if where == "host" else (lambda x: Dev(torch, x, off))
    src = {k: put(g[k]) for k in in_names(func)}
    spec = cm.out_spec(func, g)
    out = {k: (src[alias] if alias and k == "dst" else put(cm.marked(ty, shape if shape else 1)))
           for k, (ty, shape) in spec.items()}
    ptrs = [src[k].ptr for k in in_names(func)] + [out[k].ptr for k in out_names(func)]
    st = call(dsp, func, ptrs, n_of(func, g), batch, stride)
    if where != "host":
        torch.cuda.synchronize()
    for k in in_names(func):
        if k != alias:
            assert src[k].get().tobytes() == g[k].tobytes(), (func, k)
    return st, {k: out[k].get().reshape(spec[k][1]) for k in out}


def rand_operands(func, shape, rng):
    """Random operands of `shape` = (..., n): n complex samples (max / min: words) per item."""
    op, t = cm.split(func)
    words = shape if op in ("max", "min") else shape[:-1] + (2 * shape[-1],)
    g = {"a": cm.rand(t, words, rng)}
    if op in ("mult_cmplx", "dot_prod"):
        g["b"] = cm.rand(t, words, rng)
    if op == "mult_real":
        g["r"] = cm.rand(t, shape, rng)
    return g


# ------------------------------------------------------------------ GPU: drop-ins against the fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("func", cm.FUNCS)
def test_dropin_equals_fixtures(dsp, torch_gpu, func, where):
    for case in cm.case_names(func):
        g = gold(func, case)
        st, got = run_on(dsp, torch_gpu, func, g, where)
        assert dsp.last_error()[0] == 0, (func, case, dsp.last_error())
        check(func, case, got, g)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("func", [f for f in EW if cm.split(f)[0] in ("conj", "mult_cmplx", "mult_real")])
def test_in_place_alias(dsp, torch_gpu, func, where):
    """arm_cmplx_conj_f32(p, p, n), mult_cmplx into pSrcA or pSrcB, mult_real into pSrcCmplx; the batched forms
    on device memory too."""
    op = cm.split(func)[0]
    for case in cm.case_names(func):
        g = gold(func, case)
        for alias in ("a", "b") if op == "mult_cmplx" else ("a",):
            st, got = run_on(dsp, torch_gpu, func, g, where, alias=alias)
            assert dsp.last_error()[0] == 0
            check(func, case, got, g)
    if where == "device":
        g = rand_operands(func, (9, 35), np.random.default_rng(5))
        for alias in ("a", "b") if op == "mult_cmplx" else ("a",):
            st, got = run_on(dsp, torch_gpu, func, g, where, alias=alias, batch=9)
            assert st == SUCCESS
            check(func, "batch", got, cm.run(func, g))


@pytest.mark.gpu
@pytest.mark.parametrize("t", cm.CTYPES)
def test_mag_into_its_own_source(dsp, torch_gpu, t):
    """Host pointers are staged separately, so mag / mag_squared may write over their source; on device pointers
    the same call, and every partial overlap, is refused: the last error is set and nothing is written."""
    torch, lib = torch_gpu, dsp.lib
    rng = np.random.default_rng(9)
    a = cm.rand(t, 2 * 37, rng)
    for op in ("mag", "mag_squared"):
        h = a.copy()
        getattr(lib, f"arm_cmplx_{op}_{t}")(h.ctypes.data, h.ctypes.data, 37)
        assert dsp.last_error()[0] == 0
        assert h[:37].tobytes() == cm.run(f"cmplx_{op}_{t}", {"a": a})["dst"].tobytes()
        assert h[37:].tobytes() == a[37:].tobytes()
    item = a.itemsize
    for op, words in (("mag", 1), ("mag_squared", 1), ("conj", 2), ("mult_cmplx", 2), ("mult_real", 2)):
        for shift in (0, 2, -2) if words == 1 else (2, -2):           # the exact alias of the 2-word forms is allowed
            d = Dev(torch, np.concatenate([a, a, a]))
            src = d.ptr + 74 * item
            dst = src + shift * item
            two = op in ("mult_cmplx", "mult_real")
            other = Dev(torch, a)
            args = [src] + ([other.ptr] if two else []) + [dst, 37]
            getattr(lib, f"arm_cmplx_{op}_{t}")(*args)
            code, msg = dsp.last_error()
            assert code != 0 and f"arm_cmplx_{op}_{t}" in msg, (op, shift)
            lib.arm_mi355x_clear_error()
            assert getattr(lib, f"arm_cmplx_{op}_{t}_batch")(*args, 1, None) == ARGUMENT_ERROR
            assert dsp.last_error()[0] != 0
            lib.arm_mi355x_clear_error()
            torch.cuda.synchronize()
            assert d.get().tobytes() == np.concatenate([a, a, a]).tobytes()
    # mult_real: dst on the real source, and the dot product's results inside a source
    c, r = Dev(torch, a), Dev(torch, a)
    assert getattr(lib, f"arm_cmplx_mult_real_{t}_batch")(c.ptr, r.ptr, r.ptr, 18, 1, None) == ARGUMENT_ERROR
    out = Dev(torch, cm.marked(cm.DOT_OUT[t], 2))
    assert getattr(lib, f"arm_cmplx_dot_prod_{t}_batch")(c.ptr, r.ptr, 0, 37, c.ptr, out.ptr, 1, None) == ARGUMENT_ERROR
    lib.arm_mi355x_clear_error()
    torch.cuda.synchronize()
    assert c.get().tobytes() == a.tobytes() and r.get().tobytes() == a.tobytes()


@pytest.mark.gpu
def test_status_and_null_cases(dsp, torch_gpu):
    """NULL, zero sizes, batch == 0 and a bad bStride, for the drop-ins (void: the last error) and the batched
    forms (arm_status); nothing is written in any of them except the dot products' zeros."""
    torch, lib = torch_gpu, dsp.lib
    for t in ("f32", "q31", "q15", "q7"):
        a = Dev(torch, cm.rand(t, 4 * 10, np.random.default_rng(1)))
        d = Dev(torch, cm.marked(t, 4 * 10))
        idx = Dev(torch, cm.marked("u32", 4))

        def void(name, *args, fails):
            getattr(lib, name)(*args)
            code, msg = dsp.last_error()
            assert (code != 0) == fails and (not fails or name in msg), (name, args, code, msg)
            lib.arm_mi355x_clear_error()

        for op in ("max", "min"):
            name = f"arm_{op}_{t}"
            void(name, None, 10, d.ptr, idx.ptr, fails=True)
            void(name, a.ptr, 10, None, idx.ptr, fails=True)
            void(name, a.ptr, 10, d.ptr, None, fails=True)
            void(name, a.ptr, 0, d.ptr, idx.ptr, fails=True)                 # the reference reads pSrc[0]
            fb = getattr(lib, name + "_batch")
            assert fb(a.ptr, 10, d.ptr, idx.ptr, 0, None) == SUCCESS
            assert fb(a.ptr, 0, d.ptr, idx.ptr, 0, None) == SUCCESS
            assert fb(a.ptr, 0, d.ptr, idx.ptr, 4, None) == ARGUMENT_ERROR
            assert fb(None, 10, d.ptr, idx.ptr, 4, None) == ARGUMENT_ERROR
            assert fb(a.ptr, 10, None, idx.ptr, 4, None) == ARGUMENT_ERROR
            assert fb(a.ptr, 10, d.ptr, None, 4, None) == ARGUMENT_ERROR
        if t != "q7":
            b = Dev(torch, cm.rand(t, 4 * 10, np.random.default_rng(2)))
            for op in ("mag", "mag_squared", "conj"):
                name = f"arm_cmplx_{op}_{t}"
                void(name, None, d.ptr, 5, fails=True)
                void(name, a.ptr, None, 5, fails=True)
                void(name, a.ptr, d.ptr, 0, fails=False)
                fb = getattr(lib, name + "_batch")
                assert fb(a.ptr, d.ptr, 5, 0, None) == SUCCESS and fb(a.ptr, d.ptr, 0, 4, None) == SUCCESS
                assert fb(None, d.ptr, 5, 4, None) == ARGUMENT_ERROR and fb(a.ptr, None, 5, 4, None) == ARGUMENT_ERROR
            for op in ("mult_cmplx", "mult_real"):
                name = f"arm_cmplx_{op}_{t}"
                void(name, None, b.ptr, d.ptr, 5, fails=True)
                void(name, a.ptr, None, d.ptr, 5, fails=True)
                void(name, a.ptr, b.ptr, None, 5, fails=True)
                void(name, a.ptr, b.ptr, d.ptr, 0, fails=False)
                fb = getattr(lib, name + "_batch")
                assert fb(a.ptr, b.ptr, d.ptr, 5, 0, None) == SUCCESS and fb(a.ptr, b.ptr, d.ptr, 0, 4, None) == SUCCESS
                assert fb(None, b.ptr, d.ptr, 5, 4, None) == ARGUMENT_ERROR
                assert fb(a.ptr, None, d.ptr, 5, 4, None) == ARGUMENT_ERROR
                assert fb(a.ptr, b.ptr, None, 5, 4, None) == ARGUMENT_ERROR
            name = f"arm_cmplx_dot_prod_{t}"
            ot = cm.DOT_OUT[t]
            re, im = Dev(torch, cm.marked(ot, 4)), Dev(torch, cm.marked(ot, 4))
            void(name, None, b.ptr, 5, re.ptr, im.ptr, fails=True)
            void(name, a.ptr, None, 5, re.ptr, im.ptr, fails=True)
            void(name, a.ptr, b.ptr, 5, None, im.ptr, fails=True)
            void(name, a.ptr, b.ptr, 5, re.ptr, None, fails=True)
            fb = getattr(lib, name + "_batch")
            assert fb(a.ptr, b.ptr, 5, 5, re.ptr, im.ptr, 0, None) == SUCCESS
            for bad in (1, 4):
                assert fb(a.ptr, b.ptr, bad, 5, re.ptr, im.ptr, 4, None) == ARGUMENT_ERROR
            assert fb(None, b.ptr, 5, 5, re.ptr, im.ptr, 4, None) == ARGUMENT_ERROR
            assert fb(a.ptr, b.ptr, 5, 5, None, im.ptr, 4, None) == ARGUMENT_ERROR
            torch.cuda.synchronize()
            assert re.get().tobytes() == cm.marked(ot, 4).tobytes() and im.get().tobytes() == cm.marked(ot, 4).tobytes()
            # numSamples == 0: the empty sums, zeros, as the reference stores them
            void(name, a.ptr, b.ptr, 0, re.ptr, im.ptr, fails=False)
            assert fb(a.ptr, b.ptr, 0, 0, re.ptr + re.get().itemsize, im.ptr + im.get().itemsize, 3, None) == SUCCESS
            torch.cuda.synchronize()
            assert not re.get().any() and not im.get().any()
        torch.cuda.synchronize()
        assert d.get().tobytes() == cm.marked(t, 4 * 10).tobytes(), t              # nothing was written
        assert idx.get().tobytes() == cm.marked("u32", 4).tobytes()
        assert lib.arm_mi355x_last_error() == 0


# ------------------------------------------------------------------ GPU: element-wise shapes
EW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 257, 1025)


@pytest.mark.gpu
@pytest.mark.parametrize("func", EW)
def test_elementwise_shapes(dsp, torch_gpu, func):
    """Every length with the pointers 16-B aligned (the vector path and its ragged end) and at an element offset of
    1 (q15: 1 and 3; the scalar path), then a batch of 257 items of 5 samples."""
    rng = np.random.default_rng(7)
    t = cm.split(func)[1]
    offs = (0, 1, 3) if t == "q15" else (0, 1)
    for n in EW_LENGTHS:
        g = rand_operands(func, (n,), rng)
        want = cm.run(func, g)
        for off in offs:
            st, got = run_on(dsp, torch_gpu, func, g, "device", off=off)
            assert dsp.last_error()[0] == 0
            check(func, (n, off), got, want)
    g = rand_operands(func, (257, 5), rng)
    want = cm.run(func, g)
    for off in offs:
        st, got = run_on(dsp, torch_gpu, func, g, "device", off=off, batch=257)
        assert st == SUCCESS
        check(func, ("batch", off), got, want)


@pytest.mark.gpu
def test_fixed_point_extremes(dsp, torch_gpu):
    """All-minimum, all-maximum and mixed extreme operands at a length that reaches the vector path."""
    rng = np.random.default_rng(11)
    for func in EW + DOT:
        t = cm.split(func)[1]
        if t == "f32":
            continue
        i = np.iinfo(cm.DT[t])
        for fill in (i.min, i.max, None):
            g = rand_operands(func, (133,), rng)
            for k in g:
                g[k] = np.full_like(g[k], fill) if fill is not None else cm.extremes(t, g[k].shape, rng)
            st, got = run_on(dsp, torch_gpu, func, g, "device")
            check(func, fill, got, cm.run(func, g))


# ------------------------------------------------------------------ GPU: dot products and max / min
# 1, 2: one lane; 63, 64, 65: the lanes-per-item steps; 1025: a wave with several loads per lane; the last length
# is one past what a wave takes: 16-B packs when aligned, words at an element offset
def reduce_lengths(func):
    op, t = cm.split(func)
    per_pack = 16 // np.dtype(cm.DT[t]).itemsize // (1 if op in ("max", "min") else 2)
    return (1, 2, 63, 64, 65, REDUCE_WAVE_MAX + 1, 1025, REDUCE_WAVE_MAX * per_pack + per_pack)


@pytest.mark.gpu
@pytest.mark.parametrize("func", DOT + SEARCH)
def test_reduction_lengths(dsp, torch_gpu, func):
    rng = np.random.default_rng(13)
    op, t = cm.split(func)
    for n in reduce_lengths(func):
        g = rand_operands(func, (n,), rng)
        want = cm.run(func, g)
        for off in (0, 1):
            st, got = run_on(dsp, torch_gpu, func, g, "device", off=off)
            assert dsp.last_error()[0] == 0
            check(func, (n, off), got, want)
        st, got = run_on(dsp, torch_gpu, func, g, "host")
        check(func, (n, "host"), got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", DOT)
def test_dot_prod_batches(dsp, torch_gpu, func):
    """257 items of 5 and of 300 samples with bStride 0 (one shared B), numSamples and numSamples + 3; f32 also
    DOT_LANE_MIN_BATCH + 1 items (the one-lane-per-item kernel) of 5 and of 2 DOT_CHUNK + 3 samples."""
    rng = np.random.default_rng(17)
    t = cm.split(func)[1]
    shapes = [(257, 5), (257, 300)]
    if t == "f32":
        shapes += [(DOT_LANE_MIN_BATCH + 1, 5), (DOT_LANE_MIN_BATCH + 1, 2 * DOT_CHUNK + 3)]
    for batch, n in shapes:
        a = cm.rand(t, (batch, 2 * n), rng)
        for stride in (0, n, n + 3):
            b = cm.rand(t, (2 * n,) if stride == 0 else (batch, 2 * n), rng)
            want = cm.run(func, {"a": a, "b": b if stride else np.broadcast_to(b, a.shape)})
            padded = b
            if stride > n:
                padded = cm.marked(t, (batch, 2 * stride))
                padded[:, :2 * n] = b
                padded = padded.reshape(-1)[:2 * (stride * (batch - 1) + n)]
            for off in (0, 1):
                da, db = Dev(torch_gpu, a, off), Dev(torch_gpu, padded, off)
                re, im = (Dev(torch_gpu, cm.marked(cm.DOT_OUT[t], batch), off) for _ in range(2))
                assert call(dsp, func, [da.ptr, db.ptr, re.ptr, im.ptr], n, batch, stride) == SUCCESS
                torch_gpu.cuda.synchronize()
                check(func, (batch, n, stride, off), {"re": re.get(), "im": im.get()}, want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", SEARCH)
def test_search_batches_and_ties(dsp, torch_gpu, func):
    """257 items of 5 and of 300 words; one search over 70001 words with the extreme at index 70000 (past 16 bits);
    ties that straddle a lane's loads, a wave (64 lanes) and the workgroup's four waves: the lower index wins."""
    rng = np.random.default_rng(19)
    op, t = cm.split(func)
    for batch, n in ((257, 5), (257, 300)):
        g = rand_operands(func, (batch, n), rng)
        for off in (0, 1):
            st, got = run_on(dsp, torch_gpu, func, g, "device", off=off, batch=batch)
            assert st == SUCCESS
            check(func, (batch, n, off), got, cm.run(func, g))
    i = np.iinfo(cm.DT[t]) if t != "f32" else None
    peak = cm.DT[t]((5.0 if op == "max" else -5.0) if t == "f32" else (i.max if op == "max" else i.min))
    lo, hi = (-1.0, 1.0) if t == "f32" else (i.min + 1, i.max - 1)

    def field(n):
        if t == "f32":
            return rng.uniform(lo, hi, n).astype(np.float32)
        return rng.integers(lo, hi, n, endpoint=True).astype(cm.DT[t])

    a = field(70001)
    a[70000] = peak
    for off in (0, 1):
        st, got = run_on(dsp, torch_gpu, func, {"a": a}, "device", off=off)
        assert int(got["index"]) == 70000 and got["value"] == peak, (func, off)
    # 70000 words: whole 16-B packs, the whole workgroup on the item; lane l holds packs l, l + 256, ...
    per_pack = 16 // a.itemsize
    for first, second in ((63 * per_pack + 1, 64 * per_pack), (255 * per_pack + 2, 256 * per_pack),
                          (64 * per_pack - 1, 300 * per_pack + 3), (7, 69999)):
        b = field(70000)
        b[[first, second]] = peak
        for off in (0, 1):
            st, got = run_on(dsp, torch_gpu, func, {"a": b}, "device", off=off)
            assert int(got["index"]) == first, (func, first, second, off, int(got["index"]))
    # a wave per item (300 words): the tie in two lanes, and in two loads of one lane
    c = field((4, 300))
    for row, (first, second) in enumerate(((3, 4), (17, 17 + 64), (0, 299), (150, 151))):
        c[row, [first, second]] = peak
    for off in (0, 1):
        st, got = run_on(dsp, torch_gpu, func, {"a": c}, "device", off=off, batch=4)
        assert got["index"].tolist() == [3, 17, 0, 150], (func, off)


# ------------------------------------------------------------------ GPU: f32 classes
@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["subnormal", "negzero", "signzero", "mixed", "overflow", "nonfinite"])
def test_f32_classes(dsp, torch_gpu, cls):
    """Subnormals, signed zeros, overflow to +-Inf and +-Inf / NaN inputs through mag, mag_squared, mult_cmplx,
    dot_prod, max and min: finite inputs bit-equal, with non-finite inputs the non-NaN words bit-equal and the NaNs
    in place.  131 samples: the vector path and its ragged end."""
    n = 131
    a = f32_class_input(cls, 2 * n, 23, scale=1.5e19, positions=(3, 40, 200))
    b = f32_class_input(cls, 2 * n, 24, scale=1.5e19, positions=(3, 41, 201))
    if cls == "overflow":
        assert np.isfinite(a).all() and np.isfinite(b).all()
    for op in ("mag", "mag_squared", "mult_cmplx", "dot_prod"):
        func = f"cmplx_{op}_f32"
        g = {"a": a, "b": b}
        want = cm.run(func, g)
        for where in ("host", "device"):
            st, got = run_on(dsp, torch_gpu, func, g, where)
            for k in want:
                assert_same_words(np.asarray(got[k]).reshape(np.shape(want[k])), want[k], f"{op} {cls} {where} {k}")
    if cls == "subnormal":
        s = (a * np.float32(2.0 ** 62)).astype(np.float32)                        # squares that are subnormal
        st, got = run_on(dsp, torch_gpu, "cmplx_mag_f32", {"a": s}, "device")
        assert_same_words(got["dst"], cm.mag("f32", s), "mag of subnormal sums")
    x = f32_class_input(cls, n, 25, scale=3.0e38, positions=(0, 40, 100))        # nonfinite: +Inf at word 0
    y = f32_class_input(cls, n, 26, scale=3.0e38, positions=(5, 40, 0))          # nonfinite: NaN at word 0
    for op in ("max", "min"):
        for src in (x, y):
            want = cm.run(f"{op}_f32", {"a": src})
            for where in ("host", "device"):
                st, got = run_on(dsp, torch_gpu, f"{op}_f32", {"a": src}, where)
                assert_same_words(got["value"].reshape(()), want["value"], f"{op} {cls} {where}")
                assert int(got["index"]) == int(want["index"]), (op, cls, where)


# ------------------------------------------------------------------ GPU: the Python layers
@pytest.mark.gpu
def test_python_wrappers(dsp, torch_gpu):
    """cmsisdsp's 26 names with the reference binding's conventions, and cmsisdsp_amd's batched forms on tensors."""
    import cmsisdsp as d
    torch = torch_gpu
    for func in cm.FUNCS:
        op, t = cm.split(func)
        g = gold(func, "rand_67")
        got = getattr(d, "arm_" + func)(*[g[k] for k in in_names(func)])
        if op == "dot_prod":
            assert isinstance(got, tuple) and len(got) == 2 and isinstance(got[0], float if t == "f32" else int)
            assert cm.MDT[cm.DOT_OUT[t]](got[0]) == g["re"] and cm.MDT[cm.DOT_OUT[t]](got[1]) == g["im"], func
        elif op in ("max", "min"):
            assert isinstance(got, tuple) and cm.DT[t](got[0]) == g["value"] and got[1] == int(g["index"]), func
        else:
            assert isinstance(got, np.ndarray) and got.dtype == g["dst"].dtype, func
            assert got.tobytes() == g["dst"].tobytes(), func
    rng = np.random.default_rng(29)
    dev = lambda x: torch.from_numpy(x).cuda()                                   # noqa: E731
    for t in cm.CTYPES:
        a, b, r = cm.rand(t, (6, 2 * 35), rng), cm.rand(t, (6, 2 * 35), rng), cm.rand(t, (6, 35), rng)
        ta, tb, tr = dev(a), dev(b), dev(r)
        for name, fn, ref in (("mag", dsp.cmplx_mag_batch, cm.mag),
                              ("mag_squared", dsp.cmplx_mag_squared_batch, cm.mag_squared)):
            td = dev(cm.marked(t, (6, 35)))
            fn(ta, td)
            assert td.cpu().numpy().tobytes() == ref(t, a).tobytes(), (name, t)
        td = dev(cm.marked(t, (6, 70)))
        dsp.cmplx_conj_batch(ta, td)
        assert td.cpu().numpy().tobytes() == cm.conj(t, a).tobytes()
        dsp.cmplx_mult_cmplx_batch(ta, tb, td)
        assert td.cpu().numpy().tobytes() == cm.mult_cmplx(t, a, b).tobytes()
        dsp.cmplx_mult_real_batch(ta, tr, td)
        assert td.cpu().numpy().tobytes() == cm.mult_real(t, a, r).tobytes()
        ot = cm.MDT[cm.DOT_OUT[t]]
        re, im = dev(cm.marked(cm.DOT_OUT[t], 6)), dev(cm.marked(cm.DOT_OUT[t], 6))
        dsp.cmplx_dot_prod_batch(ta, tb, re, im)
        wr, wi = cm.dot_prod(t, a, b)
        assert re.cpu().numpy().tobytes() == np.asarray(wr, dtype=ot).tobytes()
        assert im.cpu().numpy().tobytes() == np.asarray(wi, dtype=ot).tobytes()
        dsp.cmplx_dot_prod_batch(ta, tb[0], re, im)
        wr, wi = cm.dot_prod(t, a, np.broadcast_to(b[0], a.shape))
        assert re.cpu().numpy().tobytes() == np.asarray(wr, dtype=ot).tobytes()
        with pytest.raises(RuntimeError):
            dsp.cmplx_dot_prod_batch(ta, tb, re, im, b_stride=34)
        with pytest.raises(RuntimeError):
            dsp.cmplx_mag_batch(ta, ta)
        dsp.lib.arm_mi355x_clear_error()
    for t in ("f32", "q31", "q15", "q7"):
        a = cm.rand(t, (6, 35), rng)
        val, idx = dev(cm.marked(t, 6)), dev(cm.marked("u32", 6).view(np.int32))
        for op, fn in (("max", dsp.max_batch), ("min", dsp.min_batch)):
            fn(dev(a), val, idx)
            wv, wi = cm.extreme(op, a)
            assert val.cpu().numpy().tobytes() == wv.tobytes()
            assert idx.cpu().numpy().view(np.uint32).tolist() == wi.tolist()
