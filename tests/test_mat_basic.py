"""arm_mat_{add,sub,scale}_{f32,q31,q15}, arm_mat_trans_{f32,q31,q15,q7}, arm_mat_cmplx_trans_{f32,q31,q15} and
arm_mat_vec_mult_{f32,q31,q15,q7}: the 20 drop-ins and their _batch forms (cmsis-dsp_amd/csrc/mat_basic.hip).

The checker is committed data: tests/golden/mat_basic.npz holds the reference's own outputs, every output buffer
pre-filled with a marker word (tools/make_golden_mat_basic.py); tests/mat_basic_ref.py restates the 20 functions
in numpy, the q15 pair wrap and the 16-bit row offset of vec_mult_q15 / _q31 included, and the generator asserted
it against the reference case by case.  Every comparison is bit-exact; f32 cases with Inf / NaN inputs follow the
rule of tests/test_f32_classes.py (non-NaN words bit-equal, NaNs at the same positions).

CPU: the fixture index, the restatement against every fixture, the probed facts, the 40 exported symbols, the
Python names.  GPU: the drop-ins on host and device pointers against every fixture, the exact in-place alias, the
status cases, and the shapes at which the kernels change path -- the 16-B / scalar split of the element-wise
kernel (aligned, offset by one element, ragged ends), the packed / tiled split of the transposes (256 elements;
tiles of 32 or 64), the 128-byte column steps and the row-tile widths of vec_mult."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mat_basic_ref as mb
from cmsisdsp_amd import _abi
from f32_classes import assert_same_words, f32_class_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "mat_basic.npz"))
INDEX = [tuple(x) for x in json.loads(str(GOLD["index"]))]
EW = [f"{op}_{t}" for op in ("add", "sub", "scale") for t in mb.EW_TYPES]
TRANS = [f for f in mb.FUNCS if "trans" in f]
VEC_TYPES = ("f32", "q31", "q15", "q7")
GUARD = 8                      # marker words after the end of every device buffer


def gold(func, case):
    pre = f"{func}/{case}/"
    return {k[len(pre):]: GOLD[k] for k in GOLD.files if k.startswith(pre)}


def check(func, case, got, want):
    for k, v in want.items():
        if k == "status":
            assert got["status"] == int(v), (func, case, got["status"])
        elif k == "dst":
            assert mb.same_words(got["dst"], v, str(case).startswith("nonfinite")), (func, case, got["dst"], v)


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert len(mb.FUNCS) == 20 and len(set(mb.FUNCS)) == 20
    assert INDEX == [(f, c) for f in mb.FUNCS for c in mb.case_names(f)]
    for f, c in INDEX:
        g = gold(f, c)
        assert "dst" in g and ("status" in g) == (not f.startswith("vec_mult")), (f, c)


def test_restatement_equals_every_fixture():
    for f, c in INDEX:
        g = gold(f, c)
        check(f, c, mb.run(f, g), g)


def test_probed_facts_hold_in_the_fixtures():
    """All-minimum q15 operands (the wrapping __SMLALD pair), the 16-bit row offset, the q31 scale saturation."""
    for shape, word in (("4x6", -32768), ("5x7", -32768), ("3x7", -32768), ("1x3", 32767)):
        d = gold("vec_mult_q15", f"min_{shape}")["dst"]
        assert (d == word).all(), (shape, d)
    d = gold("vec_mult_q15", "pairwrap_7x7")["dst"]
    assert (d[:4] == -32768).all() and (d[4:] == 32767).all()          # group rows pair columns 4, 5; tail rows do not
    for t in ("q15", "q31"):
        g = gold(f"vec_mult_{t}", "big_258x256")
        d = g["dst"]
        assert d[256] == d[0] and d[257] == d[1]
        assert not (g["m"][256] == g["m"][0]).all() and not (g["m"][257] == g["m"][1]).all()
    for t in ("f32", "q7"):
        d = gold(f"vec_mult_{t}", "big_258x256")["dst"]
        assert d[256] != d[0] and d[257] != d[1]
        assert t == "f32" or np.abs(d.astype(int)).max() < 127
    g = gold("scale_q31", "sat_3x5")
    a, d = g["a"].reshape(-1), g["dst"].reshape(-1)
    assert int(g["scale"]) == 0x7FFFFFFF and int(g["shift"]) == 1
    assert d[a == -2**31].tolist() == [-2**31] * int((a == -2**31).sum()) and (a == -2**31).any()
    assert (d[a == 2**31 - 1] == 2**31 - 1).all() and (a == 2**31 - 1).any()
    for t, (lo, hi) in mb.SHIFT_RANGE.items():
        for s in (lo, hi):
            assert (f"scale_{t}", f"shift{s}_3x5") in INDEX


def test_library_exports_the_40_symbols(dsp):
    names = [f"arm_mat_{f}{suffix}" for f in mb.FUNCS for suffix in ("", "_batch")]
    assert len(set(names)) == 40 and set(names) == set(_abi.MAT_BASIC)
    for n in names:
        assert callable(getattr(dsp.lib, n)), n


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for f in mb.FUNCS:
        fn = getattr(d, "arm_mat_" + f)
        assert callable(fn) and "cmsis_arm_mat_" + f in fn.__doc__, f
    for n in ("arm_mat_add", "arm_mat_sub", "arm_mat_scale", "arm_mat_trans", "arm_mat_cmplx_trans", "arm_mat_vec_mult",
              "mat_add_batch", "mat_sub_batch", "mat_scale_batch", "mat_trans_batch", "mat_cmplx_trans_batch",
              "mat_vec_mult_batch"):
        assert callable(getattr(dsp, n)), n


# ------------------------------------------------------------------ GPU helpers
def call(dsp, func, shape, pa, pb, pd, scale=None, shift=0, batch=None, stride=0):
    """arm_mat_<func> (batch None) or arm_mat_<func>_batch on raw host or device addresses.  shape: the source
    matrix's (rows, cols), complex: in pairs.  vec_mult: pa the matrix, pb the vector(s).  -> status."""
    op, t = mb.split(func)

    def inst(p, s):
        return C.byref(_abi.MAT_INST[t](s[0], s[1], C.cast(p, _abi.MAT_PTR[t])))

    name = f"arm_mat_{func}" + ("" if batch is None else "_batch")
    fn = getattr(dsp.lib, name)
    tail = [] if batch is None else [batch, None]
    if op in ("add", "sub"):
        st = fn(inst(pa, shape), inst(pb, shape), inst(pd, shape), *tail)
    elif op == "scale":
        args = [float(scale)] if t == "f32" else [int(scale), int(shift)]
        st = fn(inst(pa, shape), *args, inst(pd, shape), *tail)
    elif op in ("trans", "cmplx_trans"):
        st = fn(inst(pa, shape), inst(pd, shape[::-1]), *tail)
    elif batch is None:
        st = fn(inst(pa, shape), pb, pd) or 0
    else:
        st = fn(inst(pa, shape), stride, pb, pd, *tail)
    dsp._check_void(name)
    return st


class Dev:
    """A device copy of x whose first word sits `off` elements into a marker-filled allocation, GUARD marker words
    after its end."""

    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.t = {np.dtype(v): k for k, v in mb.DT.items()}[x.dtype]
        self.off, self.n, self.shape = off, x.size, x.shape
        self.buf = torch.from_numpy(mb.marked(self.t, off + x.size + GUARD)).cuda()
        self.buf[off:off + x.size].copy_(torch.from_numpy(x.reshape(-1)))
        self.ptr = self.buf.data_ptr() + off * x.itemsize

    def get(self):
        """The words, after checking that nothing around them changed."""
        b = self.buf.cpu().numpy()
        m = mb.marked(self.t, 1).tobytes()
        assert b[:self.off].tobytes() == m * self.off and b[self.off + self.n:].tobytes() == m * GUARD, "guard words"
        return b[self.off:self.off + self.n].reshape(self.shape)


def src_shape(func, a):
    return (a.shape[-2], a.shape[-1] // 2) if func.startswith("cmplx") else a.shape[-2:]


def dst_like(func, g):
    op, t = mb.split(func)
    if op == "vec_mult":
        return mb.marked(t, g["m"].shape[0])
    a = g["a"]
    if op == "trans":
        return mb.marked(t, a.shape[::-1])
    if op == "cmplx_trans":
        return mb.marked(t, (a.shape[1] // 2, 2 * a.shape[0]))
    return mb.marked(t, a.shape)


def dropin(dsp, torch, func, g, where, off=0, alias=None):
    """The drop-in on host arrays or device buffers (at element offset off), dst pre-filled with the marker;
    alias "a" / "b": dst is that source's buffer.  -> the dict mat_basic_ref.run returns."""
    op, t = mb.split(func)
    if where == "host":
        put, addr, words = (lambda x: np.ascontiguousarray(x).copy()), (lambda h: h.ctypes.data), (lambda h: h)
    else:
        put, addr, words = (lambda x: Dev(torch, x, off)), (lambda h: h.ptr), (lambda h: h.get())
    if op == "vec_mult":
        m, v, d = put(g["m"]), put(g["v"]), put(dst_like(func, g))
        call(dsp, func, g["m"].shape, addr(m), addr(v), addr(d))
        assert words(m).tobytes() == g["m"].tobytes() and words(v).tobytes() == g["v"].tobytes()
        return {"dst": words(d)}
    a = put(g["a"])
    b = put(g["b"]) if "b" in g else None
    d = a if alias == "a" else b if alias == "b" else put(dst_like(func, g))
    st = call(dsp, func, src_shape(func, g["a"]), addr(a), addr(b) if b is not None else None, addr(d),
              scale=g["scale"].item() if "scale" in g else None, shift=int(g["shift"]) if "shift" in g else 0)
    if alias != "a":
        assert words(a).tobytes() == g["a"].tobytes()
    return {"status": st, "dst": words(d)}


def ew_operands(func, shape, rng, batch=None):
    op, t = mb.split(func)
    full = shape if batch is None else (batch,) + shape
    g = {"a": mb.rand(t, full, rng)}
    if op == "scale":
        g["scale"] = np.float32(1.7) if t == "f32" else mb.DT[t](mb.rand(t, (), rng))
        g["shift"] = np.int32(int(rng.integers(-1, 4)) if t != "f32" else 0)
    else:
        g["b"] = mb.rand(t, full, rng)
    return g


# ------------------------------------------------------------------ GPU: drop-ins against the fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("func", mb.FUNCS)
def test_dropin_equals_fixtures(dsp, torch_gpu, func, where):
    for case in mb.case_names(func):
        g = gold(func, case)
        check(func, case, dropin(dsp, torch_gpu, func, g, where), g)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("func", EW)
def test_dropin_in_place_alias(dsp, torch_gpu, func, where):
    """arm_mat_add_f32(&A, &B, &A) and its kin: dst is exactly a source."""
    for case in mb.case_names(func):
        g = gold(func, case)
        for alias in ("a", "b") if "b" in g else ("a",):
            check(func, case, dropin(dsp, torch_gpu, func, g, where, alias=alias), g)


@pytest.mark.gpu
def test_status_cases(dsp, torch_gpu):
    """Mismatched shapes, NULL, an out-of-range shift (dst keeps the marker) and zero dimensions, for the drop-ins
    and the batched forms."""
    torch, lib = torch_gpu, dsp.lib
    for t in VEC_TYPES:
        I = _abi.MAT_INST[t]
        a, d = Dev(torch, mb.rand(t, (2, 3, 5), np.random.default_rng(1))), Dev(torch, mb.marked(t, (2, 3, 5)))

        def m(r, c, h=a):
            return C.byref(I(r, c, C.cast(h.ptr if h is not None else None, _abi.MAT_PTR[t])))

        tails = ([], [2, None])
        for sfx, tail in zip(("", "_batch"), tails):
            if t != "q7":
                for op in ("add", "sub"):
                    fn = getattr(lib, f"arm_mat_{op}_{t}{sfx}")
                    assert fn(m(3, 5), m(3, 5), m(5, 3, d), *tail) == mb.SIZE_MISMATCH
                    assert fn(m(3, 5), m(3, 4), m(3, 5, d), *tail) == mb.SIZE_MISMATCH
                    assert fn(None, m(3, 5), m(3, 5, d), *tail) == mb.ARGUMENT_ERROR
                    assert fn(m(3, 5), m(3, 5, None), m(3, 5, d), *tail) == mb.ARGUMENT_ERROR
                    assert fn(m(0, 5), m(0, 5), m(0, 5, d), *tail) == mb.SUCCESS
                    assert fn(m(3, 0), m(3, 0), m(3, 0, d), *tail) == mb.SUCCESS
                sc = [1.5] if t == "f32" else [3, 0]
                fn = getattr(lib, f"arm_mat_scale_{t}{sfx}")
                assert fn(m(3, 5), *sc, m(3, 4, d), *tail) == mb.SIZE_MISMATCH
                assert fn(m(3, 5), *sc, None, *tail) == mb.ARGUMENT_ERROR
                assert fn(m(3, 5, None), *sc, m(3, 5, d), *tail) == mb.ARGUMENT_ERROR
                assert fn(m(0, 0), *sc, m(0, 0, d), *tail) == mb.SUCCESS
                if t != "f32":
                    lo, hi = mb.SHIFT_RANGE[t]
                    for shift in (lo - 1, hi + 1, -100, 100):
                        assert fn(m(3, 5), 3, shift, m(3, 5, d), *tail) == mb.ARGUMENT_ERROR
                fn = getattr(lib, f"arm_mat_cmplx_trans_{t}{sfx}")
                assert fn(m(3, 2), m(3, 2, d), *tail) == mb.SIZE_MISMATCH
                assert fn(m(3, 2), None, *tail) == mb.ARGUMENT_ERROR
                assert fn(m(0, 2), m(2, 0, d), *tail) == mb.SUCCESS
            fn = getattr(lib, f"arm_mat_trans_{t}{sfx}")
            assert fn(m(3, 5), m(3, 5, d), *tail) == mb.SIZE_MISMATCH
            assert fn(m(3, 5), m(5, 4, d), *tail) == mb.SIZE_MISMATCH
            assert fn(m(3, 5, None), m(5, 3, d), *tail) == mb.ARGUMENT_ERROR
            assert fn(m(3, 0), m(0, 3, d), *tail) == mb.SUCCESS
        # batch == 0
        assert getattr(lib, f"arm_mat_trans_{t}_batch")(m(3, 5), m(5, 3, d), 0, None) == mb.SUCCESS
        fb = getattr(lib, f"arm_mat_vec_mult_{t}_batch")
        assert fb(m(3, 5), 15, a.ptr, d.ptr, 0, None) == mb.SUCCESS
        assert fb(m(0, 5), 0, a.ptr, d.ptr, 2, None) == mb.SUCCESS
        for bad in (1, 14):
            assert fb(m(3, 5), bad, a.ptr, d.ptr, 2, None) == mb.ARGUMENT_ERROR
        assert fb(None, 0, a.ptr, d.ptr, 2, None) == mb.ARGUMENT_ERROR
        assert fb(m(3, 5), 0, None, d.ptr, 2, None) == mb.ARGUMENT_ERROR
        assert fb(m(3, 5), 0, a.ptr, None, 2, None) == mb.ARGUMENT_ERROR
        # the void drop-in: NULL does no work and sets the last-error string
        fv = getattr(lib, f"arm_mat_vec_mult_{t}")
        fv(m(3, 5), None, d.ptr)
        assert dsp.last_error()[0] != 0 and f"arm_mat_vec_mult_{t}" in dsp.last_error()[1]
        lib.arm_mi355x_clear_error()
        fv(m(0, 5), a.ptr, d.ptr)
        assert dsp.last_error()[0] == 0
        torch.cuda.synchronize()
        assert d.get().tobytes() == mb.marked(t, (2, 3, 5)).tobytes(), t          # nothing was written
        assert lib.arm_mi355x_last_error() == 0


# ------------------------------------------------------------------ GPU: element-wise shapes
EW_TEST_SHAPES = ((1, 1), (1, 3), (3, 5), (17, 31), (64, 64), (255, 257))


@pytest.mark.gpu
@pytest.mark.parametrize("func", EW)
def test_elementwise_shapes(dsp, torch_gpu, func):
    """Every shape with pData 16-B aligned (the vector path and its ragged end) and at element offset 1 (the
    scalar path), then a batch of 257 items of 3 x 5, also in place."""
    rng = np.random.default_rng(7)
    for shape in EW_TEST_SHAPES:
        g = ew_operands(func, shape, rng)
        want = mb.run(func, g)
        for off in (0, 1):
            check(func, (shape, off), dropin(dsp, torch_gpu, func, g, "device", off=off), want)
    g = ew_operands(func, (3, 5), rng, batch=257)
    want = mb.run(func, g)["dst"]
    for off in (0, 1):
        for alias in (False, True):
            a = Dev(torch_gpu, g["a"], off)
            b = Dev(torch_gpu, g["b"], off) if "b" in g else None
            d = a if alias else Dev(torch_gpu, mb.marked(a.t, g["a"].shape), off)
            st = call(dsp, func, (3, 5), a.ptr, b.ptr if b else None, d.ptr, scale=g["scale"].item() if "scale" in g
                      else None, shift=int(g.get("shift", 0)), batch=257)
            assert st == 0 and d.get().tobytes() == want.tobytes(), (func, off, alias)


@pytest.mark.gpu
def test_elementwise_saturation(dsp, torch_gpu):
    """q15 32767 + 1 and -32768 - 1, the q31 extremes, and scale at both ends of the shift range."""
    for t in ("q15", "q31"):
        i = np.iinfo(mb.DT[t])
        a = np.array([[i.max, i.min, i.max, i.min, 0, -1, 1, i.max - 1]], dtype=mb.DT[t])
        b = np.array([[1, -1, i.max, i.min, i.min, i.min, i.max, 1]], dtype=mb.DT[t])
        clip = lambda v: max(i.min, min(i.max, v))                               # noqa: E731
        got = dropin(dsp, torch_gpu, f"add_{t}", {"a": a, "b": b}, "device")["dst"]
        assert got.tolist() == [[clip(int(x) + int(y)) for x, y in zip(a[0], b[0])]]
        assert got[0, :4].tolist() == [i.max, i.min, i.max, i.min]
        bs = np.array([[-1, 1, i.min, i.max, i.max, i.max, i.min, -1]], dtype=mb.DT[t])
        got = dropin(dsp, torch_gpu, f"sub_{t}", {"a": a, "b": bs}, "device")["dst"]
        assert got.tolist() == [[clip(int(x) - int(y)) for x, y in zip(a[0], bs[0])]]
        assert got[0, :4].tolist() == [i.max, i.min, i.max, i.min]
        lo, hi = mb.SHIFT_RANGE[t]
        x = mb.extremes(t, (5, 9), np.random.default_rng(3))
        for shift in (lo, hi):
            for s in (i.max, i.min, 1, -1, 12345):
                g = {"a": x, "scale": mb.DT[t](s), "shift": np.int32(shift)}
                want = mb.run(f"scale_{t}", g)
                for where in ("device", "host"):
                    check(f"scale_{t}", (shift, s), dropin(dsp, torch_gpu, f"scale_{t}", g, where), want)


# ------------------------------------------------------------------ GPU: transposes
# packed below 257 elements, tiled above: 1x1 .. 3x5 and the batches are packed, the rest tiled (tiles of 32 for
# 4- and 8-byte elements, 64 for 1 and 2 bytes: 130x70 has ragged tiles on both axes in every size)
TRANS_TEST_SHAPES = ((1, 1), (1, 9), (9, 1), (3, 5), (16, 16), (31, 33), (32, 32), (33, 31), (64, 65), (7, 100),
                     (100, 7), (130, 70))


def trans_operand(func, shape, rng, batch=None):
    t = mb.split(func)[1]
    full = (shape[0], shape[1] * (2 if func.startswith("cmplx") else 1))
    return mb.rand(t, full if batch is None else (batch,) + full, rng)


def trans_want(func, a):
    f = mb.cmplx_trans if func.startswith("cmplx") else mb.trans
    return f(a) if a.ndim == 2 else np.stack([f(x) for x in a])


@pytest.mark.gpu
@pytest.mark.parametrize("func", TRANS)
def test_transpose_shapes(dsp, torch_gpu, func):
    """Every shape and element size (odd dimensions with q7 and q15 among them), pData aligned and at element
    offset 1 (q7: 1 and 3), outputs marker-filled with guard words after the end."""
    rng = np.random.default_rng(11)
    t = mb.split(func)[1]
    for shape in TRANS_TEST_SHAPES:
        a = trans_operand(func, shape, rng)
        want = {"status": 0, "dst": trans_want(func, a)}
        for off in (0, 1, 3) if t == "q7" else (0, 1):
            check(func, (shape, off), dropin(dsp, torch_gpu, func, {"a": a}, "device", off=off), want)
        check(func, shape, dropin(dsp, torch_gpu, func, {"a": a}, "host"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", TRANS)
def test_transpose_batches(dsp, torch_gpu, func):
    """1000 items of 4 x 4 and 257 of 5 x 3 (packed, the last workgroup partly filled), 5 of 40 x 50 (tiled)."""
    rng = np.random.default_rng(13)
    t = mb.split(func)[1]
    for batch, shape in ((1000, (4, 4)), (257, (5, 3)), (5, (40, 50))):
        a = trans_operand(func, shape, rng, batch)
        want = trans_want(func, a)
        for off in (0, 1):
            s, d = Dev(torch_gpu, a, off), Dev(torch_gpu, mb.marked(t, want.shape), off)
            assert call(dsp, func, shape, s.ptr, None, d.ptr, batch=batch) == 0
            assert d.get().tobytes() == want.tobytes(), (func, batch, shape, off)
            assert s.get().tobytes() == a.tobytes()


# ------------------------------------------------------------------ GPU: matrix x vector
VEC_TEST_SHAPES = ((1, 3), (3, 7), (4, 6), (5, 7), (9, 1), (8, 8), (64, 64), (65, 129), (130, 300), (258, 256))


def vec_operands(t, shape, rng, batch=None, shared=False):
    amp = mb.VEC_AMP.get(t)
    if shape == mb.BIG:
        amp = 15 if t == "q7" else amp                 # the q7 sums stay off the clip
    ms = shape if batch is None or shared else (batch,) + shape
    vs = shape[1] if batch is None else (batch, shape[1])
    return {"m": mb.rand(t, ms, rng, amp), "v": mb.rand(t, vs, rng, amp)}


@pytest.mark.gpu
@pytest.mark.parametrize("t", VEC_TYPES)
def test_vec_mult_shapes(dsp, torch_gpu, t):
    """Every shape on device pointers (aligned and at element offset 1) and on host pointers.  258 x 256: q15
    and q31 read rows 256 / 257 from the wrapped offset, so they repeat rows 0 / 1; f32 and q7 do not."""
    rng = np.random.default_rng(17)
    func = f"vec_mult_{t}"
    for shape in VEC_TEST_SHAPES:
        g = vec_operands(t, shape, rng)
        want = mb.run(func, g)
        for off in (0, 1):
            check(func, (shape, off), dropin(dsp, torch_gpu, func, g, "device", off=off), want)
        got = dropin(dsp, torch_gpu, func, g, "host")
        check(func, shape, got, want)
        if shape == mb.BIG:
            d = got["dst"]
            if t in ("q15", "q31"):
                assert d[256] == d[0] and d[257] == d[1]
            else:
                assert d[256] != d[0] and d[257] != d[1]
                assert t == "f32" or np.abs(d.astype(int)).max() < 127


@pytest.mark.gpu
def test_vec_mult_q15_pair_structure(dsp, torch_gpu):
    """The all-minimum cases, and one matrix whose equal rows give -32768 in the 4-row group (columns 4 and 5
    paired, the int32 pair sum wraps) and 32767 in the tail rows (added alone)."""
    for shape, word in (((4, 6), -32768), ((5, 7), -32768), ((3, 7), -32768), ((1, 3), 32767)):
        g = {"m": np.full(shape, -32768, dtype=np.int16), "v": np.full(shape[1], -32768, dtype=np.int16)}
        for where in ("host", "device"):
            assert (dropin(dsp, torch_gpu, "vec_mult_q15", g, where)["dst"] == word).all(), shape
    m, v = mb.pairwrap_case()
    d = dropin(dsp, torch_gpu, "vec_mult_q15", {"m": m, "v": v}, "device")["dst"]
    assert d.tolist() == [-32768] * 4 + [32767] * 3
    # the same with the pair in the last step of a long row (column step of 64)
    m2, v2 = np.zeros((7, 135), dtype=np.int16), np.zeros(135, dtype=np.int16)
    m2[:, 132:134], v2[132:134] = -32768, -32768
    g = {"m": m2, "v": v2}
    d = dropin(dsp, torch_gpu, "vec_mult_q15", g, "device")["dst"]
    assert d.tobytes() == mb.vec_mult("q15", m2, v2).tobytes() and d.tolist() == [-32768] * 4 + [32767] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("t", VEC_TYPES)
def test_vec_mult_batch(dsp, torch_gpu, t):
    """257 items with matStride 0 (one shared matrix), rows * cols and a padded stride; 3 items of 258 x 256,
    where the 16-bit offset wraps inside each item and the item bases do not."""
    rng = np.random.default_rng(19)
    func = f"vec_mult_{t}"
    for shape in ((5, 7), (4, 4), (33, 70)):
        rows, cols = shape
        for stride in (0, rows * cols, rows * cols + 5):
            batch = 257
            g = vec_operands(t, shape, rng, batch, shared=stride == 0)
            want = np.stack([mb.vec_mult(t, g["m"] if stride == 0 else g["m"][i], g["v"][i]) for i in range(batch)])
            mats = g["m"]
            if stride > rows * cols:
                mats = mb.marked(t, (batch, stride))
                mats[:, :rows * cols] = g["m"].reshape(batch, -1)
            m, v, d = Dev(torch_gpu, mats), Dev(torch_gpu, g["v"]), Dev(torch_gpu, mb.marked(t, (batch, rows)))
            assert call(dsp, func, shape, m.ptr, v.ptr, d.ptr, batch=batch, stride=stride) == 0
            assert d.get().tobytes() == want.tobytes(), (t, shape, stride)
    g = vec_operands(t, mb.BIG, rng, 3)
    want = np.stack([mb.vec_mult(t, g["m"][i], g["v"][i]) for i in range(3)])
    m, v, d = Dev(torch_gpu, g["m"]), Dev(torch_gpu, g["v"]), Dev(torch_gpu, mb.marked(t, (3, mb.BIG[0])))
    assert call(dsp, func, mb.BIG, m.ptr, v.ptr, d.ptr, batch=3, stride=mb.BIG[0] * mb.BIG[1]) == 0
    got = d.get()
    assert got.tobytes() == want.tobytes()
    if t in ("q15", "q31"):
        assert (got[:, 256] == got[:, 0]).all() and not (got[1] == got[0]).all()


# ------------------------------------------------------------------ GPU: f32 classes
@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["subnormal", "negzero", "signzero", "mixed", "overflow", "nonfinite"])
def test_f32_classes(dsp, torch_gpu, cls):
    """Subnormals, signed zeros, overflow to +-Inf and +-Inf / NaN inputs through add, sub, scale and vec_mult:
    finite inputs bit-equal, with non-finite inputs the non-NaN words bit-equal and the NaNs in place."""
    shape = (9, 37)
    pos = (3, 40, 200)
    a = f32_class_input(cls, shape, 23, scale=3.0e38, positions=pos)
    b = f32_class_input(cls, shape, 24, scale=3.0e38, positions=(3, 41, 201))
    for op in ("add", "sub"):
        g = {"a": a, "b": b}
        for where in ("host", "device"):
            assert_same_words(dropin(dsp, torch_gpu, f"{op}_f32", g, where)["dst"], mb.run(f"{op}_f32", g)["dst"],
                              f"{op} {cls} {where}")
    for s in (0.25, 4.0, -0.0) + ((np.inf,) if cls == "nonfinite" else ()):
        g = {"a": a, "scale": np.float32(s)}
        assert_same_words(dropin(dsp, torch_gpu, "scale_f32", g, "device")["dst"], mb.run("scale_f32", g)["dst"],
                          f"scale {cls} {s}")
    m = f32_class_input(cls, shape, 25, scale=1.0e19, positions=pos)
    v = f32_class_input(cls, shape[1], 26, scale=1.0e19, positions=(0, 5, 30))
    g = {"m": m, "v": v}
    want = mb.run("vec_mult_f32", g)["dst"]
    if cls == "overflow":
        assert np.isfinite(m).all() and np.isfinite(v).all()
    for where in ("host", "device"):
        assert_same_words(dropin(dsp, torch_gpu, "vec_mult_f32", g, where)["dst"], want, f"vec_mult {cls} {where}")


# ------------------------------------------------------------------ GPU: the Python layers
@pytest.mark.gpu
def test_python_wrappers(dsp, torch_gpu):
    """cmsisdsp's 20 names with the reference binding's conventions, and cmsisdsp_amd's batched forms on tensors."""
    import cmsisdsp as d
    torch = torch_gpu
    for func in mb.FUNCS:
        op, t = mb.split(func)
        case = mb.case_names(func)[1]
        g = gold(func, case)
        fn = getattr(d, "arm_mat_" + func)
        if op == "vec_mult":
            got = fn(g["m"], g["v"])
            assert isinstance(got, np.ndarray) and got.tobytes() == g["dst"].tobytes(), func
            continue
        args = [g["a"]] + ([g["b"]] if "b" in g else []) + ([g["scale"].item()] if "scale" in g else []) + \
            ([int(g["shift"])] if "shift" in g else [])
        st, got = fn(*args)
        assert st == 0 and got.dtype == g["dst"].dtype and got.shape == g["dst"].shape, func
        assert got.tobytes() == g["dst"].tobytes(), func
    st, got = d.arm_mat_scale_q15(np.ones((2, 2), dtype=np.int16), 5, 16)
    assert st == mb.ARGUMENT_ERROR and not got.any()
    rng = np.random.default_rng(29)
    dev = lambda x: torch.from_numpy(x).cuda()                                   # noqa: E731
    for t in mb.EW_TYPES:
        a, b = mb.rand(t, (6, 3, 5), rng), mb.rand(t, (6, 3, 5), rng)
        ta, tb, td = dev(a), dev(b), dev(mb.marked(t, a.shape))
        dsp.mat_add_batch(ta, tb, td)
        assert td.cpu().numpy().tobytes() == mb.add(t, a, b).tobytes()
        dsp.mat_sub_batch(ta, tb, ta)
        assert ta.cpu().numpy().tobytes() == mb.sub(t, a, b).tobytes()
        s = 0.5 if t == "f32" else 12345
        dsp.mat_scale_batch(tb, s, td, shift=1 if t != "f32" else 0)
        assert td.cpu().numpy().tobytes() == mb.scale(t, b, s, 1 if t != "f32" else 0).tobytes()
        c = mb.rand(t, (6, 3, 10), rng)
        tc = dev(mb.marked(t, (6, 5, 6)))
        dsp.mat_cmplx_trans_batch(dev(c), tc)
        assert tc.cpu().numpy().tobytes() == np.stack([mb.cmplx_trans(x) for x in c]).tobytes()
    for t in VEC_TYPES:
        a = mb.rand(t, (6, 3, 5), rng)
        td = dev(mb.marked(t, (6, 5, 3)))
        dsp.mat_trans_batch(dev(a), td)
        assert td.cpu().numpy().tobytes() == np.stack([x.T for x in a]).tobytes()
        g = vec_operands(t, (5, 7), rng, 6)
        to = dev(mb.marked(t, (6, 5)))
        dsp.mat_vec_mult_batch(dev(g["m"]), dev(g["v"]), to)
        want = np.stack([mb.vec_mult(t, g["m"][i], g["v"][i]) for i in range(6)])
        assert to.cpu().numpy().tobytes() == want.tobytes()
        dsp.mat_vec_mult_batch(dev(g["m"][0]), dev(g["v"]), to)
        want = np.stack([mb.vec_mult(t, g["m"][0], g["v"][i]) for i in range(6)])
        assert to.cpu().numpy().tobytes() == want.tobytes()
        with pytest.raises(RuntimeError):
            dsp.mat_vec_mult_batch(dev(g["m"]), dev(g["v"]), to, mat_stride=34)
