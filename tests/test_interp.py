"""arm_linear_interp_*, arm_bilinear_interp_* (f32, q31, q15, q7), arm_spline_init_f32 and arm_spline_f32, as drop-ins
and as _batch forms (cmsis-dsp_amd/csrc/interp.hip).

The checker is committed data: tests/golden/interp.npz holds the reference's own outputs (tools/make_golden_interp.py);
tests/interp_ref.py restates the functions in numpy, and the generator asserted it against the reference sample by
sample.  Every comparison is bit-exact; f32 NaNs are compared by position (f32_classes.assert_same_words).  The
expected word of a sample is the stored one; where interp_ref marks the sample as outside the reference's defined
behaviour (the cast of a NaN or of a value outside the int32_t range) it is the restatement's, which states the rule of
include/arm_math.h.  Samples are independent, so `count` samples are taken cyclically from a case's 520.

CPU: the fixture index, the restatement against every fixture, the exported symbols, the Python names, the struct
layouts, the scalar drop-ins (they run on the host) bit for bit on every linear and bilinear fixture.  GPU: see each
test."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import interp_ref as ir
from cmsisdsp_amd import _abi
from devbuf import Dev, marker, untouched
from f32_classes import assert_same_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "interp.npz"))
IDX = json.loads(str(GOLD["index"]))
F = np.float32
SUCCESS, ARGUMENT_ERROR = 0, -1
COUNTS = (1, 63, 64, 65, 4099)
BIG = 65535 * 64 + 2
STRUCTS = ("arm_linear_interp_instance_f32", "arm_bilinear_interp_instance_f32", "arm_bilinear_interp_instance_q31",
           "arm_bilinear_interp_instance_q15", "arm_bilinear_interp_instance_q7", "arm_spline_instance_f32")
FORBIDDEN = ("arm_sin_f32", "arm_cos_f32", "arm_sqrt_f32", "arm_atan2_f32", "arm_householder_f32", "arm_mat_qr_f32",
             "arm_minkowski_distance_f32", "arm_svm_sigmoid_predict_f32")


@pytest.fixture(autouse=True)
def no_stale_error(dsp):
    dsp.lib.arm_mi355x_clear_error()


def same(got, want, what):
    if np.asarray(want).dtype == np.float32:
        assert_same_words(got, want, what)
    else:
        assert np.array_equal(got, want), (what, np.flatnonzero(np.asarray(got) != np.asarray(want))[:5])


def linear_expected(name):
    """-> (kind, table, x, the expected words, the defined mask)"""
    kind, tab, x, defined = ir.linear_case(name)
    want = ir.linear_f32(tab, ir.X1, ir.SPACING, x) if kind == "f32" else ir.linear_q(kind, tab, x)
    return kind, tab, x, np.where(defined, GOLD[f"linear/{name}"], want), defined


def bilinear_expected(name):
    kind, tab, X, Y, defined = ir.bilinear_case(name)
    want = ir.bilinear_f32(tab, X, Y) if kind == "f32" else ir.bilinear_q(kind, tab, X, Y)
    return kind, tab, X, Y, np.where(defined, GOLD[f"bilinear/{name}"], want), defined


def spline_fixtures():
    """case -> (coeffs, temp, out) of the stored arrays."""
    out, pc, pt, po = {}, 0, 0, 0
    for name in IDX["spline"]:
        n, _, _, block = name.split("_")
        n, block = int(n), int(block)
        out[name] = (GOLD["spline/coeffs"][pc:pc + 3 * (n - 1)], GOLD["spline/temp"][pt:pt + 2 * n - 1],
                     GOLD["spline/out"][po:po + block])
        pc, pt, po = pc + 3 * (n - 1), pt + 2 * n - 1, po + block
    assert (pc, pt, po) == (GOLD["spline/coeffs"].size, GOLD["spline/temp"].size, GOLD["spline/out"].size)
    return out


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert IDX["linear"] == ir.linear_case_names() and IDX["bilinear"] == ir.bilinear_case_names()
    assert IDX["spline"] == ir.spline_case_names() and len(IDX["spline"]) == 160
    assert ir.LINEAR_SIZES["f32"] == (2, 3, 5, 4096, 16384, 16385) and ir.LINEAR_SIZES["q7"] == (2, 3, 4096)
    assert ir.BILINEAR_SHAPES == ((2, 2), (3, 5), (5, 3), (64, 67)) and ir.SPLINE_N == (2, 3, 4, 9, 65)
    assert ir.SPLINE_BLOCKS == (1, 20, 33, 257)
    for name in IDX["linear"]:
        kind, tab, x, defined = ir.linear_case(name)
        assert GOLD[f"linear/{name}"].shape == (ir.SAMPLES,) and GOLD[f"linear/{name}"].dtype == ir.NP[kind], name
        if kind == "f32":
            assert np.isnan(x).any() and np.isinf(x).any() and (x < ir.X1).any() and (x == ir.X1).any(), name
            assert 4 <= (~defined).sum() <= 8, name
        else:
            assert (x < 0).any() and ((x >> 20) == min(tab.size - 2, 2047)).any() and ((x >> 20) == 2047).any(), name
            assert (x == np.int32(-0x100000)).any(), name    # 0xFFF00000: index 4095 as an unsigned word
    for name in IDX["bilinear"]:
        kind, tab, X, Y, defined = ir.bilinear_case(name)
        got = GOLD[f"bilinear/{name}"]
        assert got.shape == (ir.SAMPLES,), name
        assert (got[defined] != 0).sum() * 4 >= defined.sum() or tab.shape == (2, 2), name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "interp.npz")) < 128 << 10


def test_restatement_equals_every_fixture():
    for k, name in enumerate(IDX["linear"]):
        kind, tab, x, want, defined = linear_expected(name)
        assert ir.crc(tab, x) == int(GOLD["crc/linear"][k]), name
        got = ir.linear_f32(tab, ir.X1, ir.SPACING, x) if kind == "f32" else ir.linear_q(kind, tab, x)
        same(got[defined], GOLD[f"linear/{name}"][defined], name)
    for k, name in enumerate(IDX["bilinear"]):
        kind, tab, X, Y, want, defined = bilinear_expected(name)
        assert ir.crc(tab, X, Y) == int(GOLD["crc/bilinear"][k]), name
        got = ir.bilinear_f32(tab, X, Y) if kind == "f32" else ir.bilinear_q(kind, tab, X, Y)
        same(got[defined], GOLD[f"bilinear/{name}"][defined], name)
    fx = spline_fixtures()
    for k, name in enumerate(IDX["spline"]):
        t, x, y, xq = ir.spline_case(name)
        assert ir.crc(x, y, xq) == int(GOLD["crc/spline"][k]), name
        coeffs, temp = ir.spline_init(t, x, y)
        same(coeffs, fx[name][0], name + " coeffs")
        same(temp, fx[name][1], name + " temp")
        same(ir.spline_eval(x, y, coeffs, xq), fx[name][2], name)


def test_library_exports_the_symbols(dsp):
    names = set(_abi.INTERP)
    assert len(names) == 20 and sum(n.endswith("_batch") for n in names) == 10
    out = subprocess.run(["nm", "-D", "--defined-only", dsp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names <= exported
    assert not any(s in exported for s in FORBIDDEN)
    arm = {s for s in exported if s.startswith("arm_")}      # not the compiler's own symbols, whose names carry hashes
    assert not any(s.startswith("arm_levinson_durbin") or s.endswith("_to_f64") or "f16" in s for s in arm)
    for header, batch in (("arm_math.h", False), ("arm_math_mi355x.h", True)):
        text = open(os.path.join(ROOT, "include", header)).read()
        for n in names:
            if n.endswith("_batch") == batch:
                assert f" {n}(" in text, (header, n)


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for n in _abi.INTERP:
        if not n.endswith("_batch"):
            assert "cmsis_" + n in getattr(d, n).__doc__, n
    for n in STRUCTS:
        assert isinstance(getattr(d, n), type), n
    S = d.arm_linear_interp_instance_f32(nValues=3, x1=0.5, xSpacing=0.25, pYData=[1.0, 2.0, 4.0])
    assert (S.nValues(), S.x1(), S.xSpacing()) == (3, 0.5, 0.25)
    assert d.arm_linear_interp_f32(S, 0.625) == 1.5 and d.arm_linear_interp_f32(S, 9.0) == 4.0
    B = d.arm_bilinear_interp_instance_q15(numRows=2, numCols=2, pData=[0, 16384, 16384, 32767])
    assert (B.numRows(), B.numCols()) == (2, 2) and d.arm_bilinear_interp_q15(B, 1 << 19, 0) == 8191
    assert d.arm_linear_interp_q7([0, 64], 1 << 19, 2) == 32
    assert not hasattr(d, "arm_linear_interp_f16")
    for n in ("linear_interp_instance", "bilinear_interp_instance", "arm_linear_interp", "arm_bilinear_interp",
              "arm_spline_f32", "linear_interp_batch", "bilinear_interp_batch", "spline_init_batch", "spline_batch"):
        assert callable(getattr(dsp, n)), n


def test_struct_layouts_match_the_reference(tmp_path):
    """tools/abi_layout_interp.c compiled against include/ prints what it printed when compiled against the
    reference's headers (tests/golden/abi_layout_interp.json); the ctypes mirrors agree."""
    exe = str(tmp_path / "abi_layout_interp")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "abi_layout_interp.c"),
                    "-o", exe], check=True)
    mine = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_layout_interp.json")))
    assert mine == ref and set(ref) == set(STRUCTS) | {"arm_spline_type"}
    for name in STRUCTS:
        st = getattr(_abi, name)
        assert C.sizeof(st) == ref[name]["size"], name
        assert {f: getattr(st, f).offset for f, _ in st._fields_} == {k: v for k, v in ref[name].items() if k != "size"}


def test_scalar_drop_ins_equal_every_fixture(dsp):
    """The one-sample drop-ins run on the host: every linear and bilinear fixture, bit for bit."""
    lib = dsp.lib
    for name in IDX["linear"]:
        kind, tab, x, want, _ = linear_expected(name)
        if kind == "f32":
            S, keep = dsp.linear_interp_instance(ir.X1, ir.SPACING, tab)
            got = np.array([lib.arm_linear_interp_f32(C.byref(S), float(v)) for v in x], dtype=F)
        else:
            fn = getattr(lib, f"arm_linear_interp_{kind}")
            got = np.array([fn(tab.ctypes.data, int(v), tab.size) for v in x], dtype=ir.NP[kind])
        same(got, want, name)
    for name in IDX["bilinear"]:
        kind, tab, X, Y, want, _ = bilinear_expected(name)
        S, keep = dsp.bilinear_interp_instance(kind, tab)
        fn, conv = getattr(lib, f"arm_bilinear_interp_{kind}"), float if kind == "f32" else int
        got = np.array([fn(C.byref(S), conv(a), conv(b)) for a, b in zip(X, Y)], dtype=ir.NP[kind])
        same(got, want, name)
    assert dsp.last_error()[0] == 0
    # refusals: 0 (a NaN from the f32 forms) and the last error
    tab = np.arange(4, dtype=F)
    S = _abi.arm_linear_interp_instance_f32(0, 0.0, 1.0, tab.ctypes.data)
    assert np.isnan(lib.arm_linear_interp_f32(C.byref(S), 1.0)) and dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()
    assert lib.arm_linear_interp_q15(None, 0, 4) == 0 and dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()
    assert lib.arm_linear_interp_q31(tab.ctypes.data, 0, 0) == 0 and dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()
    B = _abi.arm_bilinear_interp_instance(65535, 65535, tab.ctypes.data)       # numRows * numCols >= 2^31
    assert lib.arm_bilinear_interp_q7(C.byref(B), 0, 0) == 0 and dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()
    assert np.isnan(lib.arm_bilinear_interp_f32(None, 0.0, 0.0)) and dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()


# ------------------------------------------------------------------ GPU
def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def linear_call(dsp, torch, kind, tab, x, offs=(0, 0, 0), n_values=None):
    """-> (status, y or the untouched marker); asserts the sources unchanged and the guards intact."""
    dt, dx = Dev(torch, tab, offs[0]), Dev(torch, x, offs[1])
    dy = Dev(torch, marker(x.shape, ir.NP[kind]), offs[2])
    n_values = tab.size if n_values is None else n_values
    if kind == "f32":
        S = _abi.arm_linear_interp_instance_f32(n_values, float(ir.X1), float(ir.SPACING), dt.ptr)
        status = dsp.lib.arm_linear_interp_f32_batch(C.byref(S), dx.ptr, dy.ptr, x.size, stream_of(torch))
    else:
        status = getattr(dsp.lib, f"arm_linear_interp_{kind}_batch")(dt.ptr, n_values, dx.ptr, dy.ptr, x.size,
                                                                     stream_of(torch))
    torch.cuda.synchronize()
    assert dt.get().tobytes() == tab.tobytes() and dx.get().tobytes() == x.tobytes(), "a source changed"
    return status, dy.get()


def bilinear_call(dsp, torch, kind, tab, X, Y, offs=(0, 0, 0, 0), shape=None):
    dt, dX, dY = Dev(torch, tab, offs[0]), Dev(torch, X, offs[1]), Dev(torch, Y, offs[2])
    do = Dev(torch, marker(X.shape, ir.NP[kind]), offs[3])
    rows, cols = tab.shape if shape is None else shape
    S = _abi.arm_bilinear_interp_instance(rows, cols, dt.ptr)
    status = getattr(dsp.lib, f"arm_bilinear_interp_{kind}_batch")(C.byref(S), dX.ptr, dY.ptr, do.ptr, X.size,
                                                                   stream_of(torch))
    torch.cuda.synchronize()
    assert dt.get().tobytes() == tab.tobytes() and dX.get().tobytes() == X.tobytes() and \
        dY.get().tobytes() == Y.tobytes(), "a source changed"
    return status, do.get()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ir.linear_case_names())
def test_linear_batch(dsp, torch_gpu, name):
    """Tables of 2, 3 (5) and 4096 values in LDS and, for f32, 16384 values (the 64 KiB limit, still in LDS) and 16385
    values from global memory; 1 .. 4099 samples below,
    at and above the range, on the knots, in the last interval, negative 12.20 words; every operand one element off
    16-byte alignment."""
    kind, tab, x, want, _ = linear_expected(name)
    assert dsp.lib is not None and (tab.size * tab.itemsize <= 65536) == (name != "f32_16385")
    for count in COUNTS:
        pick = np.arange(count) % ir.SAMPLES
        status, got = linear_call(dsp, torch_gpu, kind, tab, x[pick])
        assert status == SUCCESS, (name, count)
        same(got, want[pick], f"{name} count={count}")
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        status, got = linear_call(dsp, torch_gpu, kind, tab, x[:65], offs)
        assert status == SUCCESS, (name, offs)
        same(got, want[:65], f"{name} offs={offs}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ir.bilinear_case_names())
def test_bilinear_batch(dsp, torch_gpu, name):
    """Tables 2 x 2, 3 x 5, 5 x 3 and 64 x 67; points inside, on the last row and column, negative, NaN and +-Inf."""
    kind, tab, X, Y, want, _ = bilinear_expected(name)
    for count in COUNTS:
        pick = np.arange(count) % ir.SAMPLES
        status, got = bilinear_call(dsp, torch_gpu, kind, tab, X[pick], Y[pick])
        assert status == SUCCESS, (name, count)
        same(got, want[pick], f"{name} count={count}")
    for offs in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
        status, got = bilinear_call(dsp, torch_gpu, kind, tab, X[:65], Y[:65], offs)
        assert status == SUCCESS, (name, offs)
        same(got, want[:65], f"{name} offs={offs}")


def spline_items(n, batch, block, qkind, shared_x, shared_q):
    """-> (x [batch or 1, n], y [batch, n], xq [batch or 1, block]) of `batch` distinct items."""
    xs, ys, qs = [], [], []
    for i in range(batch):
        x, _ = ir.spline_knots(n, 0 if shared_x else i)
        _, y = ir.spline_knots(n, i)
        xs.append(x)
        ys.append(y)
        qs.append(ir.spline_queries(qkind, xs[0] if shared_q else x, block, 0 if shared_q else i))
    return np.stack(xs[:1] if shared_x else xs), np.stack(ys), np.stack(qs[:1] if shared_q else qs)


def strided(rows, stride):
    """The rows at a distance of `stride` elements (0: the one row), marker bytes between them."""
    if stride == 0:
        return rows[0].copy()
    flat = marker(((rows.shape[0] - 1) * stride + rows.shape[1],), rows.dtype)
    for i, r in enumerate(rows):
        flat[i * stride:i * stride + r.size] = r
    return flat


def spline_call(dsp, torch, t, x, x_stride, y, xq, q_stride, off=0):
    """init and evaluation through the _batch forms -> (coeffs, temp, out), each [batch, ...]."""
    batch, n = y.shape
    block = xq.shape[-1]
    dx, dy, dq = Dev(torch, strided(x, x_stride), off), Dev(torch, y, off), Dev(torch, strided(xq, q_stride), off)
    dc, dt = Dev(torch, marker((batch, 3 * (n - 1)), F), off), Dev(torch, marker((batch, 2 * n - 1), F), off)
    do = Dev(torch, marker((batch, block), F), off)
    st = stream_of(torch)
    assert dsp.lib.arm_spline_init_f32_batch(t, dx.ptr, x_stride, dy.ptr, n, dc.ptr, dt.ptr, batch, st) == SUCCESS
    assert dsp.lib.arm_spline_f32_batch(dx.ptr, x_stride, dy.ptr, dc.ptr, n, dq.ptr, q_stride, do.ptr, block, batch,
                                        st) == SUCCESS
    torch.cuda.synchronize()
    assert dy.get().tobytes() == y.tobytes() and dx.get().tobytes() == strided(x, x_stride).tobytes()
    assert dq.get().tobytes() == strided(xq, q_stride).tobytes(), "a source changed"
    return dc.get(), dt.get(), do.get()


@pytest.mark.gpu
@pytest.mark.parametrize("n", ir.SPLINE_N)
def test_spline_equals_every_fixture(dsp, torch_gpu, n):
    """n = 2, 3, 4, 9, 65, both types, blockSize 1, 20, 33, 257, queries sorted (below x[0] and above x[n - 1]
    included), on knots, unsorted and with a NaN in the middle: the stored words, through the _batch forms at batch 1
    and through the drop-ins on host pointers."""
    fx = spline_fixtures()
    for name in IDX["spline"]:
        if int(name.split("_")[0]) != n:
            continue
        t, x, y, xq = ir.spline_case(name)
        coeffs, temp, out = spline_call(dsp, torch_gpu, t, x[None], 0, y[None], xq[None], 0,
                                        off=name.endswith("_33"))
        same(coeffs[0], fx[name][0], name + " coeffs")
        same(temp[0], fx[name][1], name + " temp")
        same(out[0], fx[name][2], name)
        if name.endswith("_20"):
            h_out, h_coeffs, h_temp = dsp.arm_spline_f32(t, x, y, xq)
            same(h_coeffs, fx[name][0], name + " drop-in coeffs")
            same(h_temp, fx[name][1], name + " drop-in temp")
            same(h_out, fx[name][2], name + " drop-in")


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (1, 3, 65, 257))
def test_spline_batch(dsp, torch_gpu, batch):
    """Independent items (one lane each in init, one wave each in the evaluation; 257 items are more than one
    workgroup of either), strides 0 and the item length + 3, against the restatement item by item."""
    for n, block, qkind in ((4, 33, "unsorted"), (9, 257, "nan"), (9, 20, "knots")):
        for t in (0, 1):
            for shared in (False, True):
                x, y, xq = spline_items(n, batch, block, qkind, shared, shared)
                xs, qs = (0, 0) if shared else (n + 3, block + 3)
                coeffs, temp, out = spline_call(dsp, torch_gpu, t, x, xs, y, xq, qs, off=1)
                for i in range(batch):
                    xi, qi = x[0 if shared else i], xq[0 if shared else i]
                    wc, wt = ir.spline_init(t, xi, y[i])
                    same(coeffs[i], wc, f"coeffs n={n} item {i}")
                    same(temp[i], wt, f"temp n={n} item {i}")
                    same(out[i], ir.spline_eval(xi, y[i], wc, qi), f"out n={n} item {i}")


@pytest.mark.gpu
def test_refusals_write_nothing(dsp, torch_gpu):
    torch = torch_gpu
    lib, st = dsp.lib, stream_of(torch_gpu)
    for name in ("f32_5", "q31_3", "q15_3", "q7_3"):
        kind, tab, x, want, _ = linear_expected(name)
        status, got = linear_call(dsp, torch, kind, tab, x[:65], n_values=0)
        assert status == ARGUMENT_ERROR and untouched(got), name
        dt, dx = Dev(torch, tab), Dev(torch, x[:65])
        dy = Dev(torch, marker((65,), ir.NP[kind]))
        if kind == "f32":
            S = _abi.arm_linear_interp_instance_f32(tab.size, float(ir.X1), float(ir.SPACING), dt.ptr)
            call = lambda t, a, b, cnt: lib.arm_linear_interp_f32_batch(                       # noqa: E731
                C.byref(_abi.arm_linear_interp_instance_f32(tab.size, float(ir.X1), float(ir.SPACING), t)), a, b, cnt, st)
            assert lib.arm_linear_interp_f32_batch(None, dx.ptr, dy.ptr, 65, st) == ARGUMENT_ERROR
        else:
            call = lambda t, a, b, cnt: getattr(lib, f"arm_linear_interp_{kind}_batch")(t, tab.size, a, b, cnt, st)  # noqa: E731
        assert call(None, dx.ptr, dy.ptr, 65) == ARGUMENT_ERROR and call(dt.ptr, None, dy.ptr, 65) == ARGUMENT_ERROR
        assert call(dt.ptr, dx.ptr, None, 65) == ARGUMENT_ERROR and call(dt.ptr, dx.ptr, dy.ptr, 0) == SUCCESS
        assert dsp.last_error()[0] == 0, name
        if kind in ("f32", "q31"):                           # the result over the samples, one element on
            before = dx.get().copy()
            assert call(dt.ptr, dx.ptr, dx.ptr + 4, 64) == ARGUMENT_ERROR
            torch.cuda.synchronize()
            assert dx.get().tobytes() == before.tobytes() and dsp.last_error()[0] != 0
            lib.arm_mi355x_clear_error()
        torch.cuda.synchronize()
        assert untouched(dy.get()), name
    for name in ("f32_3x5", "q31_3x5", "q15_5x3", "q7_5x3"):
        kind, tab, X, Y, want, _ = bilinear_expected(name)
        status, got = bilinear_call(dsp, torch, kind, tab, X[:65], Y[:65], shape=(65535, 65535))
        assert status == ARGUMENT_ERROR and untouched(got), name
        fn = getattr(lib, f"arm_bilinear_interp_{kind}_batch")
        dt, dX, dY = Dev(torch, tab), Dev(torch, X[:65]), Dev(torch, Y[:65])
        do = Dev(torch, marker((65,), ir.NP[kind]))
        S = _abi.arm_bilinear_interp_instance(tab.shape[0], tab.shape[1], dt.ptr)
        N = _abi.arm_bilinear_interp_instance(tab.shape[0], tab.shape[1], None)
        assert fn(None, dX.ptr, dY.ptr, do.ptr, 65, st) == ARGUMENT_ERROR
        assert fn(C.byref(N), dX.ptr, dY.ptr, do.ptr, 65, st) == ARGUMENT_ERROR
        assert fn(C.byref(S), None, dY.ptr, do.ptr, 65, st) == ARGUMENT_ERROR
        assert fn(C.byref(S), dX.ptr, None, do.ptr, 65, st) == ARGUMENT_ERROR
        assert fn(C.byref(S), dX.ptr, dY.ptr, None, 65, st) == ARGUMENT_ERROR
        assert fn(C.byref(S), dX.ptr, dY.ptr, do.ptr, 0, st) == SUCCESS
        torch.cuda.synchronize()
        assert untouched(do.get()) and dsp.last_error()[0] == 0, name
    # spline
    x, y, xq = spline_items(4, 3, 20, "sorted", False, False)
    dx, dy, dq = Dev(torch, x), Dev(torch, y), Dev(torch, xq)
    dc, dt, do = Dev(torch, marker((3, 9), F)), Dev(torch, marker((3, 7), F)), Dev(torch, marker((3, 20), F))
    init, ev = lib.arm_spline_init_f32_batch, lib.arm_spline_f32_batch
    assert init(0, dx.ptr, 4, dy.ptr, 1, dc.ptr, dt.ptr, 3, st) == ARGUMENT_ERROR          # n < 2
    assert init(0, dx.ptr, 4, dy.ptr, 0, dc.ptr, dt.ptr, 3, st) == ARGUMENT_ERROR
    assert init(2, dx.ptr, 4, dy.ptr, 4, dc.ptr, dt.ptr, 3, st) == ARGUMENT_ERROR          # no such type
    assert init(0, dx.ptr, 3, dy.ptr, 4, dc.ptr, dt.ptr, 3, st) == ARGUMENT_ERROR          # a stride below n
    assert init(0, None, 4, dy.ptr, 4, dc.ptr, dt.ptr, 3, st) == ARGUMENT_ERROR
    assert init(0, dx.ptr, 4, dy.ptr, 4, None, dt.ptr, 3, st) == ARGUMENT_ERROR
    assert init(0, dx.ptr, 4, dy.ptr, 4, dc.ptr, None, 3, st) == ARGUMENT_ERROR
    assert init(0, dx.ptr, 4, dy.ptr, 4, dc.ptr, dt.ptr, 0, st) == SUCCESS
    assert ev(dx.ptr, 4, dy.ptr, dc.ptr, 1, dq.ptr, 20, do.ptr, 20, 3, st) == ARGUMENT_ERROR
    assert ev(dx.ptr, 3, dy.ptr, dc.ptr, 4, dq.ptr, 20, do.ptr, 20, 3, st) == ARGUMENT_ERROR
    assert ev(dx.ptr, 4, dy.ptr, dc.ptr, 4, dq.ptr, 19, do.ptr, 20, 3, st) == ARGUMENT_ERROR
    assert ev(dx.ptr, 4, dy.ptr, dc.ptr, 4, dq.ptr, 20, None, 20, 3, st) == ARGUMENT_ERROR
    assert ev(dx.ptr, 4, dy.ptr, dc.ptr, 4, dq.ptr, 20, do.ptr, 0, 3, st) == SUCCESS
    assert ev(dx.ptr, 4, dy.ptr, dc.ptr, 4, dq.ptr, 20, do.ptr, 20, 0, st) == SUCCESS
    assert dsp.last_error()[0] == 0
    assert ev(dx.ptr, 4, dy.ptr, dc.ptr, 4, dq.ptr, 20, dq.ptr, 20, 3, st) == ARGUMENT_ERROR     # the result over xq
    assert init(0, dx.ptr, 4, dy.ptr, 4, dy.ptr, dt.ptr, 3, st) == ARGUMENT_ERROR                # coeffs over y
    assert dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()
    torch.cuda.synchronize()
    assert untouched(dc.get()) and untouched(dt.get()) and untouched(do.get())
    assert dq.get().tobytes() == xq.tobytes() and dy.get().tobytes() == y.tobytes()
    # the drop-ins are void: a refusal is the last error
    S = _abi.arm_spline_instance_f32()
    hx, hy, hc, ht = x[0].copy(), y[0].copy(), marker((9,), F), marker((7,), F)
    lib.arm_spline_init_f32(C.byref(S), 0, hx.ctypes.data, hy.ctypes.data, 1, hc.ctypes.data, ht.ctypes.data)
    assert dsp.last_error()[0] != 0 and untouched(hc) and untouched(ht) and not S.x
    lib.arm_mi355x_clear_error()
    lib.arm_spline_init_f32(C.byref(S), 0, hx.ctypes.data, None, 4, hc.ctypes.data, ht.ctypes.data)
    assert dsp.last_error()[0] != 0 and untouched(hc)
    lib.arm_mi355x_clear_error()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ir.KINDS)
def test_linear_and_bilinear_past_a_16_bit_grid(dsp, torch_gpu, kind):
    """One call per kernel with more samples than 65,535 blocks of 64 hold."""
    torch = torch_gpu
    tdt = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16, "q7": torch.int8}[kind]
    reps = -(-BIG // ir.SAMPLES)
    big = lambda v: np.tile(v, reps)[:BIG]                   # noqa: E731
    _, tab, x, want, _ = linear_expected(f"{kind}_3")
    t, dx = torch.from_numpy(tab).cuda(), torch.from_numpy(big(x)).cuda()
    out = torch.zeros(BIG + 8, dtype=tdt, device="cuda")
    arg = dsp.linear_interp_instance(ir.X1, ir.SPACING, t)[0] if kind == "f32" else t
    dsp.linear_interp_batch(kind, arg, dx, out[:BIG])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[BIG:] == 0).all()
    same(got[:BIG], big(want), f"linear {kind}")
    _, tab, X, Y, want, _ = bilinear_expected(f"{kind}_3x5")
    S, keep = dsp.bilinear_interp_instance(kind, torch.from_numpy(tab).cuda())
    dX, dY = torch.from_numpy(big(X)).cuda(), torch.from_numpy(big(Y)).cuda()
    out.zero_()
    dsp.bilinear_interp_batch(kind, S, dX, dY, out[:BIG])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[BIG:] == 0).all()
    same(got[:BIG], big(want), f"bilinear {kind}")


@pytest.mark.gpu
def test_spline_past_a_16_bit_grid(dsp, torch_gpu):
    """More items than 65,535 blocks of 64 hold, through both spline kernels: 2 knots, 1 query, 7 distinct items."""
    torch = torch_gpu
    x, _ = ir.spline_knots(2)
    ys = np.stack([ir.spline_knots(2, i)[1] for i in range(7)])
    xq = np.array([x[0] + F(0.25)], dtype=F)
    reps = -(-BIG // 7)
    y = np.tile(ys, (reps, 1))[:BIG]
    dx, dy, dq = (torch.from_numpy(a).cuda() for a in (x, y, xq))
    coeffs = torch.zeros((BIG + 2, 3), dtype=torch.float32, device="cuda")
    temp = torch.zeros((BIG + 2, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros((BIG + 2, 1), dtype=torch.float32, device="cuda")
    for t in (0, 1):
        dsp.spline_init_batch(t, dx, dy, coeffs[:BIG], temp[:BIG])
        dsp.spline_batch(dx, dy, coeffs[:BIG], dq, out[:BIG])
        torch.cuda.synchronize()
        wc, wt, wo = [], [], []
        for i in range(7):
            c, tp = ir.spline_init(t, x, ys[i])
            wc.append(c)
            wt.append(tp)
            wo.append(ir.spline_eval(x, ys[i], c, xq))
        tile = lambda w: np.tile(np.stack(w), (reps, 1))[:BIG]          # noqa: E731
        gc, gt, go = coeffs.cpu().numpy(), temp.cpu().numpy(), out.cpu().numpy()
        assert (gc[BIG:] == 0).all() and (gt[BIG:] == 0).all() and (go[BIG:] == 0).all()
        same(gc[:BIG], tile(wc), f"coeffs type {t}")
        same(gt[:BIG], tile(wt), f"temp type {t}")
        same(go[:BIG], tile(wo), f"out type {t}")


@pytest.mark.gpu
def test_table_written_on_the_calls_stream(dsp, torch_gpu):
    """The tables hold other valid words until the call's own stream, behind a device-side delay, writes the true ones
    immediately before the call: the LDS-staged linear table, the one read from global memory, the bilinear table."""
    torch = torch_gpu
    cases = []
    for name in ("f32_4096", "f32_16385"):
        _, tab, x, want, _ = linear_expected(name)
        pick = np.arange(4099) % ir.SAMPLES
        cases.append(("linear", tab, (x[pick],), want[pick]))
    _, tab, X, Y, want, _ = bilinear_expected("f32_64x67")
    cases.append(("bilinear", tab, (X[pick], Y[pick]), want[pick]))
    side = torch.cuda.Stream()
    work = []
    for what, tab, xs, want in cases:
        true = torch.from_numpy(tab).cuda()
        t = torch.from_numpy(np.ascontiguousarray(tab.reshape(-1)[::-1]).reshape(tab.shape).copy()).cuda()
        out = torch.full((4099,), float("nan"), dtype=torch.float32, device="cuda")
        work.append((what, true, t, [torch.from_numpy(v).cuda() for v in xs], out, want))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)
        for what, true, t, xs, out, want in work:
            t.copy_(true)
            if what == "linear":
                dsp.linear_interp_batch("f32", dsp.linear_interp_instance(ir.X1, ir.SPACING, t)[0], xs[0], out,
                                        stream=side)
            else:
                dsp.bilinear_interp_batch("f32", dsp.bilinear_interp_instance("f32", t)[0], xs[0], xs[1], out,
                                          stream=side)
        busy = not side.query()
    side.synchronize()
    assert busy, "the delay ended before the calls were enqueued: the check showed nothing"
    for what, true, t, xs, out, want in work:
        assert_same_words(out.cpu().numpy(), want, what)
