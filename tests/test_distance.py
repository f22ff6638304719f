"""The distance functions: eight f32 distances, nine boolean distances on packed words, arm_dtw_init_window_q7,
arm_dtw_distance_f32 and arm_dtw_path_f32, each as a drop-in and as a _batch form (cmsis-dsp_amd/csrc/distance.hip).

The checker is committed data: tests/golden/distance.npz holds the reference's own outputs between guard words
(tools/make_golden_distance.py); tests/distance_ref.py restates the functions in numpy / Python ints, and the
generator asserted it against the reference case by case.  Every comparison is bit-exact; a NaN result is compared by
being a NaN (the rule of tests/test_f32_classes.py).  The jensenshannon tests skip where the host's logf is not the
one csrc/host_logf.hpp restates.

CPU: the fixture index, the restatement against every fixture, the probed facts, the exported symbols, the Python
names.  GPU: every function through its _batch form and its drop-in against every fixture; batches either side of
kSumLaneMinBatch (f32) and of every lanes-per-item step (boolean); bStride / wStride 0, the item size and the item
size + 3; every pointer in turn one element off 16-byte alignment; marker bytes around every device buffer; the
sources unchanged; the correlation drop-in's shifted words; every refusal writing nothing; batch == 0."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import mfcc_cfg
from cmsisdsp_amd import _abi
from f32_classes import assert_same_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "distance.npz"))
IDX = json.loads(str(GOLD["index"]))
F = np.float32
SUCCESS, ARGUMENT_ERROR = 0, -1
GUARD = 32                     # marker bytes after the end of every device buffer
SUM_LANE_MIN_BATCH = 4096      # kSumLaneMinBatch of chain_f32.hpp: from here on one lane per f32 item
MARK_BYTES = np.asarray(dr.MARK).tobytes()


def unguard(v):
    v = np.asarray(v)
    assert v[..., :1].tobytes() == MARK_BYTES * (v.size // 3) and v[..., -1:].tobytes() == MARK_BYTES * (v.size // 3)
    return v[..., 1]


def f32_expected(func):
    """case -> the reference's result word."""
    return dict(zip(IDX["f32"], unguard(GOLD[f"f32/{func}/value"])))


def bool_expected(func):
    return dict(zip(IDX["bool"], unguard(GOLD[f"bool/{func}/value"])))


def needs_host_logf(func):
    if func == "jensenshannon" and not mfcc_cfg.host_libm_status()[0]:
        pytest.skip("host libm differs: the recorded jensenshannon words are another logf's")


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert IDX["f32"] == dr.f32_case_names() and IDX["bool"] == dr.bool_case_names()
    assert IDX["dtw"] == dr.dtw_case_names()
    assert IDX["f32"][:22] == [f"rand_{n}" for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257,
                                                     1023, 1025, 4097, 33000)]
    assert {dr.bool_case_n(c) for c in IDX["bool"]} == {0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1023,
                                                        1025, 4097, 33000, 200000, (1 << 25) + 33}
    assert IDX["empty"] == {f: ("refused" if f == "chebyshev" else "value") for f in dr.F32_FUNCS}
    assert len(IDX["win"]) == 6 * len(dr.DTW_SHAPES) and int(GOLD["win/status"][0]) == ARGUMENT_ERROR
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "distance.npz"))
    assert size < 1 << 20


def test_restatement_equals_every_fixture():
    logf_ok = mfcc_cfg.host_libm_status()[0]
    pos = {"f32": 0, "js": 0}
    for func in dr.F32_FUNCS:
        want = f32_expected(func)
        for k, case in enumerate(IDX["f32"]):
            a, b = dr.f32_operands(func, case)
            assert dr.crc(a, b) == int(GOLD[f"f32/{func}/crc"][k]), (func, case, "operands")
            g = "js" if func == "jensenshannon" else "f32"
            if a.size <= dr.STORE_MAX and func in ("braycurtis", "jensenshannon"):
                for key, x in (("a", a), ("b", b)):
                    assert GOLD[f"f32ops/{g}/{key}"][pos[g]:pos[g] + x.size].tobytes() == x.tobytes(), (func, case)
                pos[g] += a.size
            if func == "jensenshannon" and not logf_ok:
                continue
            got = dr.distance_f32(func, a, b)
            if func == "correlation":
                got, sa, sb = got
                z = lambda x: np.where(np.isnan(x), F(0), x)                    # noqa: E731
                assert dr.crc(z(sa), z(sb)) == int(GOLD["f32/correlation/shift"][k]), case
            assert dr.same_word(got, want[case]), (func, case, got, want[case])
        if func != "chebyshev":
            got = dr.distance_f32(func, np.zeros(0, F), np.zeros(0, F))
            assert dr.same_word(got[0] if func == "correlation" else got, unguard(GOLD[f"f32/{func}/empty"])), func
    bpos = 0
    want = {f: bool_expected(f) for f in dr.BOOL_FUNCS}
    for k, case in enumerate(IDX["bool"]):
        a, b, n = dr.bool_operands(case)
        assert dr.crc(a, b) == int(GOLD["bool/crc"][k]), case
        if a.size <= dr.STORE_MAX:
            assert GOLD["bool/a"][bpos:bpos + a.size].tobytes() == a.tobytes(), case
            assert GOLD["bool/b"][bpos:bpos + a.size].tobytes() == b.tobytes(), case
            bpos += a.size
        counts = dr.bool_counts(a, b, n)
        for func in dr.BOOL_FUNCS:
            assert dr.same_word(dr.bool_finish(func, *counts, n), want[func][case]), (func, case)
    cpos = ppos = 0
    for k, case in enumerate(IDX["dtw"]):
        d, w = dr.dtw_operands(case)
        assert dr.crc(d, w) == int(GOLD["dtw/crc"][k]), case
        st, res, cost = dr.dtw_distance(d, w)
        assert st == int(GOLD["dtw/status"][k]) and dr.crc(cost) == int(GOLD["dtw/ccrc"][k]), case
        value = GOLD["dtw/value"][k]
        if d.size <= 1024:
            stored = GOLD["dtw/cost"][cpos:cpos + d.size + 2]
            assert stored[:1].tobytes() == MARK_BYTES and stored[-1:].tobytes() == MARK_BYTES, case
            assert stored[1:-1].tobytes() == cost.tobytes(), case
            cpos += d.size + 2
        if st:
            assert value.tobytes() == MARK_BYTES * 3 and int(GOLD["dtw/pathlen"][k]) == -1, case
        else:
            assert dr.same_word(res, unguard(value)), case
            path, n = dr.dtw_path(cost), int(GOLD["dtw/pathlen"][k])
            assert n == (0 if path is None else len(path)), case
            assert np.array_equal(GOLD["dtw/path"][ppos:ppos + 2 * n].reshape(-1, 2), path if n else np.zeros((0, 2)))
            ppos += 2 * n
    for (q, t, kind, size), crc in zip(IDX["win"], GOLD["win/crc"]):
        assert dr.crc(dr.init_window(kind, size, q, t)) == int(crc), (q, t, kind, size)


def test_probed_facts_hold_in_the_fixtures():
    """The traps the issue lists, read off the reference's own outputs."""
    u32 = lambda x: int(np.asarray(x, dtype=F).reshape(1).view(np.uint32)[0])                 # noqa: E731
    js = f32_expected("jensenshannon")
    assert u32(js["pair00_67"]) == 0                        # a 0, 0 pair: the chain is NaN, arm_sqrt_f32 gives +0.0
    assert u32(js["rand_64"]) != 0 and not np.isnan(js["rand_64"])
    assert u32(unguard(GOLD["f32/jensenshannon/empty"])) == 0 and u32(unguard(GOLD["f32/euclidean/empty"])) == 0
    assert np.isnan(unguard(GOLD["f32/braycurtis/empty"])) and np.isnan(unguard(GOLD["f32/cosine/empty"]))
    cheb = f32_expected("chebyshev")
    assert np.isnan(cheb["nan0_67"]) and not np.isnan(cheb["nanmid_67"])
    assert cheb["maxfirst_67"] == cheb["maxlast_67"] == cheb["maxrepeat_67"] == F(5.0)
    can = f32_expected("canberra")
    assert not np.isnan(can["zeros00_67"]) and not np.isnan(can["zerospm_67"]) and np.isnan(can["nanelem_67"])
    assert np.isinf(f32_expected("braycurtis")["zeroden_67"])
    assert np.isnan(f32_expected("cosine")["zeropower_67"]) and np.isnan(f32_expected("correlation")["constant_67"])
    a, b, n = dr.bool_operands(f"rand_{dr.BOOL_WRAP}_0")
    assert dr.yule_wraps(a, b, n)
    for func in dr.BOOL_FUNCS:                              # the unused low bits of a partial word do not count
        e = bool_expected(func)
        for case in IDX["bool"]:
            if case.endswith("_1"):
                assert dr.same_word(e[case], e[case[:-1] + "0"]), (func, case)
    assert np.isnan(bool_expected("hamming")["rand_0_0"])   # 0 / 0
    st = dict(zip(IDX["dtw"], GOLD["dtw/status"]))
    assert st["sakoe0_3x5"] == st["slanted0_63x7"] == st["blockend_3x5"] == ARGUMENT_ERROR
    assert st["sakoe0_2x2"] == st["gapcol0_3x5"] == st["none_129x130"] == SUCCESS
    assert np.isinf(GOLD["dtw/cost"][1:]).any()             # F32_MAX + D overflowed somewhere


def test_library_exports_the_symbols(dsp):
    names = [f"arm_{f}_distance_f32{s}" for f in dr.F32_FUNCS for s in ("", "_batch")] + \
        [f"arm_{f}_distance{s}" for f in dr.BOOL_FUNCS for s in ("", "_batch")] + \
        [f"arm_dtw_{f}{s}" for f in ("init_window_q7", "distance_f32", "path_f32") for s in ("", "_batch")]
    assert len(set(names)) == 40 and set(names) == set(_abi.DISTANCE)
    out = subprocess.run(["nm", "-D", "--defined-only", dsp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(names) <= exported
    assert {s for s in exported if s.startswith("arm_") and ("_distance" in s or "_dtw_" in s)} == set(names)
    assert not any("minkowski" in s for s in exported)
    for header, suffix in (("arm_math.h", ""), ("arm_math_mi355x.h", "_batch")):
        text = open(os.path.join(ROOT, "include", header)).read()
        for n in ("arm_dtw_init_window_q7", "arm_dtw_distance_f32", "arm_dtw_path_f32"):
            assert f"{n}{suffix}(" in text, (header, n)
        for n in ("arm_##NAME##_distance_f32", "arm_##NAME##_distance"):
            assert n + suffix + "(" in text, (header, n)
        for f in dr.F32_FUNCS + dr.BOOL_FUNCS:
            assert f"({f})" in text or f"arm_{f}_distance_f32(" in text, (header, f)


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for f in dr.F32_FUNCS:
        assert "cmsis_arm_" + f in getattr(d, f"arm_{f}_distance_f32").__doc__, f
    for f in dr.BOOL_FUNCS:
        assert "cmsis_arm_" + f in getattr(d, f"arm_{f}_distance").__doc__, f
    for n in ("arm_dtw_init_window_q7", "arm_dtw_distance_f32", "arm_dtw_path_f32"):
        assert callable(getattr(d, n)) and callable(getattr(dsp, n)), n
    assert (d.ARM_DTW_SAKOE_CHIBA_WINDOW, d.ARM_DTW_SLANTED_BAND_WINDOW) == (1, 3)
    assert not hasattr(d, "arm_minkowski_distance_f32") and not hasattr(d, "arm_euclidean_distance_f64")
    for n in ("arm_distance_f32", "arm_correlation_distance_f32", "arm_boolean_distance", "distance_batch",
              "boolean_distance_batch", "dtw_init_window_batch", "dtw_distance_batch", "dtw_path_batch"):
        assert callable(getattr(dsp, n)), n


# ------------------------------------------------------------------ GPU helpers
class Dev:
    """A device copy of x whose first element sits `off` elements into an allocation filled with 0x5A bytes (which is
    16-byte aligned), GUARD such bytes after its end."""

    def __init__(self, torch, x, off=0):
        x = np.ascontiguousarray(x)
        self.lo, self.nb, self.shape, self.dtype = off * x.itemsize, x.nbytes, x.shape, x.dtype
        raw = np.full(self.lo + self.nb + GUARD, 0x5A, dtype=np.uint8)
        raw[self.lo:self.lo + self.nb] = x.reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(raw).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == 0x5A).all() and (b[self.lo + self.nb:] == 0x5A).all(), "guard bytes"
        return b[self.lo:self.lo + self.nb].view(self.dtype).reshape(self.shape)


def marker(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, dtype=np.uint8).view(dtype).reshape(shape)


def strided(rows, stride):
    """[rows, n] -> the flat array with the rows `stride` words apart (stride 0: the one row), the gaps marked."""
    rows = np.atleast_2d(rows)
    n = rows.shape[1]
    if stride == 0:
        return rows[0].copy()
    flat = marker(((rows.shape[0] - 1) * stride + n,), rows.dtype)
    for i, r in enumerate(rows):
        flat[i * stride:i * stride + n] = r
    return flat


def batch_call(dsp, torch, name, a, b, b_stride, n, batch, offs=(0, 0, 0)):
    """arm_<name>_batch on device copies -> (status, result [batch] or the untouched marker); checks the guard bytes
    and that the sources are unchanged."""
    da, db = Dev(torch, a, offs[0]), Dev(torch, b, offs[1])
    dres = Dev(torch, marker((batch,), F), offs[2])
    st = getattr(dsp.lib, name)(da.ptr, db.ptr, b_stride, n, dres.ptr, batch, None)
    torch.cuda.synchronize()
    assert da.get().tobytes() == np.ascontiguousarray(a).tobytes(), (name, "source a changed")
    assert db.get().tobytes() == np.ascontiguousarray(b).tobytes(), (name, "source b changed")
    return st, dres.get()


def f32_groups(func):
    """n -> (cases, A [cases, n], B [cases, n], the reference's results)."""
    want, groups = f32_expected(func), {}
    for case in IDX["f32"]:
        a, b = dr.f32_operands(func, case)
        groups.setdefault(a.size, []).append((case, a, b))
    return {n: ([c for c, _, _ in g], np.stack([a for _, a, _ in g]), np.stack([b for _, _, b in g]),
                np.array([want[c] for c, _, _ in g], dtype=F)) for n, g in groups.items()}


# ------------------------------------------------------------------ GPU: f32
@pytest.mark.gpu
@pytest.mark.parametrize("func", dr.F32_FUNCS)
def test_gpu_f32_batch_every_fixture_both_mappings(dsp, torch_gpu, func):
    """Every case as an item of a batch, below kSumLaneMinBatch (one wave per item) and, tiled on the device to just
    above it, one lane per item."""
    needs_host_logf(func)
    torch = torch_gpu
    name = f"arm_{func}_distance_f32_batch"
    for n, (cases, A, B, want) in f32_groups(func).items():
        st, got = batch_call(dsp, torch, name, A, B, n, n, len(cases))
        assert st == SUCCESS
        assert_same_words(got, want, f"{func} n={n} wave form {cases}")
        reps = -(-(SUM_LANE_MIN_BATCH + 3) // len(cases))
        ta = torch.from_numpy(A).cuda().repeat(reps, 1).contiguous()
        tb = torch.from_numpy(B).cuda().repeat(reps, 1).contiguous()
        res = torch.full((ta.shape[0] + 8,), float("nan"), dtype=torch.float32, device="cuda")
        dsp.distance_batch(func, ta, tb, res)
        torch.cuda.synchronize()
        got = res.cpu().numpy()
        assert np.isnan(got[ta.shape[0]:]).all() and got[ta.shape[0]:].view(np.uint32).tolist() == [0x7FC00000] * 8
        assert_same_words(got[:ta.shape[0]], np.tile(want, reps), f"{func} n={n} lane form")
        assert ta[-len(cases):].cpu().numpy().tobytes() == A.tobytes(), "source a changed"
        assert tb[-len(cases):].cpu().numpy().tobytes() == B.tobytes(), "source b changed"


@pytest.mark.gpu
@pytest.mark.parametrize("func", dr.F32_FUNCS)
def test_gpu_f32_dropin_every_fixture(dsp, torch_gpu, func):
    """Host pointers for every case, device pointers for three; blockSize 0; the correlation drop-in's shifted words."""
    needs_host_logf(func)
    torch = torch_gpu
    fn = getattr(dsp.lib, f"arm_{func}_distance_f32")
    want = f32_expected(func)
    for case in IDX["f32"]:
        a, b = dr.f32_operands(func, case)
        x, y = a.copy(), b.copy()
        got = F(fn(x.ctypes.data, y.ctypes.data, a.size))
        assert dsp.last_error()[0] == 0, (func, case, dsp.last_error())
        assert dr.same_word(got, want[case]), (func, case, got, want[case])
        if func == "correlation":
            _, sa, sb = dr.distance_f32(func, a, b)
            assert_same_words(x, sa, f"{case}: pA after the call")
            assert_same_words(y, sb, f"{case}: pB after the call")
        else:
            assert x.tobytes() == a.tobytes() and y.tobytes() == b.tobytes(), (func, case, "a source changed")
        if case in ("rand_5", "rand_257", "mixed_1025"):
            da, db = Dev(torch, a, 1), Dev(torch, b, 3)
            assert dr.same_word(F(fn(da.ptr, db.ptr, a.size)), want[case]), (func, case, "device pointers")
            if func == "correlation":
                assert_same_words(da.get(), sa, "device pA after the call")
            else:
                assert da.get().tobytes() == a.tobytes() and db.get().tobytes() == b.tobytes()
    z = np.zeros(1, dtype=F)
    got = F(fn(z.ctypes.data, z.ctypes.data, 0))
    if func == "chebyshev":
        assert np.isnan(got) and dsp.last_error()[0] != 0
        dsp.lib.arm_mi355x_clear_error()
    else:
        assert dsp.last_error()[0] == 0 and dr.same_word(got, unguard(GOLD[f"f32/{func}/empty"])), (func, got)
    assert np.isnan(F(fn(None, z.ctypes.data, 1))) and dsp.last_error()[0] != 0          # a null pointer
    dsp.lib.arm_mi355x_clear_error()


@pytest.mark.gpu
@pytest.mark.parametrize("func", dr.F32_FUNCS)
def test_gpu_f32_strides_alignment_refusals(dsp, torch_gpu, func):
    needs_host_logf(func)
    torch = torch_gpu
    name = f"arm_{func}_distance_f32_batch"
    for n in (67, 1025):
        for batch in (5, SUM_LANE_MIN_BATCH + 1):
            _, A, B, _ = f32_groups(func)[n]
            rows = np.arange(batch) % A.shape[0]
            a, b = A[rows], B[(rows + 1) % A.shape[0]]
            for stride, offs in ((0, (0, 0, 0)), (n, (1, 0, 0)), (n + 3, (0, 1, 0)), (n, (0, 0, 1)), (0, (1, 1, 1))):
                if batch > 5 and n > 67 and offs != (1, 1, 1):
                    continue
                st, got = batch_call(dsp, torch, name, a, strided(b, stride), stride, n, batch, offs)
                assert st == SUCCESS
                want = [dr.distance_f32(func, a[i], b[0 if stride == 0 else i]) for i in range(min(batch, A.shape[0]))]
                want = np.array([v[0] if func == "correlation" else v for v in want], dtype=F)
                # the rows repeat with period A.shape[0]
                assert_same_words(got, np.resize(want, batch), f"{func} n={n} batch={batch} stride={stride} offs={offs}")
    # refusals: nothing is written
    n, batch = 67, 3
    _, A, B, _ = f32_groups(func)[n]
    a, b = A[:batch], B[:batch]
    lib = dsp.lib
    for args in ("null a", "null b", "null result", "stride"):
        da, db, dres = Dev(torch, a), Dev(torch, b), Dev(torch, marker((batch,), F))
        st = getattr(lib, name)(None if args == "null a" else da.ptr, None if args == "null b" else db.ptr,
                                n - 1 if args == "stride" else n, n, None if args == "null result" else dres.ptr,
                                batch, None)
        torch.cuda.synchronize()
        assert st == ARGUMENT_ERROR, args
        assert dres.get().tobytes() == marker((batch,), F).tobytes(), args
    da, db = Dev(torch, a), Dev(torch, b)
    st = getattr(lib, name)(da.ptr, db.ptr, n, n, da.ptr + 4 * n, batch, None)          # the result inside a
    torch.cuda.synchronize()
    assert st == ARGUMENT_ERROR and da.get().tobytes() == a.tobytes()
    lib.arm_mi355x_clear_error()
    st, got = batch_call(dsp, torch, name, a, b, n, 0, batch)
    if func == "chebyshev":
        assert st == ARGUMENT_ERROR and got.tobytes() == marker((batch,), F).tobytes()
    else:
        assert st == SUCCESS
        assert_same_words(got, np.full(batch, unguard(GOLD[f"f32/{func}/empty"]), dtype=F), "blockSize 0")
    da, db, dres = Dev(torch, a), Dev(torch, b), Dev(torch, marker((batch,), F))
    assert getattr(lib, name)(da.ptr, db.ptr, n, n, dres.ptr, 0, None) == SUCCESS       # batch 0: a no-op
    assert getattr(lib, name)(None, None, n, n, None, 0, None) == SUCCESS
    torch.cuda.synchronize()
    assert dres.get().tobytes() == marker((batch,), F).tobytes()


# ------------------------------------------------------------------ GPU: boolean
def bool_groups():
    groups = {}
    for case in IDX["bool"]:
        a, b, n = dr.bool_operands(case)
        groups.setdefault(n, []).append((case, a, b))
    return groups


@pytest.mark.gpu
def test_gpu_boolean_batch_every_fixture(dsp, torch_gpu):
    """Every case as an item of a batch (all the lanes-per-item steps: 1 word to a whole workgroup), as a few items
    and tiled over several workgroups; both pointers 16-byte aligned (packs where the item size allows) and one word
    off (single words)."""
    torch = torch_gpu
    want = {f: bool_expected(f) for f in dr.BOOL_FUNCS}
    for n, g in bool_groups().items():
        w = dr.bool_words(n)
        A = np.stack([a for _, a, _ in g]).reshape(len(g), w)
        B = np.stack([b for _, _, b in g]).reshape(len(g), w)
        reps = 1 if w > 4096 else -(-600 // len(g))
        for func in dr.BOOL_FUNCS:
            exp = np.array([want[func][c] for c, _, _ in g], dtype=F)
            for offs in ((0, 0, 0), (1, 1, 0)) if n != dr.BOOL_HUGE or func == "yule" else ((0, 0, 0),):
                st, got = batch_call(dsp, torch, f"arm_{func}_distance_batch", np.tile(A, (reps, 1)),
                                     np.tile(B, (reps, 1)), w, n, len(g) * reps, offs)
                assert st == SUCCESS
                assert_same_words(got, np.tile(exp, reps), f"{func} n={n} offs={offs}")


@pytest.mark.gpu
def test_gpu_boolean_dropin_every_fixture(dsp, torch_gpu):
    torch = torch_gpu
    for func in dr.BOOL_FUNCS:
        fn = getattr(dsp.lib, f"arm_{func}_distance")
        want = bool_expected(func)
        for case in IDX["bool"]:
            a, b, n = dr.bool_operands(case)
            if n == dr.BOOL_HUGE and func not in ("yule", "kulsinski"):
                continue                                    # the batched test runs every function on it
            x, y = a.copy(), b.copy()
            got = F(fn(x.ctypes.data if a.size else np.zeros(1, np.uint32).ctypes.data,
                       y.ctypes.data if a.size else np.zeros(1, np.uint32).ctypes.data, n))
            assert dsp.last_error()[0] == 0, (func, case, dsp.last_error())
            assert dr.same_word(got, want[case]), (func, case, got, want[case])
            assert x.tobytes() == a.tobytes() and y.tobytes() == b.tobytes()
        a, b, n = dr.bool_operands("rand_1025_1")
        da, db = Dev(torch, a, 1), Dev(torch, b, 2)
        assert dr.same_word(F(fn(da.ptr, db.ptr, n)), want["rand_1025_1"]), (func, "device pointers")
        assert np.isnan(F(fn(None, b.ctypes.data, n))) and dsp.last_error()[0] != 0
        dsp.lib.arm_mi355x_clear_error()


@pytest.mark.gpu
@pytest.mark.parametrize("func", ("dice", "yule"))
def test_gpu_boolean_strides_alignment_refusals(dsp, torch_gpu, func):
    torch = torch_gpu
    name = f"arm_{func}_distance_batch"
    for n in (33, 129, 4097, 33000):
        w = dr.bool_words(n)
        g = bool_groups()[n]
        batch = 7
        a = np.stack([g[i % len(g)][1] for i in range(batch)])
        b = np.stack([g[(i + 2) % len(g)][2] for i in range(batch)])
        for stride, offs in ((0, (0, 0, 0)), (w, (1, 0, 0)), (w + 3, (0, 1, 0)), (w, (0, 0, 1)), (w + 4, (0, 0, 0))):
            st, got = batch_call(dsp, torch, name, a, strided(b, stride), stride, n, batch, offs)
            assert st == SUCCESS
            want = np.array([dr.boolean_distance(func, a[i], b[0 if stride == 0 else i], n) for i in range(batch)])
            assert_same_words(got, want, f"{func} n={n} stride={stride} offs={offs}")
    n, batch = 129, 3
    w = dr.bool_words(n)
    g = bool_groups()[n]
    a, b = np.stack([g[i][1] for i in range(batch)]), np.stack([g[i][2] for i in range(batch)])
    lib = dsp.lib
    for args in ("null a", "null b", "null result", "stride"):
        da, db, dres = Dev(torch, a), Dev(torch, b), Dev(torch, marker((batch,), F))
        st = getattr(lib, name)(None if args == "null a" else da.ptr, None if args == "null b" else db.ptr,
                                w - 1 if args == "stride" else w, n, None if args == "null result" else dres.ptr,
                                batch, None)
        torch.cuda.synchronize()
        assert st == ARGUMENT_ERROR and dres.get().tobytes() == marker((batch,), F).tobytes(), args
    da, db = Dev(torch, a), Dev(torch, b)
    st = getattr(lib, name)(da.ptr, db.ptr, w, n, db.ptr + 4, batch, None)                # the result inside b
    torch.cuda.synchronize()
    assert st == ARGUMENT_ERROR and db.get().tobytes() == b.tobytes()
    lib.arm_mi355x_clear_error()
    dres = Dev(torch, marker((batch,), F))
    assert getattr(lib, name)(da.ptr, db.ptr, w, n, dres.ptr, 0, None) == SUCCESS         # batch 0: a no-op
    st, got = batch_call(dsp, torch, name, a, b, 0, 0, batch)                             # no booleans: no word read
    assert st == SUCCESS and dres.get().tobytes() == marker((batch,), F).tobytes()
    assert_same_words(got, np.full(batch, bool_expected(func)["rand_0_0"], dtype=F), "numberOfBools 0")


# ------------------------------------------------------------------ GPU: DTW
def dtw_batch(dsp, torch, d, w, batch, w_stride, offs=(0, 0, 0, 0)):
    """arm_dtw_distance_f32_batch and arm_dtw_path_f32_batch on `batch` copies of one case -> (status [batch], result
    [batch], cost [batch, q, t], path length [batch], path [batch, q + t, 2])."""
    q, t = d.shape
    dd = Dev(torch, np.stack([d] * batch), offs[0])
    dw = None if w is None else Dev(torch, strided(np.stack([w.reshape(-1)] * batch), w_stride), offs[1])
    dc, dres = Dev(torch, marker((batch, q, t), F), offs[2]), Dev(torch, marker((batch,), F), offs[3])
    dst = Dev(torch, marker((batch,), np.int32), offs[3])   # offs[3]: the result, status, path and length words
    st = dsp.lib.arm_dtw_distance_f32_batch(dd.ptr, None if w is None else dw.ptr, w_stride, dc.ptr, q, t, dres.ptr,
                                            dst.ptr, batch, None)
    assert st == SUCCESS
    dp, dl = Dev(torch, marker((batch, q + t, 2), np.int16), offs[3]), Dev(torch, marker((batch,), np.uint32), offs[3])
    assert dsp.lib.arm_dtw_path_f32_batch(dc.ptr, q, t, dp.ptr, dl.ptr, batch, None) == SUCCESS
    torch.cuda.synchronize()
    assert dd.get().tobytes() == np.stack([d] * batch).tobytes(), "the distance matrix changed"
    if dw is not None:
        dw.get()
    return dst.get(), dres.get(), dc.get(), dl.get(), dp.get()


def check_dtw(case, out, k):
    status, result, cost, plen, path = out
    d, w = dr.dtw_operands(case)
    wst, wres, wcost = dr.dtw_distance(d, w)
    assert wst == int(GOLD["dtw/status"][k]) and dr.crc(wcost) == int(GOLD["dtw/ccrc"][k])   # the reference's words
    wpath = dr.dtw_path(wcost)                              # the walk does not ask whether the last cell was reached
    if wst == 0 and wpath is not None:
        n0 = int(GOLD["dtw/pathlen"][k])
        p0 = int(2 * GOLD["dtw/pathlen"][:k].clip(0).sum())
        assert np.array_equal(GOLD["dtw/path"][p0:p0 + 2 * n0].reshape(-1, 2), wpath), (case, "the reference's path")
    for i in range(len(status)):
        assert status[i] == wst, (case, i)
        assert_same_words(cost[i], wcost, f"{case} item {i}: cost matrix")
        if wst:
            assert result[i:i + 1].tobytes() == MARK_BYTES, (case, "a result without a path")
        else:
            assert dr.same_word(result[i], wres), (case, result[i], wres)
        if wpath is None:
            assert plen[i] == 0, (case, i, plen[i])
        else:
            assert plen[i] == len(wpath) and np.array_equal(path[i][:plen[i]], wpath), (case, i)
            assert path[i][plen[i]:].tobytes() == marker((len(path[i]) - plen[i], 2), np.int16).tobytes()


@pytest.mark.gpu
def test_gpu_dtw_batch_every_fixture(dsp, torch_gpu):
    """Every case as one item and as a batch of six (two workgroups), the window shared (wStride 0), at the matrix
    size and at the matrix size + 3, every pointer in turn off 16-byte alignment."""
    for k, case in enumerate(IDX["dtw"]):
        d, w = dr.dtw_operands(case)
        check_dtw(case, dtw_batch(dsp, torch_gpu, d, w, 1, 0), k)
        if case.endswith(("3x5", "65x7", "7x65", "129x130")):
            for batch, stride, offs in ((6, 0, (1, 0, 0, 0)), (6, d.size, (0, 1, 0, 0)), (6, d.size + 3, (0, 0, 1, 0)),
                                        (2, d.size, (0, 0, 0, 1))):
                if w is None and stride != 0:
                    continue
                check_dtw(case, dtw_batch(dsp, torch_gpu, d, w, batch, stride, offs), k)


@pytest.mark.gpu
def test_gpu_dtw_dropin_every_fixture(dsp, torch_gpu):
    import cmsisdsp
    for k, case in enumerate(IDX["dtw"]):
        d, w = dr.dtw_operands(case)
        wst, wres, wcost = dr.dtw_distance(d, w)
        d0 = d.copy()
        st, value, cost = cmsisdsp.arm_dtw_distance_f32(d, w)
        assert st == wst and d.tobytes() == d0.tobytes(), case
        assert_same_words(cost, wcost, f"{case}: cost matrix")
        assert np.isnan(value) if wst else dr.same_word(value, wres), (case, value)
        wpath = dr.dtw_path(wcost)
        if wst == 0 and wpath is not None:
            assert np.array_equal(cmsisdsp.arm_dtw_path_f32(cost).reshape(-1, 2), wpath), case
        elif wst == 0:
            n = C.c_uint32(77)
            path = marker((2 * sum(d.shape),), np.int16)
            m = _abi.arm_matrix_instance_f32(d.shape[0], d.shape[1], C.cast(wcost.ctypes.data, _abi.c_f32p))
            dsp.lib.arm_dtw_path_f32(C.byref(m), path.ctypes.data, C.byref(n))
            assert n.value == 0 and dsp.last_error()[0] != 0, case      # the reference would not return
            dsp.lib.arm_mi355x_clear_error()


@pytest.mark.gpu
def test_gpu_dtw_init_window_and_refusals(dsp, torch_gpu):
    torch = torch_gpu
    lib = dsp.lib
    for q, t, kind, size in IDX["win"]:
        want = dr.init_window(kind, size, q, t)
        st, got = dsp.arm_dtw_init_window_q7(kind, size, q, t)
        assert st == SUCCESS and got.tobytes() == want.tobytes(), (q, t, kind, size)
        for batch, off in ((1, 0), (3, 1)):
            dw = Dev(torch, marker((batch, q, t), np.int8), off)
            assert lib.arm_dtw_init_window_q7_batch(kind, size, dw.ptr, q, t, batch, None) == SUCCESS
            torch.cuda.synchronize()
            assert dw.get().tobytes() == np.stack([want] * batch).tobytes(), (q, t, kind, size, batch)
    st, got = dsp.arm_dtw_init_window_q7(2, 1, 3, 5)                                      # an unknown type
    assert st == ARGUMENT_ERROR and not got.any()
    dw = Dev(torch, marker((2, 3, 5), np.int8))
    for args in ((2, 1, dw.ptr, 3, 5, 2), (1, 1, None, 3, 5, 2), (1, 1, dw.ptr, 32769, 1, 1)):
        assert lib.arm_dtw_init_window_q7_batch(*args, None) == ARGUMENT_ERROR, args
    assert lib.arm_dtw_init_window_q7_batch(1, 1, dw.ptr, 3, 5, 0, None) == SUCCESS       # batch 0
    torch.cuda.synchronize()
    assert dw.get().tobytes() == marker((2, 3, 5), np.int8).tobytes()
    # arm_dtw_distance_f32_batch / arm_dtw_path_f32_batch
    d, w = dr.dtw_operands("sakoe1_3x5")
    q, t = d.shape
    dd, dwin = Dev(torch, np.stack([d, d])), Dev(torch, np.stack([w, w]))
    dc, dres, dst = Dev(torch, marker((2, q, t), F)), Dev(torch, marker((2,), F)), Dev(torch, marker((2,), np.int32))
    dp, dl = Dev(torch, marker((2, q + t, 2), np.int16)), Dev(torch, marker((2,), np.uint32))
    bad = [(None, dwin.ptr, 0, dc.ptr, q, t, dres.ptr, dst.ptr, 2), (dd.ptr, dwin.ptr, 0, None, q, t, dres.ptr, dst.ptr, 2),
           (dd.ptr, dwin.ptr, 0, dc.ptr, q, t, None, dst.ptr, 2), (dd.ptr, dwin.ptr, q * t - 1, dc.ptr, q, t, dres.ptr, dst.ptr, 2),
           (dd.ptr, dwin.ptr, 0, dc.ptr, 0, t, dres.ptr, dst.ptr, 2), (dd.ptr, dwin.ptr, 0, dc.ptr, q, 0, dres.ptr, dst.ptr, 2),
           (dd.ptr, None, 0, dc.ptr, 32769, 1, dres.ptr, dst.ptr, 1), (dd.ptr, dwin.ptr, 0, dd.ptr, q, t, dres.ptr, dst.ptr, 2)]
    for args in bad:
        assert lib.arm_dtw_distance_f32_batch(*args, None) == ARGUMENT_ERROR, args
    assert lib.arm_dtw_distance_f32_batch(dd.ptr, dwin.ptr, 0, dc.ptr, q, t, dres.ptr, dst.ptr, 0, None) == SUCCESS
    for args in ((None, q, t, dp.ptr, dl.ptr, 2), (dd.ptr, q, t, None, dl.ptr, 2), (dd.ptr, q, t, dp.ptr, None, 2),
                 (dd.ptr, 0, t, dp.ptr, dl.ptr, 2), (dd.ptr, 1, 32769, dp.ptr, dl.ptr, 1)):
        assert lib.arm_dtw_path_f32_batch(*args, None) == ARGUMENT_ERROR, args
    assert lib.arm_dtw_path_f32_batch(dd.ptr, q, t, dp.ptr, dl.ptr, 0, None) == SUCCESS
    torch.cuda.synchronize()
    lib.arm_mi355x_clear_error()
    for dev, shape, dt in ((dc, (2, q, t), F), (dres, (2,), F), (dst, (2,), np.int32), (dp, (2, q + t, 2), np.int16),
                           (dl, (2,), np.uint32)):
        assert dev.get().tobytes() == marker(shape, dt).tobytes()
    assert dd.get().tobytes() == np.stack([d, d]).tobytes()
    # a null status pointer is allowed
    assert lib.arm_dtw_distance_f32_batch(dd.ptr, dwin.ptr, 0, dc.ptr, q, t, dres.ptr, None, 2, None) == SUCCESS
    torch.cuda.synchronize()
    assert_same_words(dc.get()[1], dr.dtw_distance(d, w)[2], "cost with a null status")
    # the drop-in's shape and length refusals
    m = lambda x, inst, p: inst(x.shape[0], x.shape[1], C.cast(x.ctypes.data, p))          # noqa: E731
    cost, value = marker((q, t), F), marker((1,), F)
    wrong = marker((q, t + 1), F)
    st = lib.arm_dtw_distance_f32(C.byref(m(d, _abi.arm_matrix_instance_f32, _abi.c_f32p)), None,
                                  C.byref(m(wrong, _abi.arm_matrix_instance_f32, _abi.c_f32p)), value.ctypes.data)
    assert st == -3 and value.tobytes() == MARK_BYTES                                     # ARM_MATH_SIZE_MISMATCH
    empty = _abi.arm_matrix_instance_f32(0, t, C.cast(cost.ctypes.data, _abi.c_f32p))
    assert lib.arm_dtw_distance_f32(C.byref(empty), None, C.byref(empty), value.ctypes.data) == ARGUMENT_ERROR
    n = C.c_uint32(77)
    lib.arm_dtw_path_f32(C.byref(empty), marker((8,), np.int16).ctypes.data, C.byref(n))
    assert n.value == 0 and dsp.last_error()[0] != 0
    lib.arm_mi355x_clear_error()
