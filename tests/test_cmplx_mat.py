"""Complex matrix multiply: arm_mat_cmplx_mult_{f32,q31,q15}, their batched and multi-shard forms.

The checker is committed data: tests/golden/cmplx_mat.npz holds the reference's own outputs
(tools/make_golden_cmplx_mat.py), tests/cmplx_mat_ref.py restates the functions in numpy.
CPU: the restatement equals the fixtures bit for bit; which fixtures saturate; the f32 chain the kernel
states (oracle.mat_mult_fmaf on the embedded product) against float64 and the fixture words; exported symbols.
GPU: q15 / q31 are bit-exact everywhere (drop-in against the fixtures with host and device pointers and the
q15 scratch; the batched form against the restatement on both kernels, at the accumulator limit and past it);
f32 is bit-equal to the stated chain and inside 2K 2^-24 (|A||B'|)ij of float64.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cmplx_mat_ref as cr
from cmsisdsp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cmplx_mat.npz"))
INDEX = json.loads(str(GOLD["index"]))
KINDS = list(cr.KINDS)
FIXED = ["q15", "q31"]
SHAPE_IDS = [f"{m}x{k}x{n}" for m, k, n in cr.SHAPES]
SYMBOLS = [f"arm_mat_cmplx_mult_{t}{s}" for t in KINDS for s in ("", "_batch", "_batch_multi")]


def cases_of(kind):
    return [c for k, c in INDEX if k == kind]


def gold(kind, case):
    k = f"{kind}/{case}/"
    return {n[len(k):]: GOLD[n] for n in GOLD.files if n.startswith(k)}


def words_differ(got, want):
    return int((np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)).sum())


# ------------------------------------------------------------------ CPU
def test_fixture_cases_present():
    for kind in KINDS:
        have = set(cases_of(kind))
        if kind == "f32":
            assert have == {f"uniform_{s}" for s in SHAPE_IDS} | {"mixed_17x33x9", "subnormal_17x33x9"}
        else:
            assert have == {f"{f}_{s}" for f in ("full", "scaled") for s in SHAPE_IDS} | \
                {"min_4x8x4", "min_2x1x2", "extreme_4x9x4", "extreme_5x130x3"}
        for case in have:
            g = gold(kind, case)
            assert int(g["status"]) == 0 and g["a"].dtype == g["b"].dtype == g["c"].dtype == cr.KINDS[kind]
            assert g["c"].shape == (g["a"].shape[0], g["b"].shape[1]) and g["a"].shape[1] == 2 * g["b"].shape[0]


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_fixtures(kind):
    for case in cases_of(kind):
        g = gold(kind, case)
        want = cr.mult_f32_ref(g["a"], g["b"]) if kind == "f32" else cr.mult_fixed(kind, g["a"], g["b"])
        assert want.tobytes() == g["c"].tobytes(), case
        if kind == "q15":
            assert cr.scratch_q15(g["b"]).tobytes() == g["scratch"].tobytes(), case


@pytest.mark.parametrize("kind", FIXED)
def test_fixture_saturation(kind):
    """The scaled cases cannot saturate (|v| <= 2^bits / (2 sqrt K)) and do not; the others reach both ends."""
    lo_any = hi_any = False
    for case in cases_of(kind):
        g = gold(kind, case)
        lo, hi = cr.saturated(kind, g["c"])
        if case.startswith("scaled"):
            k = g["b"].shape[0]
            lim = 2.0 ** cr.BITS[kind] / (2.0 * np.sqrt(k))
            assert max(np.abs(g["a"].astype(np.int64)).max(), np.abs(g["b"].astype(np.int64)).max()) <= lim, case
            assert not lo.any() and not hi.any(), case
        else:
            lo_any, hi_any = lo_any or bool(lo.any()), hi_any or bool(hi.any())
    assert lo_any and hi_any
    if kind == "q31":   # the imaginary sum 2^63 wraps to -2^63: the minimum where unwrapped arithmetic gives the maximum
        g = gold(kind, "min_2x1x2")
        assert (g["c"][:, 1::2] == np.iinfo(np.int32).min).all()


def test_embed_is_the_complex_product():
    rng = np.random.default_rng(5)
    a, b = cr.operands("f32", "uniform", 4, 6, 3, rng)
    za = a.astype(np.float64).view(np.complex128)
    zb = b.astype(np.float64).view(np.complex128)
    want = np.ascontiguousarray(za @ zb).view(np.float64)
    assert np.allclose(cr.exact64(a, b), want, rtol=1e-13, atol=1e-15)
    e = cr.embed(b)
    assert e.shape == (12, 6) and e.dtype == np.float32
    assert (e[0::2] == b).all() and (e[1::2, 1::2] == b[:, 0::2]).all() and (e[1::2, 0::2] == -b[:, 1::2]).all()


def test_stated_chain_against_float64_and_fixtures(oracle):
    """The kernel's words, oracle.mat_mult_fmaf(a, embed(b)): within 2K 2^-24 (|A||B'|)ij of float64 (the
    recursive-summation bound of the 2K-term dot product), hence within twice that of the reference's."""
    for case in cases_of("f32"):
        g = gold("f32", case)
        st, chain = oracle.mat_mult_fmaf(g["a"], cr.embed(g["b"]))
        assert st == 0
        bd = cr.bound(g["a"], g["b"])
        assert (np.abs(chain.astype(np.float64) - cr.exact64(g["a"], g["b"])) <= bd).all(), case
        assert (np.abs(chain.astype(np.float64) - g["c"].astype(np.float64)) <= 2 * bd).all(), case


def test_library_exports_cmplx_mat_symbols(dsp):
    assert len(set(SYMBOLS)) == 9 and set(SYMBOLS) == set(_abi.CMPLX_MAT)
    for n in SYMBOLS:
        assert callable(getattr(dsp.lib, n)), n
    for n in ("arm_mat_cmplx_mult", "mat_cmplx_mult_batch", "mat_cmplx_mult_batch_multi"):
        assert callable(getattr(dsp, n)), n


def test_cmsisdsp_module_exposes_cmplx_mat_names():
    import cmsisdsp as d
    for t in KINDS:
        assert callable(getattr(d, f"arm_mat_cmplx_mult_{t}")), t


# ------------------------------------------------------------------ GPU: drop-in against the fixtures
PTR = {"f32": _abi.c_f32p, "q31": _abi.c_i32p, "q15": _abi.c_i16p}
GUARD = 16


def dropin(dsp, torch, kind, a, b, where, scratch="buffer"):
    """arm_mat_cmplx_mult_<kind> on host numpy arrays or device tensors -> (status, C, scratch words or None)."""
    dt = cr.KINDS[kind]
    inst = _abi.CMPLX_MAT_INST[kind]
    if where == "host":
        put, addr, words = (lambda x: x.copy()), (lambda t: t.ctypes.data), (lambda t: t)
    else:
        put, addr, words = (lambda x: torch.from_numpy(x.copy()).cuda()), (lambda t: t.data_ptr()), \
            (lambda t: t.cpu().numpy())
    ta, tb, tc = put(a), put(b), put(np.full((a.shape[0], b.shape[1]), 9, dtype=dt))
    A, B, Cm = (inst(s[0], s[1] // 2, C.cast(addr(t), PTR[kind])) for s, t in ((a.shape, ta), (b.shape, tb),
                                                                                 ((a.shape[0], b.shape[1]), tc)))
    args, ts = [C.byref(A), C.byref(B), C.byref(Cm)], None
    if kind == "q15":
        if scratch == "buffer":
            ts = put(np.full(b.size + GUARD, 0x5a5a, dtype=np.int16))
            args.append(addr(ts))
        else:
            args.append(None)
    st = getattr(dsp.lib, f"arm_mat_cmplx_mult_{kind}")(*args)
    dsp._check_void(f"arm_mat_cmplx_mult_{kind}")
    return st, words(tc), None if ts is None else words(ts)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("kind", FIXED)
def test_dropin_fixed_equals_fixtures(dsp, torch_gpu, kind, where):
    for case in cases_of(kind):
        g = gold(kind, case)
        st, c, scratch = dropin(dsp, torch_gpu, kind, g["a"], g["b"], where)
        assert st == 0 and c.tobytes() == g["c"].tobytes(), (case, words_differ(c, g["c"]))
        if kind == "q15":
            n = g["b"].size
            assert scratch[:n].tobytes() == g["scratch"].tobytes(), case
            assert (scratch[n:] == 0x5a5a).all(), case            # nothing beyond 2 K N words


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_dropin_q15_null_scratch(dsp, torch_gpu, where):
    for case in ("full_17x33x9", "extreme_4x9x4"):
        g = gold("q15", case)
        st, c, _ = dropin(dsp, torch_gpu, "q15", g["a"], g["b"], where, scratch=None)
        assert st == 0 and c.tobytes() == g["c"].tobytes(), case


@pytest.mark.gpu
def test_dropin_q15_mixed_pointers(dsp, torch_gpu):
    """Host operands with a device scratch, and device operands with a host scratch."""
    torch = torch_gpu
    g = gold("q15", "full_7x33x5")
    inst = _abi.CMPLX_MAT_INST["q15"]
    for dev_ops in (False, True):
        a, b, c = g["a"].copy(), g["b"].copy(), np.zeros_like(g["c"])
        keep = [torch.from_numpy(x).cuda() for x in (a, b, c)] if dev_ops else None
        ptrs = [t.data_ptr() for t in keep] if dev_ops else [x.ctypes.data for x in (a, b, c)]
        A, B, Cm = (inst(x.shape[0], x.shape[1] // 2, C.cast(p, _abi.c_i16p)) for x, p in zip((a, b, c), ptrs))
        hs = np.zeros(b.size, dtype=np.int16)
        ds = torch.zeros(b.size, dtype=torch.int16, device="cuda")
        st = dsp.lib.arm_mat_cmplx_mult_q15(C.byref(A), C.byref(B), C.byref(Cm), hs.ctypes.data if dev_ops else ds.data_ptr())
        dsp._check_void("arm_mat_cmplx_mult_q15")
        got = keep[2].cpu().numpy() if dev_ops else c
        assert st == 0 and got.tobytes() == g["c"].tobytes()
        assert (hs if dev_ops else ds.cpu().numpy()).tobytes() == g["scratch"].tobytes()


# ------------------------------------------------------------------ GPU: batched fixed point against the restatement
# (complex M, K, N, batch, fills).  BN differs per type, so the whole-tile shapes do.
FILLS3 = ("full", "scaled", "extreme")
FIXED_BATCH = {
    "q15": [(130, 33, 65, 2, FILLS3),            # ragged, past one tile and one K step
            (128, 32, 64, 1, FILLS3),            # one whole tile: the unguarded kernel
            (256, 64, 128, 3, FILLS3),           # whole tiles, two K steps
            (2, 16352, 3, 1, ("min",) + FILLS3),  # real depth 32704: the int32 class accumulators' limit
            (2, 16353, 2, 1, FILLS3)],           # past it: the VALU kernel
    "q31": [(130, 33, 65, 2, FILLS3),
            (128, 32, 32, 1, FILLS3),
            (256, 64, 64, 3, FILLS3),
            (2, 16352, 3, 1, ("min",) + FILLS3),
            (2, 16353, 2, 1, FILLS3)],
}
FIXED_BATCH_CASES = [(t, *c[:4], f) for t in FIXED for c in FIXED_BATCH[t] for f in c[4]]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,m,k,n,batch,fill", FIXED_BATCH_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}x{c[4]}-{c[5]}" for c in FIXED_BATCH_CASES])
def test_fixed_batch_equals_restatement(dsp, torch_gpu, kind, m, k, n, batch, fill):
    torch = torch_gpu
    rng = np.random.default_rng([m, k, n, batch, len(fill), cr.BITS[kind]])
    a, b = cr.operands(kind, fill, m, k, n, rng, batch)
    want = cr.mult_fixed(kind, a, b)
    dc = torch.full((batch, m, 2 * n), 9, dtype=torch.from_numpy(a).dtype, device="cuda")
    dsp.mat_cmplx_mult_batch(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), dc)
    got = dc.cpu().numpy()
    assert got.tobytes() == want.tobytes(), f"{words_differ(got, want)} bytes differ"
    if fill == "scaled":
        lo, hi = cr.saturated(kind, want)
        assert not lo.any() and not hi.any()


def offset_tensor(torch, x, off):
    """A device copy of x whose first word sits `off` elements past an allocation's (aligned) start."""
    buf = torch.zeros(x.size + off, dtype=torch.from_numpy(x).dtype, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["a", "b", "c", "all"])
def test_batch_pdata_offset_by_one_element(dsp, torch_gpu, oracle, kind, which):
    """Whole-tile shapes whose pData is one element past an aligned address fall back to the guarded kernel."""
    torch = torch_gpu
    m, k, n = {"q15": (128, 32, 64), "q31": (128, 32, 32), "f32": (128, 8, 64)}[kind]
    rng = np.random.default_rng([3, cr.KINDS[kind]().itemsize, len(which)])
    a, b = cr.operands(kind, "uniform" if kind == "f32" else "full", m, k, n, rng, 2)
    off = {x: int(which in (x, "all")) for x in "abc"}
    da, db = offset_tensor(torch, a, off["a"]), offset_tensor(torch, b, off["b"])
    dc = offset_tensor(torch, np.zeros((2, m, 2 * n), dtype=a.dtype), off["c"])
    dsp.mat_cmplx_mult_batch(da, db, dc)
    got = dc.cpu().numpy()
    if kind == "f32":
        want = np.stack([oracle.mat_mult_fmaf(a[i], cr.embed(b[i]))[1] for i in range(2)])
    else:
        want = cr.mult_fixed(kind, a, b)
    assert got.tobytes() == want.tobytes(), f"{words_differ(got, want)} bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batch_multi_on_one_device(dsp, torch_gpu, oracle, kind):
    torch = torch_gpu
    m, k, n = 33, 17, 9
    rng = np.random.default_rng([7, cr.KINDS[kind]().itemsize])
    shards, wants = [], []
    for batch in (2, 3):
        a, b = cr.operands(kind, "uniform" if kind == "f32" else "full", m, k, n, rng, batch)
        dc = torch.zeros((batch, m, 2 * n), dtype=torch.from_numpy(a).dtype, device="cuda:0")
        shards.append((torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0"), dc))
        wants.append(np.stack([oracle.mat_mult_fmaf(a[i], cr.embed(b[i]))[1] for i in range(batch)])
                     if kind == "f32" else cr.mult_fixed(kind, a, b))
    dsp.mat_cmplx_mult_batch_multi(shards)
    for (_, _, dc), want in zip(shards, wants):
        assert dc.cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------ GPU: f32
def tf32(x):
    """Round f32 to a 10-bit mantissa (TF32 / xf32 operands), nearest-even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0xFFF + ((u >> 13) & 1)) & ~np.uint64(0x1FFF)
    return u.astype(np.uint32).view(np.float32)


# complex (M, K, N, batch): (128, 8, 64) and (256, 24, 128) are whole tiles (the unguarded kernel)
F32_SHAPES = [(1, 1, 1, 1), (5, 7, 3, 1), (17, 33, 9, 1), (130, 9, 65, 1), (128, 8, 64, 1), (256, 24, 128, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["uniform", "mixed", "subnormal"])
@pytest.mark.parametrize("m,k,n,batch", F32_SHAPES, ids=[f"{m}x{k}x{n}x{b}" for m, k, n, b in F32_SHAPES])
def test_f32_batch_is_the_stated_chain(dsp, torch_gpu, oracle, m, k, n, batch, fill):
    """Bit-equal to the k-ascending fmaf chain from +0 over the embedded product, re = fma(-b, d, fma(a, c, re)),
    im = fma(b, c, fma(a, d, im)); every item within 2K 2^-24 (|A||B'|)ij of float64, plus 2^-150 per term for the
    subnormal fill, where a rounded product is off by up to half the smallest subnormal whatever the arithmetic
    (cmplx_mat_ref.bound: at K = 1 the relative term alone is near 2^-155).  Negative control: the
    same chain on TF32-rounded operands differs in more than half the words when 2K >= 16."""
    torch = torch_gpu
    rng = np.random.default_rng([m, k, n, batch, len(fill)])
    a, b = cr.operands("f32", fill, m, k, n, rng, batch)
    dc = torch.full((batch, m, 2 * n), 9.0, dtype=torch.float32, device="cuda")
    dsp.mat_cmplx_mult_batch(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), dc)
    got = dc.cpu().numpy()
    for i in range(batch):
        st, want = oracle.mat_mult_fmaf(a[i], cr.embed(b[i]))
        assert st == 0
        assert got[i].tobytes() == want.tobytes(), f"item {i}: {np.sum(got[i].view(np.uint32) != want.view(np.uint32))} words differ"
        assert (np.abs(got[i].astype(np.float64) - cr.exact64(a[i], b[i])) <= cr.bound(a[i], b[i])).all(), i
    if 2 * k >= 16 and fill != "subnormal":
        _, tf = oracle.mat_mult_fmaf(tf32(a[0]), cr.embed(tf32(b[0])))
        assert np.mean(tf.view(np.uint32) != got[0].view(np.uint32)) > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_f32_dropin_against_chain_and_fixtures(dsp, torch_gpu, oracle, where):
    for case in cases_of("f32"):
        g = gold("f32", case)
        st, c, _ = dropin(dsp, torch_gpu, "f32", g["a"], g["b"], where)
        assert st == 0 and c.tobytes() == oracle.mat_mult_fmaf(g["a"], cr.embed(g["b"]))[1].tobytes(), case
        bd = cr.bound(g["a"], g["b"])
        assert (np.abs(c.astype(np.float64) - cr.exact64(g["a"], g["b"])) <= bd).all(), case
        assert (np.abs(c.astype(np.float64) - g["c"].astype(np.float64)) <= 2 * bd).all(), case


# ------------------------------------------------------------------ GPU: status, cmsisdsp
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shapes", [((3, 5), (4, 2), (3, 2)), ((3, 5), (5, 2), (4, 2)), ((3, 5), (5, 2), (3, 3))],
                         ids=["inner", "dst_rows", "dst_cols"])
def test_size_mismatch(dsp, torch_gpu, kind, shapes):
    """numColsA != numRowsB, or pDst not numRowsA x numColsB (complex counts): ARM_MATH_SIZE_MISMATCH, pDst untouched."""
    dt, inst = cr.KINDS[kind], _abi.CMPLX_MAT_INST[kind]
    arrs = [np.full((r, 2 * c), 7, dtype=dt) for r, c in shapes]
    A, B, Cm = (inst(r, c, C.cast(x.ctypes.data, PTR[kind])) for (r, c), x in zip(shapes, arrs))
    extra = [None] if kind == "q15" else []
    assert getattr(dsp.lib, f"arm_mat_cmplx_mult_{kind}")(C.byref(A), C.byref(B), C.byref(Cm), *extra) == dsp.ARM_MATH_SIZE_MISMATCH
    assert getattr(dsp.lib, f"arm_mat_cmplx_mult_{kind}_batch")(C.byref(A), C.byref(B), C.byref(Cm), 1, None) == \
        dsp.ARM_MATH_SIZE_MISMATCH
    assert (arrs[2] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_zero_depth_gives_zeros(dsp, torch_gpu, kind):
    torch = torch_gpu
    tdt = {"f32": torch.float32, "q31": torch.int32, "q15": torch.int16}[kind]
    da, db = torch.zeros((2, 3, 0), dtype=tdt, device="cuda"), torch.zeros((2, 0, 4), dtype=tdt, device="cuda")
    dc = torch.full((2, 3, 4), 9, dtype=tdt, device="cuda")
    dsp.mat_cmplx_mult_batch(da, db, dc)
    assert not dc.cpu().numpy().any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_cmsisdsp_module_cmplx_mat(torch_gpu, oracle, kind):
    import cmsisdsp as d
    g = gold(kind, "uniform_7x33x5" if kind == "f32" else "full_7x33x5")
    extra = [np.zeros(g["b"].size, dtype=np.int16)] if kind == "q15" else []
    st, c = getattr(d, f"arm_mat_cmplx_mult_{kind}")(g["a"], g["b"], *extra)
    want = oracle.mat_mult_fmaf(g["a"], cr.embed(g["b"]))[1] if kind == "f32" else g["c"]
    assert st == 0 and c.shape == g["c"].shape and c.tobytes() == want.tobytes()
