"""Biquad cascades: arm_biquad_cascade_df1_{f32,q31,fast_q31,q15,fast_q15}, arm_biquad_cas_df1_32x64_q31,
arm_biquad_cascade_df2T_f32, arm_biquad_cascade_stereo_df2T_f32 (+ inits and the batched device API).

The checker is committed data: tests/golden/biquad.npz holds the reference's own outputs
(tools/make_golden_biquad.py), tests/biquad_ref.py restates the functions in numpy.
CPU: the restatement equals the fixtures bit for bit; struct layouts, exported symbols, module names.
GPU: the drop-in equals the fixtures (host and device buffers, in place); the batched API equals the
restatement over stage counts, block sizes and stream counts on both sides of every path of the kernel
(streams per wave, the 64-stage pass limit, tile and group boundaries, blocks shorter than the pipeline).
Every comparison is bit-exact.
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import biquad_ref
from cmsisdsp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = list(biquad_ref.FUNCS)
INITS = sorted({v[1] for v in _abi.BIQUAD_FUNCS.values()})
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "biquad.npz"))
INDEX = json.loads(str(GOLD["index"]))


def cases_of(func):
    return [(c, n) for f, c, n in INDEX if f == func]


def gold(func, case, nblocks):
    k = f"{func}/{case}"
    return (GOLD[k + "/coeffs"], int(GOLD[k + "/ps"]), [GOLD[f"{k}/x{i}"] for i in range(nblocks)],
            [GOLD[f"{k}/y{i}"] for i in range(nblocks)], GOLD[k + "/state"])


def stages_of(func, coeffs):
    return len(coeffs) // biquad_ref.FUNCS[func][3]


# ------------------------------------------------------------------ CPU
def test_fixture_cases_present():
    names = {"s1_b1_1", "s2_b7_9", "s3_b37_37", "s8_b130_130", "s17_b64_5", "s70_b96_33"}
    for func, (dt, *_) in biquad_ref.FUNCS.items():
        have = {c for c, _ in cases_of(func)}
        assert names <= have and ("decay" if dt == np.float32 else "extreme") in have, func
        if dt != np.float32:
            assert {gold(func, c, 1)[1] for c in names} == {0, 1, 2, 3}, func


@pytest.mark.parametrize("func", FUNCS)
def test_restatement_equals_fixtures(func):
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    for case, nb in cases_of(func):
        c, ps, xs, ys, state = gold(func, case, nb)
        st = np.zeros((1, ks * stages_of(func, c)), dtype=sdt)
        for x, y in zip(xs, ys):
            got, st = biquad_ref.run(func, c, ps, x[None], st)
            assert got[0].tobytes() == y.tobytes(), case
        assert st[0].tobytes() == state.tobytes(), case


def test_decay_fixture_passes_through_subnormals():
    tiny = np.finfo(np.float32).tiny
    for func in FUNCS:
        if biquad_ref.FUNCS[func][0] == np.float32:
            y = gold(func, "decay", 2)[3][0]
            assert ((np.abs(y) > 0) & (np.abs(y) < tiny)).any() and not y[-8:].any(), func


def test_struct_layout_matches_reference(tmp_path):
    """tools/abi_layout_biquad.c compiled against include/ prints what it printed when compiled
    against the reference headers (tests/golden/abi_layout_biquad.json); the ctypes mirrors agree."""
    exe = str(tmp_path / "abi_layout_biquad")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "abi_layout_biquad.c"),
                    "-o", exe], check=True)
    ours = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_layout_biquad.json")))
    assert ours == ref and len(ref) == 6
    for name, lay in ref.items():
        st = getattr(_abi, name)
        assert C.sizeof(st) == lay["size"], name
        assert {f for f, _ in st._fields_} == set(lay) - {"size"}, name
        for fname, _ in st._fields_:
            assert getattr(st, fname).offset == lay[fname], (name, fname)


def test_library_exports_biquad_symbols(dsp):
    names = FUNCS + INITS + [f + "_batch" for f in FUNCS]
    assert len(FUNCS) == 8 and len(INITS) == 6 and len(names) == 22
    for n in names:
        assert callable(getattr(dsp.lib, n)), n


def test_cmsisdsp_module_exposes_biquad_names():
    import cmsisdsp as d
    for n in FUNCS + INITS:
        assert callable(getattr(d, n)), n
    for inst in {v[0].__name__ for v in _abi.BIQUAD_FUNCS.values()}:
        assert callable(getattr(d, inst)), inst


# ------------------------------------------------------------------ GPU: drop-in against the fixtures
def make_inst(func, stages, pcoeffs, pstate, ps):
    inst = _abi.BIQUAD_FUNCS[func][0]
    kw = {"postShift": ps} if any(f == "postShift" for f, _ in inst._fields_) else {}
    return inst(numStages=stages, pState=pstate, pCoeffs=pcoeffs, **kw)


def dropin(dsp, func, c, ps, xs, state_ptr=None, read_state=None, in_place=False, dev=None):
    """init + one call per block through the C ABI.  state_ptr: device state (read back with
    read_state()); dev: a function moving a numpy block to a device tensor (device src / dst)."""
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    inst, init, ps_t = _abi.BIQUAD_FUNCS[func]
    stages = stages_of(func, c)
    S = inst()
    state = np.full(ks * stages, 77, dtype=sdt)          # the init zeroes it
    sp = state.ctypes.data if state_ptr is None else state_ptr
    getattr(dsp.lib, init)(C.byref(S), stages, c.ctypes.data, sp, *([ps] if ps_t else []))
    assert dsp.last_error()[0] == 0, dsp.last_error()
    outs = []
    for x in xs:
        if dev is not None:
            src = dev(x)
            dst = src if in_place else dev(np.zeros_like(x))
            getattr(dsp.lib, func)(C.byref(S), src.data_ptr(), dst.data_ptr(), len(x) // ch)
            y = dst.cpu().numpy()
        else:
            src = x.copy()
            y = src if in_place else np.zeros_like(x)
            getattr(dsp.lib, func)(C.byref(S), src.ctypes.data, y.ctypes.data, len(x) // ch)
        assert dsp.last_error()[0] == 0, dsp.last_error()
        outs.append(y)
    return outs, (state if read_state is None else read_state())


def same(got, ys, state):
    outs, st = got
    for k, (u, v) in enumerate(zip(outs, ys)):
        assert u.tobytes() == v.tobytes(), k
    assert st.tobytes() == state.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_dropin_equals_fixtures(dsp, torch_gpu, func):
    """Host buffers, every fixture case (the extreme-word and subnormal-decay cases among them)."""
    for case, nb in cases_of(func):
        c, ps, xs, ys, state = gold(func, case, nb)
        same(dropin(dsp, func, c, ps, xs), ys, state)


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_dropin_device_state(dsp, torch_gpu, func):
    torch = torch_gpu
    c, ps, xs, ys, state = gold(func, "s8_b130_130", 2)
    t = torch.from_numpy(np.full(len(state), 5, dtype=state.dtype)).cuda()
    same(dropin(dsp, func, c, ps, xs, state_ptr=t.data_ptr(), read_state=lambda: t.cpu().numpy()), ys, state)


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_dropin_in_place(dsp, torch_gpu, func):
    """pSrc == pDst, host buffers and device buffers."""
    torch = torch_gpu
    c, ps, xs, ys, state = gold(func, "s3_b37_37", 2)
    same(dropin(dsp, func, c, ps, xs, in_place=True), ys, state)
    c, ps, xs, ys, state = gold(func, "s70_b96_33", 2)
    same(dropin(dsp, func, c, ps, xs, in_place=True, dev=lambda a: torch.from_numpy(a.copy()).cuda()), ys, state)


# ------------------------------------------------------------------ GPU: batched API against the restatement
def coeffs_for(func, stages, ps, seed):
    return biquad_ref.stable_coeffs(func, stages, ps, seed)


def inputs_for(func, batch, block, seed):
    dt, _, _, _, ch = biquad_ref.FUNCS[func]
    rng = np.random.default_rng(seed)
    if dt == np.float32:
        return rng.uniform(-1, 1, (batch, block * ch)).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min // 2, info.max // 2, (batch, block * ch), endpoint=True).astype(dt)


@functools.lru_cache(maxsize=None)
def expected(func, stages, blocks, batch, ps):
    """(coeffs, [x per call], [y per call], [state after each call]) from the restatement, computed once."""
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    c = coeffs_for(func, stages, ps, 1000 + stages)
    st = np.zeros((batch, ks * stages), dtype=sdt)
    xs, ys, sts = [], [], []
    for k, b in enumerate(blocks):
        x = inputs_for(func, batch, b, 7 * stages + b + k)
        y, st = biquad_ref.run(func, c, ps, x, st)
        xs.append(x), ys.append(y), sts.append(st)
    for a in [c] + xs + ys + sts:
        a.setflags(write=False)
    return c, xs, ys, sts


def tdtype(torch, dt):
    return {np.float32: torch.float32, np.int32: torch.int32, np.int16: torch.int16, np.int64: torch.int64}[dt]


def batch_call(dsp, torch, func, S, src, dst, block, batch, state):
    f = getattr(dsp.lib, func + "_batch")
    ptr = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())   # noqa: E731
    return f(C.byref(S), ptr(src), ptr(dst), block, batch, ptr(state),
             C.c_void_p(torch.cuda.current_stream().cuda_stream))


# (numStages, blocks of the two calls, batch): 3 and 17 do not divide 64; 64 | 65 cross the one-pass limit;
# 127 is the q15 maximum; the blocks put -1 / 0 / +1 around the tile (16), the I/O group (32) and larger
# powers of two, and include blocks shorter than the stage count (the pipeline never fills); batch 65 is
# more streams than a wave holds at any stage count.
BATCH_CASES = [(1, (1000, 1), 65), (2, (257, 2), 5), (3, (255, 3), 65), (8, (65, 15), 1), (17, (64, 16), 65),
               (64, (63, 17), 5), (65, (16, 64), 5), (127, (255, 2), 1), (1, (33, 31), 5),
               # from 6 (f32) / 16 (fixed point) stages per pass and 1024 * 2 * (64 / stages) streams a lane
               # runs two streams with half tiles of 8: both sides of each threshold
               (32, (17, 40), 4097), (32, (5, 3), 4096), (32, (33, 2), 4095), (65, (20, 5), 2049),
               (5, (9, 20), 24577), (6, (9, 20), 20481), (15, (9, 20), 8193), (16, (9, 20), 8193)]
BIG = (255, (17, 65), 5)         # uint8 stage counts: four passes
BATCH_PARAMS = [(f, *c) for f in FUNCS for c in BATCH_CASES] + \
    [(f, *BIG) for f in ("arm_biquad_cascade_df2T_f32", "arm_biquad_cas_df1_32x64_q31",
                         "arm_biquad_cascade_stereo_df2T_f32")]


@pytest.mark.gpu
@pytest.mark.parametrize("func,stages,blocks,batch", BATCH_PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_batch_equals_restatement(dsp, torch_gpu, func, stages, blocks, batch):
    """Two consecutive calls, the state carried on the device; coefficients through the host cache."""
    torch = torch_gpu
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    ps = stages % 4 if func in biquad_ref.HAS_SHIFT else 0
    c, xs, ys, sts = expected(func, stages, blocks, batch, ps)
    S = make_inst(func, stages, c.ctypes.data, None, ps)
    state = torch.zeros((batch, ks * stages), dtype=tdtype(torch, sdt), device="cuda")
    for x, y, st, b in zip(xs, ys, sts, blocks):
        src = torch.from_numpy(x.copy()).cuda()
        dst = torch.zeros_like(src)
        assert batch_call(dsp, torch, func, S, src, dst, b, batch, state) == 0, dsp.last_error()
        assert dst.cpu().numpy().tobytes() == y.tobytes(), b
        assert src.cpu().numpy().tobytes() == x.tobytes(), b
        assert state.cpu().numpy().tobytes() == st.tobytes(), b


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("stages,blocks,batch", [(17, (64, 16), 65), (32, (17, 40), 4097)], ids=["one", "two"])
def test_batch_in_place(dsp, torch_gpu, func, stages, blocks, batch):
    """d_src == d_dst (one and two streams per lane); coefficients in device memory."""
    torch = torch_gpu
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    ps = stages % 4 if func in biquad_ref.HAS_SHIFT else 0
    c, xs, ys, sts = expected(func, stages, blocks, batch, ps)
    dc = torch.from_numpy(c.copy()).cuda()
    S = make_inst(func, stages, dc.data_ptr(), None, ps)
    state = torch.zeros((batch, ks * stages), dtype=tdtype(torch, sdt), device="cuda")
    for x, y, st, b in zip(xs, ys, sts, blocks):
        buf = torch.from_numpy(x.copy()).cuda()
        assert batch_call(dsp, torch, func, S, buf, buf, b, batch, state) == 0, dsp.last_error()
        assert buf.cpu().numpy().tobytes() == y.tobytes(), b
        assert state.cpu().numpy().tobytes() == st.tobytes(), b


@pytest.mark.gpu
@pytest.mark.parametrize("func", ["arm_biquad_cascade_df1_q15", "arm_biquad_cascade_df1_fast_q15",
                                  "arm_biquad_cascade_df1_f32", "arm_biquad_cascade_stereo_df2T_f32"])
@pytest.mark.parametrize("offs", [(1, 3, 2), (3, 2, 1), (2, 1, 3)])
def test_batch_pointer_offsets(dsp, torch_gpu, func, offs):
    """d_src, d_dst and d_state are views at element offsets 1 .. 3 into guard-padded tensors; the
    guard words are unchanged afterwards."""
    torch = torch_gpu
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    stages, blocks, batch = 3, (255, 3), 65
    ps = stages % 4 if func in biquad_ref.HAS_SHIFT else 0
    c, xs, ys, sts = expected(func, stages, blocks, batch, ps)
    S = make_inst(func, stages, c.ctypes.data, None, ps)
    pad, guard = 8, 21
    o_src, o_dst, o_st = offs

    def padded(a, off):
        flat = np.full(a.size + 2 * pad, guard, dtype=a.dtype)
        flat[off:off + a.size] = a.reshape(-1)
        return torch.from_numpy(flat).cuda()

    def check(t, off, want, what):
        h = t.cpu().numpy()
        assert h[off:off + want.size].tobytes() == want.tobytes(), what
        assert (h[:off] == guard).all() and (h[off + want.size:] == guard).all(), what + " guard"

    st0 = np.zeros((batch, ks * stages), dtype=sdt)
    state = padded(st0, o_st)
    esz = state.element_size()
    for x, y, st, b in zip(xs, ys, sts, blocks):
        src, dst = padded(x, o_src), padded(np.full_like(x, guard), o_dst)
        rc = batch_call(dsp, torch, func, S, src.data_ptr() + o_src * src.element_size(),
                        dst.data_ptr() + o_dst * dst.element_size(), b, batch, state.data_ptr() + o_st * esz)
        assert rc == 0, dsp.last_error()
        check(dst, o_dst, y, "dst")
        check(src, o_src, x, "src")
        check(state, o_st, st, "state")


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_batch_argument_errors(dsp, torch_gpu, func):
    torch = torch_gpu
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    stages, batch, block = 2, 3, 16
    c = coeffs_for(func, stages, 1, 5)
    src = torch.from_numpy(inputs_for(func, batch, block, 1)).cuda()
    dst = torch.full_like(src, 9)
    state = torch.full((batch, ks * stages), 4, dtype=tdtype(torch, sdt), device="cuda")
    S = make_inst(func, stages, c.ctypes.data, None, 1)
    err = _abi.ARM_MATH_ARGUMENT_ERROR
    assert batch_call(dsp, torch, func, make_inst(func, 0, c.ctypes.data, None, 1), src, dst, block, batch, state) == err
    assert batch_call(dsp, torch, func, make_inst(func, stages, None, None, 1), src, dst, block, batch, state) == err
    assert batch_call(dsp, torch, func, S, 0, dst, block, batch, state) == err
    assert batch_call(dsp, torch, func, S, src, 0, block, batch, state) == err
    assert batch_call(dsp, torch, func, S, src, dst, block, batch, 0) == err
    f = getattr(dsp.lib, func + "_batch")
    assert f(None, src.data_ptr(), dst.data_ptr(), block, batch, state.data_ptr(), None) == err
    assert batch_call(dsp, torch, func, S, src, dst, 0, batch, state) == 0
    assert batch_call(dsp, torch, func, S, src, dst, block, 0, state) == 0
    torch.cuda.synchronize()
    assert (dst == 9).all().item() and (state == 4).all().item()
    dsp.lib.arm_mi355x_clear_error()


@pytest.mark.gpu
@pytest.mark.parametrize("func", ["arm_biquad_cascade_df1_f32", "arm_biquad_cascade_df1_q15"])
def test_cmsisdsp_module_biquad(torch_gpu, func):
    """cmsisdsp_filtering.c call shapes: init (S, numStages, pCoeffs, pState[, postShift]), then
    (S, pSrc) -> pDst; init plus two calls equal the fixtures."""
    import cmsisdsp as d
    inst, init, ps_t = _abi.BIQUAD_FUNCS[func]
    for case in ("s3_b37_37", "s8_b130_130"):
        c, ps, xs, ys, state = gold(func, case, 2)
        stages = stages_of(func, c)
        S = getattr(d, inst.__name__)()
        getattr(d, init)(S, stages, c, np.zeros(4 * stages), *([ps] if ps_t else []))
        for x, y in zip(xs, ys):
            got = getattr(d, func)(S, x)
            assert got.dtype == y.dtype and got.tobytes() == y.tobytes(), case
