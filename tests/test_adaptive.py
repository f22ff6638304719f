"""IIR lattice and LMS / normalised LMS: arm_iir_lattice_{f32,q31,q15}, arm_lms_{f32,q31,q15},
arm_lms_norm_{f32,q15} (+ inits, the batched device API and armRecipTableQ15).

The checker is committed data: tests/golden/adaptive.npz holds the reference's own outputs
(tools/make_golden_adaptive.py), tests/adaptive_ref.py restates the functions in numpy.
CPU: the restatement equals the fixtures bit for bit; struct layouts, exported symbols, the reciprocal
table, module names.
GPU: the drop-in equals the fixtures (host and device buffers, the aliased forms, what the inits zero);
the batched API equals the restatement, per-stream coefficients, states and energies, over stream counts
and sizes on both sides of every path of the kernels.  Every comparison is bit-exact.
"""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
from cmsisdsp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = list(ar.FUNCS)
IIR = [f for f in FUNCS if ar.FUNCS[f][1] == "iir"]
LMS = [f for f in FUNCS if ar.FUNCS[f][1] != "iir"]
INITS = [v[1] for v in _abi.ADAPTIVE_FUNCS.values()]
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "adaptive.npz"))
INDEX = json.loads(str(GOLD["index"]))
MAIN = {"n1_b1_1", "n2_b7_9", "n3_b37_37", "n8_b130_130", "n17_b64_5", "n70_b96_33"}
TINY = np.finfo(np.float32).tiny


def cases_of(func):
    return [c for f, c in INDEX if f == func]


def gold(func, case):
    k = f"{func}/{case}/"
    return {n[len(k):]: GOLD[n] for n in GOLD.files if n.startswith(k)}


def subnormal(a):
    return bool(((np.abs(a) > 0) & (np.abs(a) < TINY)).any())


def mu_of(func, g):
    return float(g["mu"]) if ar.FUNCS[func][0] == np.float32 else int(g["mu"])


# ------------------------------------------------------------------ CPU
def test_fixture_cases_present():
    assert list(ar.FUNCS) == list(_abi.ADAPTIVE_FUNCS) and len(FUNCS) == 8
    for func, (dt, fam) in ar.FUNCS.items():
        have = set(cases_of(func))
        assert MAIN <= have, func
        assert ("decay" if dt == np.float32 else "extreme") in have, func
        assert (fam == "iir") != ("converge" in have), func
        if fam != "iir" and dt != np.float32:
            assert {int(gold(func, c)["ps"]) for c in MAIN} == {0, 1, 2, 3}, func


@pytest.mark.parametrize("func", FUNCS)
def test_restatement_equals_fixtures(func):
    dt, fam = ar.FUNCS[func]
    for case in cases_of(func):
        g = gold(func, case)
        if fam == "iir":
            st = np.zeros((1, len(g["k"])), dtype=dt)
            for i in range(2):
                y, st = ar.iir_lattice(func, g["k"], g["v"], g[f"x{i}"][None], st)
                assert y[0].tobytes() == g[f"y{i}"].tobytes(), (case, i)
            assert st[0].tobytes() == g["state"].tobytes(), case
            continue
        c, st = g["coeffs0"][None].copy(), np.zeros((1, len(g["coeffs0"]) - 1), dtype=dt)
        ex = np.zeros((1, 2), dtype=dt) if fam == "nlms" else None
        for i in range(2):
            y, e, c, st, ex = ar.lms(func, mu_of(func, g), int(g["ps"]), g[f"x{i}"][None], g[f"d{i}"][None], c, st, ex)
            assert y[0].tobytes() == g[f"out{i}"].tobytes() and e[0].tobytes() == g[f"err{i}"].tobytes(), (case, i)
        assert c[0].tobytes() == g["coeffs"].tobytes() and st[0].tobytes() == g["state"].tobytes(), case
        assert ex is None or ex[0].tobytes() == g["ex"].tobytes(), case


def test_decay_fixtures_pass_through_subnormals():
    for func, (dt, fam) in ar.FUNCS.items():
        if dt != np.float32:
            continue
        g = gold(func, "decay")
        if fam == "iir":
            assert subnormal(g["y0"]) and not g["state"].any(), func
        else:
            assert subnormal(g["x0"]) and subnormal(g["out0"]) and subnormal(g["state"]), func


def test_extreme_fixtures_saturate():
    for func, (dt, fam) in ar.FUNCS.items():
        if dt == np.float32:
            continue
        g = gold(func, "extreme")
        ends = [np.iinfo(dt).min, np.iinfo(dt).max]
        assert np.isin(g["state" if fam == "iir" else "coeffs"], ends).any(), func
        if fam == "nlms":
            assert int(g["ex"][0]) == 32767, func       # reciprocal argument 32772, wrapped to -32764


def test_converge_fixtures_converge():
    for func in LMS:
        g = gold(func, "converge")
        e = np.abs(np.concatenate([g["err0"], g["err1"]]).astype(np.float64))
        assert e[-65:].mean() < 0.5 * e[:65].mean(), func
        assert not g["coeffs0"].any() and g["coeffs"].any(), func


def test_struct_layout_matches_reference(tmp_path):
    """tools/abi_layout_adaptive.c compiled against include/ prints what it printed when compiled
    against the reference headers (tests/golden/abi_layout_adaptive.json); the ctypes mirrors agree."""
    exe = str(tmp_path / "abi_layout_adaptive")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "abi_layout_adaptive.c"),
                    "-o", exe], check=True)
    ours = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_layout_adaptive.json")))
    assert ours == ref and len(ref) == 8
    assert set(ref) == {v[0].__name__ for v in _abi.ADAPTIVE_FUNCS.values()}
    for name, lay in ref.items():
        st = getattr(_abi, name)
        assert C.sizeof(st) == lay["size"], name
        assert {f for f, _ in st._fields_} == set(lay) - {"size"}, name
        for fname, _ in st._fields_:
            assert getattr(st, fname).offset == lay[fname], (name, fname)


def test_library_exports_adaptive_symbols(dsp):
    names = FUNCS + INITS + [f + "_batch" for f in FUNCS]
    assert len(set(names)) == 24
    for n in names:
        assert callable(getattr(dsp.lib, n)), n
    C.c_int16.in_dll(dsp.lib, "armRecipTableQ15")


def test_recip_table_equals_reference_words(dsp):
    want = GOLD["armRecipTableQ15"]
    assert want.dtype == np.int16 and want.shape == (64,)
    got = np.array((C.c_int16 * 64).in_dll(dsp.lib, "armRecipTableQ15"), dtype=np.int16)
    assert got.tobytes() == want.tobytes()
    assert ar.recip_table().tobytes() == want.tobytes()


def test_norm_init_points_at_recip_table(dsp):
    S = _abi.arm_lms_norm_instance_q15()
    c, st = np.zeros(4, np.int16), np.full(4 + 8 - 1, 3, np.int16)
    S.energy, S.x0 = 9, 9
    dsp.lib.arm_lms_norm_init_q15(C.byref(S), 4, c.ctypes.data, st.ctypes.data, 123, 8, 2)
    assert S.recipTable == C.addressof(C.c_int16.in_dll(dsp.lib, "armRecipTableQ15"))
    assert (S.numTaps, S.mu, S.postShift, S.energy, S.x0) == (4, 123, 2, 0, 0) and not st.any()
    assert S.pCoeffs == c.ctypes.data and S.pState == st.ctypes.data


def test_cmsisdsp_module_exposes_adaptive_names():
    import cmsisdsp as d
    for n in FUNCS + INITS:
        assert callable(getattr(d, n)), n
    for inst in {v[0].__name__ for v in _abi.ADAPTIVE_FUNCS.values()}:
        assert callable(getattr(d, inst)), inst


# ------------------------------------------------------------------ GPU: drop-in against the fixtures
def mover(torch, where):
    """(to buffer, buffer's address, buffer's words) for host numpy arrays or device tensors."""
    if where == "host":
        return (lambda a: a.copy()), (lambda b: b.ctypes.data), (lambda b: b)
    return (lambda a: torch.from_numpy(a.copy()).cuda()), (lambda b: b.data_ptr()), (lambda b: b.cpu().numpy())


def dropin_iir(dsp, torch, func, g, where, alias):
    dt, _ = ar.FUNCS[func]
    inst, init, _ = _abi.ADAPTIVE_FUNCS[func]
    put, addr, words = mover(torch, where)
    n, bmax = len(g["k"]), max(len(g["x0"]), len(g["x1"]))
    k, v = g["k"].copy(), g["v"].copy()
    state = put(np.full(n + bmax, 77, dtype=dt))
    S = inst()
    getattr(dsp.lib, init)(C.byref(S), n, k.ctypes.data, v.ctypes.data, addr(state), bmax)
    assert dsp.last_error()[0] == 0, dsp.last_error()
    assert not words(state).any()                       # the init zeroes numStages + blockSize words
    for i in range(2):
        src = put(g[f"x{i}"])
        dst = src if alias else put(np.zeros_like(g[f"x{i}"]))
        getattr(dsp.lib, func)(C.byref(S), addr(src), addr(dst), len(g[f"x{i}"]))
        assert dsp.last_error()[0] == 0, dsp.last_error()
        assert words(dst).tobytes() == g[f"y{i}"].tobytes(), i
    assert words(state)[:n].tobytes() == g["state"].tobytes()


def dropin_lms(dsp, torch, func, g, where, alias):
    dt, fam = ar.FUNCS[func]
    inst, init, extra = _abi.ADAPTIVE_FUNCS[func]
    put, addr, words = mover(torch, where)
    n, bmax = len(g["coeffs0"]), max(len(g["x0"]), len(g["x1"]))
    coeffs = put(g["coeffs0"])
    state = put(np.full(n + bmax - 1, 77, dtype=dt))
    S = inst()
    if fam == "nlms":
        S.energy, S.x0 = 9, 9
    getattr(dsp.lib, init)(C.byref(S), n, addr(coeffs), addr(state), mu_of(func, g), bmax,
                           *([int(g["ps"])] if len(extra) == 2 else []))
    assert dsp.last_error()[0] == 0, dsp.last_error()
    assert not words(state).any()                       # the init zeroes numTaps + blockSize - 1 words
    for i in range(2):
        src, ref = put(g[f"x{i}"]), put(g[f"d{i}"])
        out = src if alias else put(np.zeros_like(g[f"x{i}"]))
        err = ref if alias else put(np.zeros_like(g[f"x{i}"]))
        getattr(dsp.lib, func)(C.byref(S), addr(src), addr(ref), addr(out), addr(err), len(g[f"x{i}"]))
        assert dsp.last_error()[0] == 0, dsp.last_error()
        assert words(out).tobytes() == g[f"out{i}"].tobytes(), i
        assert words(err).tobytes() == g[f"err{i}"].tobytes(), i
    assert words(coeffs).tobytes() == g["coeffs"].tobytes()
    assert words(state)[:n - 1].tobytes() == g["state"].tobytes()
    if fam == "nlms":
        assert np.array([S.energy, S.x0], dtype=dt).tobytes() == g["ex"].tobytes()


def dropin(dsp, torch, func, case, where, alias=False):
    (dropin_iir if ar.FUNCS[func][1] == "iir" else dropin_lms)(dsp, torch, func, gold(func, case), where, alias)


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_dropin_equals_fixtures(dsp, torch_gpu, func):
    """Host buffers, every fixture case (the extreme-word, subnormal-decay and convergence cases among them)."""
    for case in cases_of(func):
        dropin(dsp, torch_gpu, func, case, "host")


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_dropin_device_buffers(dsp, torch_gpu, func):
    """Signals, coefficients (LMS) and state all in device memory."""
    for case in ("n8_b130_130", "n70_b96_33", "n1_b1_1"):
        dropin(dsp, torch_gpu, func, case, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("where", ["host", "device"])
def test_dropin_aliased(dsp, torch_gpu, func, where):
    """IIR lattice: pDst == pSrc; LMS: pOut == pSrc and pErr == pRef."""
    for case in ("n3_b37_37", "n70_b96_33"):
        dropin(dsp, torch_gpu, func, case, where, alias=True)


@pytest.mark.gpu
def test_dropin_refuses_undefined_post_shift(dsp, torch_gpu):
    """postShift 15 (q15) / 31 (q31): a shift count outside 0...31 in the reference; reported, nothing written."""
    for func, ps in (("arm_lms_q15", 15), ("arm_lms_q31", 31), ("arm_lms_norm_q15", 15)):
        dt, _ = ar.FUNCS[func]
        inst, init, _ = _abi.ADAPTIVE_FUNCS[func]
        c, st = np.full(2, 5, dt), np.zeros(2 + 4 - 1, dt)
        x, d, y, e = np.full(4, 100, dt), np.full(4, 50, dt), np.full(4, 7, dt), np.full(4, 7, dt)
        S = inst()
        getattr(dsp.lib, init)(C.byref(S), 2, c.ctypes.data, st.ctypes.data, 1000, 4, ps)
        getattr(dsp.lib, func)(C.byref(S), x.ctypes.data, d.ctypes.data, y.ctypes.data, e.ctypes.data, 4)
        assert dsp.last_error()[0] != 0, func
        dsp.lib.arm_mi355x_clear_error()
        assert (y == 7).all() and (e == 7).all() and (c == 5).all(), func
        stream = C.c_void_p(torch_gpu.cuda.current_stream().cuda_stream)
        t = torch_gpu.zeros(16, dtype=tdtype(torch_gpu, dt), device="cuda")
        p = C.c_void_p(t.data_ptr())
        args = [C.byref(S), p, p, p, p, 4, 1, p, p] + ([p] if "norm" in func else []) + [stream]
        assert getattr(dsp.lib, func + "_batch")(*args) == _abi.ARM_MATH_ARGUMENT_ERROR, func
        dsp.lib.arm_mi355x_clear_error()


# ------------------------------------------------------------------ GPU: batched API against the restatement
def tdtype(torch, dt):
    return {np.float32: torch.float32, np.int32: torch.int32, np.int16: torch.int16}[dt]


@functools.lru_cache(maxsize=None)
def expected_iir(func, stages, blocks, batch):
    """(k, v, state0, [x], [y], [state after each call]) from the restatement, computed once."""
    dt, _ = ar.FUNCS[func]
    k, v = ar.lattice_coeffs(func, stages, 1000 + stages)
    st0 = ar.signal(func, (batch, stages), 3 * stages + batch, 0.25)
    st, xs, ys, sts = st0, [], [], []
    for i, b in enumerate(blocks):
        x = ar.signal(func, (batch, b), 7 * stages + b + i)
        y, st = ar.iir_lattice(func, k, v, x, st)
        xs.append(x), ys.append(y), sts.append(st)
    for a in [k, v, st0] + xs + ys + sts:
        a.setflags(write=False)
    return k, v, st0, xs, ys, sts


@functools.lru_cache(maxsize=None)
def expected_lms(func, taps, blocks, batch):
    """(mu, postShift, coeffs0, state0, ex0, [(x, d, out, err, coeffs, state, ex) per call]), computed once;
    every stream has its own coefficients, history and energy."""
    dt, fam = ar.FUNCS[func]
    mu, ps = ar.default_mu(func), (taps % 4 if dt != np.float32 else 0)
    rng = np.random.default_rng(50 * taps + batch)
    c0 = ar.quantise(rng.uniform(-0.3, 0.3, (batch, taps)) / 2.0 ** ps, dt)
    st0 = ar.signal(func, (batch, taps - 1), taps + batch + 1, 0.3)
    ex0 = None
    if fam == "nlms":      # energy well above the small magnitudes whose q15 reciprocal argument is undefined
        ex0 = np.stack([ar.quantise(rng.uniform(0.2, 0.6, batch), dt), ar.quantise(rng.uniform(-0.2, 0.2, batch), dt)], 1)
    c, st, ex, calls = c0, st0, ex0, []
    for i, b in enumerate(blocks):
        x, d = ar.signal(func, (batch, b), 9 * taps + b + i, 0.3), ar.signal(func, (batch, b), 11 * taps + b + i, 0.3)
        y, e, c, st, ex = ar.lms(func, mu, ps, x, d, c, st, ex)
        calls.append((x, d, y, e, c, st, ex))
    return mu, ps, c0, st0, ex0, calls


# (numStages, blocks of the two calls, batch).  Paths of iir_lattice.hip: the state in registers, instances of
# 4, 8, 16 and 32 stages, guard-free at exactly those counts (4 | 5, 8 | 9, 16 | 17, 32 | 33; 1, 2, 3 and 9 run
# guarded), in LDS up to 128 (128 | 129), beyond that in d_state (129, 300); I/O tiles of 32 samples, fetched one
# tile ahead (31 | 32 | 33, 65, 130) and 64 streams per wave (1, 63 | 64 | 65, 257); blocks shorter than the
# stage count.
IIR_CASES = [(1, (33, 31), 65), (2, (7, 9), 1), (3, (64, 96), 5), (4, (130, 64), 257), (5, (31, 2), 64),
             (8, (32, 1), 63), (9, (31, 33), 64), (16, (33, 32), 65), (17, (40, 2), 3), (32, (65, 3), 65),
             (33, (40, 2), 257), (128, (33, 5), 65), (129, (20, 13), 3), (300, (40, 7), 3)]
# (numTaps, blocks, batch).  Paths of lms.hip: coefficients and window in registers, instances of 4, 8, 16 and
# 32 taps, guard-free at exactly those counts (4 | 5, 8 | 9, 16 | 17, 32 | 33; 1, 2, 3 run guarded), coefficients
# and ring in LDS up to 64 taps (33, 64 | 65), beyond that in global memory (65, 300); numTaps 1 has no history;
# I/O tiles of 32 samples and 64 streams per wave as above; blocks shorter than the tap count (the ring never
# wraps) and longer (it wraps many times).
LMS_CASES = [(1, (33, 31), 65), (2, (7, 9), 1), (3, (32, 1), 63), (4, (130, 64), 257), (5, (33, 2), 64),
             (8, (65, 31), 65), (9, (31, 33), 3), (16, (33, 32), 65), (17, (31, 33), 64), (32, (65, 3), 257),
             (33, (40, 2), 65), (40, (5, 3), 2), (64, (40, 2), 65), (65, (20, 13), 5), (300, (40, 7), 3)]
ids = lambda v: str(v).replace(" ", "")   # noqa: E731


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same(t, want, what):
    assert t.cpu().numpy().tobytes() == want.tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("func,stages,blocks,batch", [(f, *c) for f in IIR for c in IIR_CASES], ids=ids)
def test_iir_lattice_batch_equals_restatement(dsp, torch_gpu, func, stages, blocks, batch):
    """Two consecutive calls, distinct states per stream carried on the device; d_src == d_dst on the second."""
    torch = torch_gpu
    k, v, st0, xs, ys, sts = expected_iir(func, stages, blocks, batch)
    kk, vv = k.copy(), v.copy()
    S = _abi.ADAPTIVE_FUNCS[func][0](numStages=stages, pState=None, pkCoeffs=kk.ctypes.data, pvCoeffs=vv.ctypes.data)
    state = torch.from_numpy(st0.copy()).cuda()
    f = getattr(dsp.lib, func + "_batch")
    for i, (x, y, st, b) in enumerate(zip(xs, ys, sts, blocks)):
        src = torch.from_numpy(x.copy()).cuda()
        dst = src if i else torch.zeros_like(src)
        rc = f(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), b, batch,
               C.c_void_p(state.data_ptr()), stream_of(torch))
        assert rc == 0, dsp.last_error()
        same(dst, y, ("dst", i))
        same(state, st, ("state", i))
        if not i:
            same(src, x, "src")


@pytest.mark.gpu
@pytest.mark.parametrize("func,taps,blocks,batch", [(f, *c) for f in LMS for c in LMS_CASES], ids=ids)
def test_lms_batch_equals_restatement(dsp, torch_gpu, func, taps, blocks, batch):
    """Two consecutive calls; coefficients, history and energy / x0 distinct per stream and carried on the
    device; d_out == d_src and d_err == d_ref on the second."""
    torch = torch_gpu
    dt, fam = ar.FUNCS[func]
    mu, ps, c0, st0, ex0, calls = expected_lms(func, taps, blocks, batch)
    inst = _abi.ADAPTIVE_FUNCS[func][0]
    kw = {"postShift": ps} if any(n == "postShift" for n, _ in inst._fields_) else {}
    S = inst(numTaps=taps, pState=None, pCoeffs=None, mu=mu, **kw)       # recipTable NULL: the library's table
    coeffs = torch.from_numpy(c0.copy()).cuda()
    state = torch.from_numpy(st0.copy()).cuda() if taps > 1 else None
    ex = torch.from_numpy(ex0.copy()).cuda() if fam == "nlms" else None
    f = getattr(dsp.lib, func + "_batch")
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
    for i, ((x, d, y, e, c, st, nex), b) in enumerate(zip(calls, blocks)):
        src, ref = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
        out, err = (src, ref) if i else (torch.zeros_like(src), torch.zeros_like(src))
        args = [C.byref(S), ptr(src), ptr(ref), ptr(out), ptr(err), b, batch, ptr(coeffs), ptr(state)]
        rc = f(*args, *([ptr(ex)] if fam == "nlms" else []), stream_of(torch))
        assert rc == 0, dsp.last_error()
        same(out, y, ("out", i))
        same(err, e, ("err", i))
        same(coeffs, c, ("coeffs", i))
        if taps > 1:
            same(state, st, ("state", i))
        if fam == "nlms":
            same(ex, nex, ("energy, x0", i))
        if not i:
            same(src, x, "src")
            same(ref, d, "ref")


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_batch_argument_errors(dsp, torch_gpu, func):
    torch = torch_gpu
    dt, fam = ar.FUNCS[func]
    inst = _abi.ADAPTIVE_FUNCS[func][0]
    t = torch.full((64,), 4, dtype=tdtype(torch, dt), device="cuda")
    p, nul = C.c_void_p(t.data_ptr()), C.c_void_p(None)
    f = getattr(dsp.lib, func + "_batch")
    err = _abi.ARM_MATH_ARGUMENT_ERROR
    if fam == "iir":
        k = np.zeros(3, dt)
        good = inst(numStages=2, pState=None, pkCoeffs=k.ctypes.data, pvCoeffs=k.ctypes.data)
        none = inst(numStages=0, pState=None, pkCoeffs=k.ctypes.data, pvCoeffs=k.ctypes.data)
        call = lambda S, a, blk=4, bat=2: f(C.byref(S), a[0], a[1], blk, bat, a[2], stream_of(torch))   # noqa: E731
        nptr = 3
    else:
        good, none = inst(numTaps=2, mu=1), inst(numTaps=0, mu=1)
        nptr = 7 if fam == "nlms" else 6
        call = lambda S, a, blk=4, bat=2: f(C.byref(S), *a[:4], blk, bat, *a[4:], stream_of(torch))   # noqa: E731
    assert call(none, [p] * nptr) == err
    for i in range(nptr):
        assert call(good, [nul if j == i else p for j in range(nptr)]) == err, i
    assert call(good, [p] * nptr, blk=0) == 0 and call(good, [p] * nptr, bat=0) == 0
    torch.cuda.synchronize()
    assert (t == 4).all().item()
    dsp.lib.arm_mi355x_clear_error()


@pytest.mark.gpu
@pytest.mark.parametrize("func", ["arm_iir_lattice_f32", "arm_iir_lattice_q15", "arm_lms_f32", "arm_lms_q31",
                                  "arm_lms_norm_q15"])
def test_cmsisdsp_module_adaptive(torch_gpu, func):
    """cmsisdsp_filtering.c call shapes: iir init (S, numStages, pkCoeffs, pvCoeffs, pState), (S, pSrc) -> pDst;
    lms init (S, numTaps, pCoeffs, pState, mu[, postShift]), (S, pSrc, pRef, pErr) -> pOut.  Init plus two calls
    equal the fixtures."""
    import cmsisdsp as d
    dt, fam = ar.FUNCS[func]
    inst, init, extra = _abi.ADAPTIVE_FUNCS[func]
    for case in ("n3_b37_37", "n8_b130_130"):
        g = gold(func, case)
        S = getattr(d, inst.__name__)()
        if fam == "iir":
            getattr(d, init)(S, len(g["k"]), g["k"], g["v"], np.zeros(len(g["k"]) + 130))
            for i in range(2):
                got = getattr(d, func)(S, g[f"x{i}"])
                assert got.dtype == dt and got.tobytes() == g[f"y{i}"].tobytes(), case
            continue
        n = len(g["coeffs0"])
        getattr(d, init)(S, n, g["coeffs0"], np.zeros(n + 130 - 1), mu_of(func, g),
                         *([int(g["ps"])] if len(extra) == 2 else []))
        for i in range(2):
            e = np.zeros(len(g[f"x{i}"]), dtype=dt)
            got = getattr(d, func)(S, g[f"x{i}"], g[f"d{i}"], e)
            assert got.dtype == dt and got.tobytes() == g[f"out{i}"].tobytes(), case
            assert e.tobytes() == g[f"err{i}"].tobytes(), case
        assert S.coeffs().tobytes() == g["coeffs"].tobytes(), case
