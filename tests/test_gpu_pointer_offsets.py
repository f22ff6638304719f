"""The transform, filter, GEMM and MFCC kernels under pointer offsets and guard bands.

The reference API takes any element-aligned pointer (a q15_t* at 2 bytes, a float32_t* at 4); a
freshly allocated device tensor is 512-B aligned, so the other GPU tests only ever hand the kernels
addresses = 0 mod 16.  Here every operand that is a device pointer -- data, state, output, and the
device-resident pCoeffs / pTapDelay / pTwiddle where the case names one -- is a view at an element
offset into a guarded flat buffer (tests/padded.py):

* an aligned control run first; then each operand offset alone with the others at 0 (4-byte types
  by 1, 2, 3 elements, 2-byte types by 1, 2, 4, q7 by 1, 2, 4, 8); then all operands together;
* outputs, and states where the entry point updates one, equal the reference build's words byte
  for byte (f32: assert_same_words; f32 GEMM: oracle.mat_mult_fmaf; MFCC f32: mfcc_cfg's parity);
* every pad of every operand keeps its fill (a store outside an operand);
* integer cases run twice, the pads holding 0x55.. and then 0xAA..: both runs must give the
  reference's words, so no output depends on a word outside an input.  f32 inputs sit between NaN
  pads: a word read from outside and used poisons an output.

Inputs and reference outputs are built once per case (functools.lru_cache) and all failing
(mode, offset) pairs of a case are reported in one assertion message.  Two tests are not marked gpu:
test_case_table_reference_ignores_pads builds every case on the CPU, and
test_runner_reports_planted_defects runs the runner itself on CPU-backed operands with toy kernels
that store or read one element outside an operand.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import mfcc_cfg
import refs
from cmsisdsp_amd import _abi
from f32_classes import assert_same_words
from padded import F32_SENTINEL, FILL_A, FILL_B, NAN_FILL, Padded

DT = refs.DTYPE
OFFSETS = {4: (1, 2, 3), 2: (1, 2, 4), 1: (1, 2, 4, 8)}
TABLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmsis-dsp_amd", "tables")


def _base(kind):
    return kind.split("_")[-1]


def _rand(kind, shape, rng):
    """Random full-range words (f32: uniform in [-1, 1))."""
    if kind == "f32":
        return rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    info = np.iinfo(DT[kind])
    return rng.integers(info.min, info.max, shape, endpoint=True).astype(DT[kind])


def _ptr(a):
    return a.ctypes.data


class Op:
    """One device-pointer operand.  role: "in" (read only), "io" (read and written), "out",
    "state" (zeroed before the first call, carried between calls)."""

    def __init__(self, name, dt, shape, role, offsets=None):
        self.name, self.dt, self.role = name, np.dtype(dt), role
        self.shape = tuple(shape) if hasattr(shape, "__len__") else (shape,)
        self.offsets = tuple(offsets) if offsets is not None else OFFSETS[self.dt.itemsize]


class Case:
    """A row of the table: its operands, inputs(), expect(inputs) on the reference, launch() on the
    product.  inputs(): name -> array (put once) or list of arrays (one per call).  expect():
    (per call: name -> words | (words, untouched mask), after the last call: name -> words)."""
    ncalls = 1
    f32 = False
    compare = None                          # None: byte equality / assert_same_words; "mfcc_f32"

    def __init__(self, family, cid, ops):
        self.family, self.id, self.ops = family, f"{family}-{cid}", ops


CASES = {}
_TOYS = {}                                  # the runner's own negative controls (CPU)


def _add(case):
    assert case.id not in CASES, case.id
    CASES[case.id] = case


# ------------------------------------------------------------------ CFFT
class Cfft(Case):
    def __init__(self, kind, n, ifft, bitrev, batch, tw=False):
        self.kind, self.n, self.ifft, self.bitrev, self.batch, self.tw = kind, n, ifft, bitrev, batch, tw
        self.f32 = kind == "f32"
        ops = [Op("data", DT[kind], (batch, 2 * n), "io")]
        if tw:
            ops.append(Op("tw", DT[kind], (2 * n if kind == "f32" else 3 * n // 2,), "in", offsets=(1,)))
        super().__init__("cfft", f"{kind}-{n}-ifft{ifft}-brev{bitrev}" + ("-tw" if tw else ""), ops)

    def inputs(self):
        seed = 1000 * self.n + 7 * self.ifft + 3 * self.bitrev
        x = {"data": [np.stack([refs.rand_input(self.kind, 2 * self.n, seed=seed + r) for r in range(self.batch)])]}
        if self.tw:
            suffix = "" if self.kind == "f32" else "_" + self.kind
            x["tw"] = np.fromfile(os.path.join(TABLES, f"twiddleCoef_{self.n}{suffix}.bin"), dtype=DT[self.kind])
        return x

    def expect(self, x):
        r = refs.ref_lib()
        S = r.cfft_instance(self.kind, self.n)
        if self.tw:                          # the reference reads the caller's table too
            S.pTwiddle = C.cast(_ptr(x["tw"]), type(S.pTwiddle))
        out = np.ascontiguousarray(x["data"][0]).copy()
        f = r.fn(f"arm_cfft_{self.kind}")
        for row in out:
            f(C.byref(S), _ptr(row), self.ifft, self.bitrev)
        return [{"data": out}], {}

    def launch(self, dsp, torch, T, call):
        S = getattr(dsp, f"arm_cfft_instance_{self.kind}")()
        assert getattr(dsp, f"arm_cfft_init_{self.kind}")(S, self.n) == 0
        if self.tw:
            S.pTwiddle = C.cast(T["tw"].ptr, type(S.pTwiddle))
        dsp.cfft_batch(S, T["data"].t, self.ifft, self.bitrev)


for _k in ("f32", "q31", "q15"):
    # f32 N <= 256 and fixed-point N <= 128: the generic kernels, several transforms per workgroup and
    # a ragged last one; beyond them the specialists (fixed-point 256 .. 2048: the radix-16 kernel)
    for _n in (16, 64, 256, 512, 1024, 2048, 4096) + ((128,) if _k != "f32" else ()):
        _b = 37 if _n <= 256 else 5
        for _f in ((0, 1), (1, 1)) + (((0, 0),) if _n in (256, 1024) else ()):
            _add(Cfft(_k, _n, _f[0], _f[1], _b))
for _k, _n in (("f32", 1024), ("f32", 64), ("q15", 256), ("q15", 4096), ("q31", 1024)):
    _add(Cfft(_k, _n, 0, 1, 37 if _n <= 256 else 5, tw=True))


# ------------------------------------------------------------------ RFFT fast f32
class RfftFast(Case):
    f32 = True

    def __init__(self, n, ifft, p_scratch, batch=5):
        self.n, self.ifft, self.p_scratch, self.batch = n, ifft, p_scratch, batch
        super().__init__("rfft_fast", f"{n}-ifft{ifft}" + ("-pscratch" if p_scratch else ""),
                         [Op("p", np.float32, (batch, n), "io"), Op("out", np.float32, (batch, n), "out")])

    def inputs(self):
        return {"p": [np.stack([refs.rand_input("f32", self.n, seed=self.n + r + 100 * self.ifft)
                                for r in range(self.batch)])]}

    def expect(self, x):
        r = refs.ref_lib()
        rows = [r.rfft(self.n, row, self.ifft) for row in x["p"][0]]
        want = {"out": np.stack([o for o, _ in rows])}
        if not self.p_scratch or self.ifft:   # where test_rfft_batch_bitexact compares p
            want["p"] = np.stack([p for _, p in rows])
        return [want], {}

    def launch(self, dsp, torch, T, call):
        S = dsp.const_instance(f"arm_rfft_fast_sR_f32_len{self.n}")
        dsp.rfft_fast_batch(S, T["p"].t, T["out"].t, self.ifft, p_scratch=self.p_scratch)


for _n in (32, 256, 1024, 2048, 4096):
    for _f in (0, 1, 2):
        for _s in (False, True):
            _add(RfftFast(_n, _f, _s))


# ------------------------------------------------------------------ RFFT q31 / q15
class RfftFixed(Case):
    """tw: the inner CFFT's pTwiddle (a private copy of the instance init made) in device memory at
    element offset 1, as the CFFT rows: the RFFT reaches the same q15 kernels."""

    def __init__(self, kind, n, ifft, batch=5, tw=False):
        self.kind, self.n, self.ifft, self.batch, self.tw = kind, n, ifft, batch, tw
        self.win, self.wout = (2 * n, n) if ifft == 1 else (n, 2 * n)
        ops = [Op("src", DT[kind], (batch, self.win), "io"), Op("dst", DT[kind], (batch, self.wout), "out")]
        if tw:
            ops.append(Op("tw", DT[kind], (3 * (n // 2) // 2,), "in", offsets=(1,)))
        super().__init__("rfft_fixed", f"{kind}-{n}-ifft{ifft}" + ("-tw" if tw else ""), ops)

    def inputs(self):
        x = {"src": [np.stack([refs.rand_input(self.kind, self.win, seed=self.n + r + 50 * self.ifft)
                               for r in range(self.batch)])]}
        if self.tw:
            x["tw"] = np.fromfile(os.path.join(TABLES, f"twiddleCoef_{self.n // 2}_{self.kind}.bin"), dtype=DT[self.kind])
        return x

    def _instance(self, lib_init, tw_ptr):
        """(S, keep): an initialised instance; tw_ptr: its inner CFFT instance replaced by a copy
        whose pTwiddle is tw_ptr."""
        S = _abi.arm_rfft_instance_q31() if self.kind == "q31" else _abi.arm_rfft_instance_q15()
        assert lib_init(C.byref(S), self.n, self.ifft, 1) == 0
        inner = None
        if tw_ptr is not None:
            inner = type(S.pCfft.contents)()
            C.memmove(C.byref(inner), S.pCfft, C.sizeof(inner))
            inner.pTwiddle = C.cast(tw_ptr, type(inner.pTwiddle))
            S.pCfft = C.pointer(inner)
        return S, inner

    def expect(self, x):
        r = refs.ref_lib()
        S, _keep = self._instance(r.fn(f"arm_rfft_init_{self.kind}"), _ptr(x["tw"]) if self.tw else None)
        src = np.ascontiguousarray(x["src"][0]).copy()
        dst = np.zeros((self.batch, self.wout), DT[self.kind])
        f = r.fn(f"arm_rfft_{self.kind}")
        for i in range(self.batch):
            f(C.byref(S), _ptr(src[i]), _ptr(dst[i]))
        want = {"dst": dst}
        if self.ifft != 1:                   # the forward transform overwrites its input
            want["src"] = src
        return [want], {}

    def launch(self, dsp, torch, T, call):
        S, _keep = self._instance(getattr(dsp.lib, f"arm_rfft_init_{self.kind}"), T["tw"].ptr if self.tw else None)
        dsp.rfft_fixed_batch(S, T["src"].t, T["dst"].t)


for _k in ("q31", "q15"):
    for _n in (32, 512, 1024, 4096, 8192):
        for _f in (0, 1):
            _add(RfftFixed(_k, _n, _f))
for _n, _f in ((512, 0), (512, 1), (8192, 0)):   # the radix-16 kernel both ways, the 4096 kernel with the fused split
    _add(RfftFixed("q15", _n, _f, tw=True))


# ------------------------------------------------------------------ streaming filters: two calls, the state carried
class Stream(Case):
    """src [batch, block] -> dst [batch, nout] twice, hist / state [batch, H] carried, coefficients
    (and the sparse tap delays) resident in device memory."""
    ncalls = 2

    def _stream_inputs(self, kind, ncoef, seed, scale=True):
        rng = np.random.default_rng(seed)
        c = _rand(kind, ncoef, rng)
        if kind == "f32" and scale:
            c = (c / np.sqrt(ncoef)).astype(np.float32)
        return {"coeffs": c, "src": [_rand(kind, (self.batch, self.block), rng) for _ in range(2)]}

    @staticmethod
    def _stack(per_filter, H):
        """per_filter: [(outs[call], state)] -> ([{dst}, {dst}], {hist})"""
        calls = [{"dst": np.stack([o[k] for o, _ in per_filter])} for k in range(2)]
        final = {"hist": np.stack([s[:H] for _, s in per_filter])} if H else {}
        return calls, final


class Fir(Stream):
    def __init__(self, kind, taps, block, batch=5):
        self.kind, self.taps, self.block, self.batch = kind, taps, block, batch
        self.f32 = kind == "f32"
        dt = DT[_base(kind)]
        super().__init__("fir", f"{kind}-{taps}-{block}",
                         [Op("src", dt, (batch, block), "in"), Op("dst", dt, (batch, block), "out"),
                          Op("hist", dt, (batch, taps - 1), "state"), Op("coeffs", dt, (taps,), "in")])

    def inputs(self):
        return self._stream_inputs(_base(self.kind), self.taps, self.taps * 7 + self.block)

    def expect(self, x):
        r = refs.ref_lib()
        return self._stack([r.fir(self.kind, x["coeffs"], [x["src"][0][f], x["src"][1][f]])
                            for f in range(self.batch)], self.taps - 1)

    def launch(self, dsp, torch, T, call):
        S = getattr(dsp, f"arm_fir_instance_{_base(self.kind)}")()
        S.numTaps = self.taps
        S.pCoeffs = C.cast(T["coeffs"].ptr, S._fields_[2][1])
        dsp.fir_batch(S, T["src"].t, T["dst"].t, T["hist"].t, kind=self.kind)


for _k in ("f32", "q15", "q31", "fast_q15", "fast_q31", "q7"):
    # batch 5 stays below the MFMA threshold: the VALU kernels.  (32, 512): block % 8 == 0, the 16-B
    # store when dst allows; (130, 2049): a second chunk; (1030, 300): the long-filter kernels
    for _t, _b in ((29, 32), (32, 512), (130, 2049), (1030, 300)):
        _add(Fir(_k, _t + (_t & 1 if _k.endswith("q15") else 0), _b))


class Multirate(Stream):
    def __init__(self, fn, taps, factor, block, batch=5):
        self.fn, self.taps, self.factor, self.block, self.batch = fn, taps, factor, block, batch
        self.decim = fn.startswith("decimate")
        self.f32 = fn.endswith("f32")
        self.H = taps - 1 if self.decim else taps // factor - 1
        self.nout = block // factor if self.decim else block * factor
        dt = DT[_base(fn)]
        super().__init__("multirate", f"{fn}-{taps}-{factor}-{block}",
                         [Op("src", dt, (batch, block), "in"), Op("dst", dt, (batch, self.nout), "out"),
                          Op("hist", dt, (batch, self.H), "state"), Op("coeffs", dt, (taps,), "in")])

    def inputs(self):
        return self._stream_inputs(_base(self.fn), self.taps, self.taps * 5 + self.factor + self.block)

    def expect(self, x):
        r = refs.ref_lib()
        rows = []
        for f in range(self.batch):
            st, outs, state = r.multirate(self.fn, self.factor, x["coeffs"], [x["src"][0][f], x["src"][1][f]])
            assert st == 0
            rows.append((outs, state))
        return self._stack(rows, self.H)

    def launch(self, dsp, torch, T, call):
        if self.decim:
            S = _abi.arm_fir_decimate_instance(M=self.factor, numTaps=self.taps, pCoeffs=T["coeffs"].ptr, pState=None)
        else:
            S = _abi.arm_fir_interpolate_instance(L=self.factor, phaseLength=self.taps // self.factor,
                                                  pCoeffs=T["coeffs"].ptr, pState=None)
        st = getattr(dsp.lib, f"arm_fir_{self.fn}_batch")(
            C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block, self.batch,
            C.c_void_p(T["hist"].ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, dsp.last_error()


# the eight multirate entry points the library has (five decimators, three interpolators)
for _fn in ("decimate_f32", "decimate_q15", "decimate_fast_q15", "decimate_q31", "decimate_fast_q31"):
    for _m in (2, 5):                        # M = 2: the FIR pass; M = 5: the decimator's own kernel
        _add(Multirate(_fn, 30, _m, 100))
for _fn in ("interpolate_f32", "interpolate_q15", "interpolate_q31"):
    for _t, _l in ((32, 2), (30, 5)):
        for _b in (50, 64):                  # 64: the four-inputs-per-lane kernel's N % 4 == 0
            _add(Multirate(_fn, _t, _l, _b))


class Sparse(Stream):
    def __init__(self, kind, taps, max_delay, block, batch=5):
        self.kind, self.taps, self.max_delay, self.block, self.batch = kind, taps, max_delay, block, batch
        self.f32 = kind == "f32"
        dt = DT[kind]
        super().__init__("sparse", f"{kind}-{taps}-{max_delay}-{block}",
                         [Op("src", dt, (batch, block), "in"), Op("dst", dt, (batch, block), "out"),
                          Op("hist", dt, (batch, max_delay), "state"), Op("coeffs", dt, (taps,), "in"),
                          Op("delays", np.int32, (taps,), "in")])

    def inputs(self):
        x = self._stream_inputs(self.kind, self.taps, self.taps * 3 + self.max_delay)
        rng = np.random.default_rng(self.max_delay)
        d = rng.integers(0, self.max_delay, self.taps, endpoint=True).astype(np.int32)
        d[0], d[1] = self.max_delay, 0
        d[2] = d[0]                          # a repeated delay
        x["delays"] = d
        return x

    def expect(self, x):
        r = refs.ref_lib()
        rows = []
        for f in range(self.batch):
            xs = [x["src"][0][f], x["src"][1][f]]
            outs, _, _ = r.sparse(self.kind, x["coeffs"], x["delays"], self.max_delay, xs)
            # d_hist carries the last maxDelay samples (test_sparse_batch_bitexact)
            tail = np.concatenate([np.zeros(self.max_delay, DT[self.kind])] + [np.asarray(v) for v in xs])
            rows.append((outs, tail[-self.max_delay:]))
        return self._stack(rows, self.max_delay)

    def launch(self, dsp, torch, T, call):
        S = _abi.arm_fir_sparse_instance(numTaps=self.taps, pCoeffs=T["coeffs"].ptr, maxDelay=self.max_delay,
                                         pTapDelay=T["delays"].ptr)
        st = getattr(dsp.lib, f"arm_fir_sparse_{self.kind}_batch")(
            C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block, self.batch,
            C.c_void_p(T["hist"].ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, dsp.last_error()


for _k in ("f32", "q31", "q15", "q7"):
    for _d in (20, 12300):                   # the LDS-staged kernel; the direct-read kernel
        _add(Sparse(_k, 16, _d, 100))


class Lattice(Stream):
    def __init__(self, kind, stages, block, batch):
        self.kind, self.stages, self.block, self.batch = kind, stages, block, batch
        self.f32 = kind == "f32"
        dt = DT[kind]
        super().__init__("lattice", f"{kind}-{stages}-{block}-{batch}",
                         [Op("src", dt, (batch, block), "in"), Op("dst", dt, (batch, block), "out"),
                          Op("hist", dt, (batch, stages), "state"), Op("coeffs", dt, (stages,), "in")])

    def inputs(self):
        x = self._stream_inputs(self.kind, self.stages, self.stages * 13 + self.block, scale=False)
        if self.f32:
            x["coeffs"] = (x["coeffs"] * np.float32(0.9)).astype(np.float32)
        return x

    def expect(self, x):
        r = refs.ref_lib()
        return self._stack([r.lattice(self.kind, x["coeffs"], [x["src"][0][f], x["src"][1][f]])
                            for f in range(self.batch)], self.stages)

    def launch(self, dsp, torch, T, call):
        S = _abi.arm_fir_lattice_instance(numStages=self.stages, pState=None, pCoeffs=T["coeffs"].ptr)
        st = getattr(dsp.lib, f"arm_fir_lattice_{self.kind}_batch")(
            C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block, self.batch,
            C.c_void_p(T["hist"].ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, dsp.last_error()


for _k in ("f32", "q31", "q15"):
    for _s, _b, _n in ((8, 100, 5), (33, 257, 70)):
        _add(Lattice(_k, _s, _b, _n))


# ------------------------------------------------------------------ convolution / correlation
def _partial_range(la, lb):
    """partial_range of test_f32_classes.py: starts inside the head, ends among the full overlaps."""
    return 3, min(la, lb) + 14


class Conv(Case):
    """The batched entry points (FULL + PARTIAL: partial outputs compact), and the scratch-buffer
    _opt names, which only exist as drop-ins: one call per item on device pointers into the same
    three operands, host scratch.  The words an entry point leaves alone (correlate with unequal
    lengths; a partial call's words outside its range) must keep the caller's fill."""
    batch = 3

    def __init__(self, fn, la, lb):
        self.fn, self.la, self.lb = fn, la, lb
        self.kind = fn.split("_")[-1]
        self.f32 = self.kind == "f32"
        self.opt = "_opt" in fn
        self.partial = fn.startswith("conv_partial")
        self.first, self.num = _partial_range(la, lb) if self.partial else (0, 0)
        full = 2 * max(la, lb) - 1 if fn.startswith("correlate") else la + lb - 1
        self.width = self.num if self.partial and not self.opt else full
        dt = DT[self.kind]
        super().__init__("conv", f"{fn}-{la}-{lb}",
                         [Op("a", dt, (self.batch, la), "in"), Op("b", dt, (self.batch, lb), "in"),
                          Op("out", dt, (self.batch, self.width), "out")])

    def inputs(self):
        rng = np.random.default_rng(self.la * 3 + self.lb)
        return {"a": _rand(self.kind, (self.batch, self.la), rng), "b": _rand(self.kind, (self.batch, self.lb), rng)}

    def _scratch(self):
        return [np.zeros(self.la + 2 * self.lb + 16, np.int16) for _ in range(2)]

    def _dropin(self, h, a, la, b, lb, y):
        """One call of the _opt drop-in of library h on raw pointers."""
        s1, s2 = self._scratch()
        f = h.fn(f"arm_{self.fn}")
        if self.partial:
            assert f(a, la, b, lb, y, self.first, self.num, _ptr(s1), _ptr(s2)) == 0
        elif _abi.CONV_OPT_FULL[self.fn] == 2:
            f(a, la, b, lb, y, _ptr(s1), _ptr(s2))
        else:
            f(a, la, b, lb, y, _ptr(s1))

    def _ref_row(self, a, b, fill):
        r = refs.ref_lib()
        if not self.opt:
            y, st = r.conv_family(self.fn, a, b, self.first, self.num, fill=fill)
            assert st == 0
            return y[self.first:self.first + self.num] if self.partial else y
        y = np.full(self.width, fill, DT[self.kind])
        self._dropin(r, _ptr(a), len(a), _ptr(b), len(b), _ptr(y))
        return y

    def expect(self, x):
        # two fills: the words that follow the fill are the ones the reference leaves alone
        y1 = np.stack([self._ref_row(x["a"][i], x["b"][i], 1) for i in range(self.batch)])
        y2 = np.stack([self._ref_row(x["a"][i], x["b"][i], 2) for i in range(self.batch)])
        untouched = y1.view(np.uint8).reshape(y1.shape + (-1,)) != y2.view(np.uint8).reshape(y2.shape + (-1,))
        return [{"out": (y1, untouched.any(axis=-1))}], {}

    def launch(self, dsp, torch, T, call):
        if not self.opt:
            dsp.conv_family_batch(self.fn, T["a"].t, T["b"].t, T["out"].t, self.first, self.num)
            return
        h = _product(dsp)
        size = np.dtype(DT[self.kind]).itemsize
        for i in range(self.batch):
            self._dropin(h, T["a"].ptr + i * self.la * size, self.la, T["b"].ptr + i * self.lb * size, self.lb,
                         T["out"].ptr + i * self.width * size)
            dsp._check_void(self.fn)


@functools.lru_cache(maxsize=None)
def _product(dsp):
    return refs.Host(dsp.lib, "")


for _fn in list(_abi.CONV_FULL) + list(_abi.CONV_PARTIAL) + list(_abi.CONV_OPT_FULL) + list(_abi.CONV_OPT_PARTIAL):
    for _la, _lb in ((50, 7), (7, 50), (1100, 1030)):   # both orders; srcBLen > 1024: the direct kernel
        _add(Conv(_fn, _la, _lb))


# ------------------------------------------------------------------ real GEMMs
class Gemm(Case):
    batch = 2

    def __init__(self, kind, m, k, n):
        self.kind, self.m, self.k, self.n = kind, m, k, n
        self.f32 = kind == "f32"
        dt = DT[_base(kind)]
        super().__init__("gemm", f"{kind}-{m}-{k}-{n}",
                         [Op("a", dt, (self.batch, m, k), "in"), Op("b", dt, (self.batch, k, n), "in"),
                          Op("c", dt, (self.batch, m, n), "out")])

    def inputs(self):
        rng = np.random.default_rng(self.m + 3 * self.k + 7 * self.n)
        return {"a": _rand(_base(self.kind), (self.batch, self.m, self.k), rng),
                "b": _rand(_base(self.kind), (self.batch, self.k, self.n), rng)}

    def expect(self, x):
        rows = []
        for i in range(self.batch):
            if self.f32:                     # the product's stated k-ordered fmaf chain, as today
                st, c = refs.oracle_lib().mat_mult_fmaf(x["a"][i], x["b"][i])
            elif self.kind == "q7" and self.m * self.n > 65536:
                # arm_mat_mult_q7 keeps its output row offset in a uint16_t (arm_mat_mult_q7.c:704,:782)
                # and writes later rows over earlier ones: the reference on the rows it places, the
                # exact formula (which it equals there) on the rest, as test_mat_mult_q7_bitexact
                rows_ok = 65536 // self.n
                st, head = refs.ref_lib().mat_mult_fixed("q7", x["a"][i][:rows_ok], x["b"][i])
                s = np.matmul(np.asarray(x["a"][i], np.int64), np.asarray(x["b"][i], np.int64))
                c = np.clip(s >> 7, -128, 127).astype(np.int8)
                assert head.tobytes() == c[:rows_ok].tobytes()
            else:
                st, c = refs.ref_lib().mat_mult_fixed(self.kind, x["a"][i], x["b"][i])
            assert st == 0
            rows.append(c)
        return [{"c": np.stack(rows)}], {}

    def launch(self, dsp, torch, T, call):
        dsp.mat_mult_batch(T["a"].t, T["b"].t, T["c"].t, fast=self.kind.startswith("fast"))


# whole-tile shapes (an offset must leave the unguarded kernel), then ragged ones
for _k, _s in (("f32", (128, 16, 128)), ("q15", (128, 64, 128)), ("q31", (128, 64, 128)), ("fast_q15", (128, 64, 128)),
               ("fast_q31", (64, 64, 64)), ("q7", (256, 64, 256)), ("q7", (256, 128, 256)), ("q7", (256, 192, 256)),
               ("f32", (65, 77, 33)), ("q15", (65, 130, 67)), ("q31", (65, 130, 67)), ("fast_q15", (65, 130, 67)),
               ("fast_q31", (65, 130, 67)), ("q7", (256, 80, 272))):
    _add(Gemm(_k, *_s))


# ------------------------------------------------------------------ MFCC
def _fixed(a, bits):
    return np.clip(np.round(np.asarray(a, np.float64) * 2.0**bits), -2**bits, 2**bits - 1).astype(
        np.int32 if bits == 31 else np.int16)


class Mfcc(Case):
    def __init__(self, kind, n, work, batch=6):
        self.kind, self.n, self.work, self.batch = kind, n, work, batch
        self.f32 = kind == "f32"
        if self.f32:
            self.compare = "mfcc_f32"
        self.cfg = mfcc_cfg.make_cfg(n)
        if not self.f32:
            bits = 31 if kind == "q31" else 15
            self.cfg = dict(self.cfg, **{k: _fixed(self.cfg[k], bits) for k in ("dct", "coefs", "window")})
        dt = DT[kind]
        ops = [Op("frames", dt, (batch, n), "io"), Op("out", dt, (batch, self.cfg["dct"].shape[0]), "out")]
        if work:                             # the wrapper's own shapes: f32 as frames, fixed 2 * fftLen words
            ops.append(Op("work", dt, (batch, n if self.f32 else 2 * n), "out"))
        super().__init__("mfcc", f"{kind}-{n}" + ("-work" if work else ""), ops)

    def inputs(self):
        rng = np.random.default_rng(7 * self.n)
        if self.f32:
            f = rng.uniform(-1, 1, (self.batch, self.n)).astype(np.float32)
            f[3] = 0.0                       # max == 0: no normalisation (arm_mfcc_f32.c:102)
            f[5] = np.sin(np.arange(self.n) * 0.3).astype(np.float32) * 1e4
        else:                                # frames_for of test_mfcc_q31.py / _q15.py
            top = 30 if self.kind == "q31" else 14
            f = rng.integers(-2**top, 2**top, (self.batch, self.n)).astype(DT[self.kind])
            f[1] = 0
            f[2] = rng.integers(-3, 4, self.n)
            f[3, 5] = -2**(top + 1)
            f[5] = rng.integers(-1, 2, self.n)
            f[5, 3] = -1
        return {"frames": [f]}

    def expect(self, x):
        r = refs.ref_lib()
        fn = {"f32": r.mfcc, "q31": r.mfcc_q31, "q15": r.mfcc_q15}[self.kind]
        return [{"out": fn(self.cfg, x["frames"][0])}], {}

    def launch(self, dsp, torch, T, call):
        cls = {"f32": dsp.MfccF32, "q31": dsp.MfccQ31, "q15": dsp.MfccQ15}[self.kind]
        c = self.cfg
        m = cls(self.n, c["dct"], c["pos"], c["len"], c["coefs"], c["window"])
        m.batch(T["frames"].t, T["out"].t, T["work"].t if self.work else None)


for _k in ("f32", "q31", "q15"):
    for _n in (256, 1024):
        for _w in (False, True):
            _add(Mfcc(_k, _n, _w))


# ------------------------------------------------------------------ the runner
@functools.lru_cache(maxsize=None)
def _built(cid):
    """(inputs, expected words per call, expected words after the last call), once per case."""
    case = CASES.get(cid) or _TOYS[cid]
    x = case.inputs()
    calls, final = case.expect(x)
    for d in calls + [final]:
        for w in d.values():
            (w[0] if isinstance(w, tuple) else w).setflags(write=False)
    return x, calls, final


def _ids(family):
    return [cid for cid, c in CASES.items() if c.family == family]


def _modes(case):
    """("aligned", {}), then (operand, {operand: o}) for each operand and offset, then ("all", {...})."""
    yield "aligned", {}
    for op in case.ops:
        for o in op.offsets:
            yield op.name, {op.name: o}
    for i in range(max(len(op.offsets) for op in case.ops)):
        yield "all", {op.name: op.offsets[min(i, len(op.offsets) - 1)] for op in case.ops}


def _op_fill(op, fill):
    """The pad fill of one operand: integer operands take the run's fill; f32 inputs sit between
    NaNs, f32 outputs and states between finite sentinels."""
    if op.dt != np.float32:
        return fill
    return NAN_FILL if op.role in ("in", "io") else F32_SENTINEL


def _diff(case, got, want, word):
    """None, or what differs.  want: words, or (words, mask of the words the call leaves alone)."""
    mask = None
    if isinstance(want, tuple):
        want, mask = want
    if mask is not None and mask.any():
        bits = got.view(f"int{8 * got.dtype.itemsize}")
        if not (bits[mask] == word).all():
            return f"{int((bits[mask] != word).sum())} words the reference leaves alone were written"
        got, want = got[~mask], want[~mask]
    if case.compare == "mfcc_f32":
        ok, _, _ = mfcc_cfg.host_libm_status()
        if not ok:                           # another libm: the reference suite's tolerance (mfcc_cfg.assert_parity)
            good = np.abs(got - want) <= 1e-5 + 1.2e-3 * np.abs(want)
            return None if good.all() else f"beyond the suite tolerance at {np.argwhere(~good)[:4].tolist()}"
    if case.f32:
        try:
            assert_same_words(got, want)
        except AssertionError as e:
            return str(e)
        return None
    if got.tobytes() != want.tobytes():
        idx = np.argwhere(got != want)
        return f"{len(idx)} words differ, first at {idx[:4].tolist()}"
    return None


def _run(case, dsp, torch, device="cuda"):
    x, calls, final = _built(case.id)
    bad, seen = [], {}
    for fill in ((FILL_A,) if case.f32 else (FILL_A, FILL_B)):   # f32 cases: FILL_A for their integer tables
        for mode, offs in _modes(case):
            tag = ("pads NaN" if case.f32 else f"pads 0x{fill:02X}", mode, sorted(offs.items()))
            T = {op.name: Padded(torch, op.dt, op.shape, offs.get(op.name, 0), _op_fill(op, fill), device=device)
                 for op in case.ops}
            for op in case.ops:
                if op.role == "state":
                    T[op.name].t.zero_()
                elif op.name in x and not isinstance(x[op.name], list):
                    T[op.name].put(torch, x[op.name])
            for k in range(case.ncalls):
                for op in case.ops:
                    if op.role == "out":
                        T[op.name].reset()
                    elif isinstance(x.get(op.name), list):
                        T[op.name].put(torch, x[op.name][k])
                case.launch(dsp, torch, T, k)
                if device == "cuda":
                    torch.cuda.synchronize()
                for name, want in list(calls[k].items()) + (list(final.items()) if k == case.ncalls - 1 else []):
                    got = T[name].fetch()[0]
                    msg = _diff(case, got, want, T[name].word)
                    if msg:
                        bad.append(tag + ("call", k, name, msg))
                    if not case.f32:         # the two pad fills give identical words (where the call writes)
                        wrote = ~want[1] if isinstance(want, tuple) else np.ones(got.shape, bool)
                        first = seen.setdefault((mode, tuple(sorted(offs.items())), k, name), got)
                        if first is not got and (first[wrote] != got[wrote]).any():
                            bad.append(tag + ("call", k, name, "differs from the run with the other pad fill"))
            for op in case.ops:
                if not T[op.name].fetch()[1]:
                    bad.append(tag + (op.name, "pad written"))
    assert not bad, f"{len(bad)} failures, the first 12:\n" + "\n".join(str(b) for b in bad[:12])
    if case.compare == "mfcc_f32" and not mfcc_cfg.host_libm_status()[0]:
        pytest.skip("host libm differs: suite tolerance checked, bit-exactness not assessable on this host")


def _family_test(family):
    @pytest.mark.gpu
    @pytest.mark.parametrize("cid", _ids(family))
    def test(dsp, torch_gpu, cid):
        _run(CASES[cid], dsp, torch_gpu)
    test.__name__ = test.__qualname__ = f"test_{family}_offset_pointers"
    test.__doc__ = f"Every case of the {family} rows: see the module docstring and the case table above."
    return test


test_cfft_offset_pointers = _family_test("cfft")
test_rfft_fast_offset_pointers = _family_test("rfft_fast")
test_rfft_fixed_offset_pointers = _family_test("rfft_fixed")
test_fir_offset_pointers = _family_test("fir")
test_multirate_offset_pointers = _family_test("multirate")
test_sparse_offset_pointers = _family_test("sparse")
test_lattice_offset_pointers = _family_test("lattice")
test_conv_offset_pointers = _family_test("conv")
test_gemm_offset_pointers = _family_test("gemm")
test_mfcc_offset_pointers = _family_test("mfcc")


# ------------------------------------------------------------------ drop-ins on device pointers at offset 1
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "q15"])
def test_cfft_dropin_device_pointer_offset(dsp, torch_gpu, kind):
    """arm_cfft_f32 / arm_cfft_q15 on a device pointer at element offset 1, N = 1024, one transform
    (f32: the 2-wave latency kernel), forward and inverse."""
    torch = torch_gpu
    n = 1024
    x = refs.rand_input(kind, 2 * n, seed=31)
    bad = []
    for fill in ((NAN_FILL,) if kind == "f32" else (FILL_A, FILL_B)):
        for ifft in (0, 1):
            want = refs.ref_lib().cfft(kind, n, x, ifft, 1)
            for o in (0, 1):
                d = Padded(torch, DT[kind], (2 * n,), o, fill).put(torch, x)
                S = getattr(dsp, f"arm_cfft_instance_{kind}")()
                assert getattr(dsp, f"arm_cfft_init_{kind}")(S, n) == 0
                getattr(dsp.lib, f"arm_cfft_{kind}")(C.byref(S), C.c_void_p(d.ptr), ifft, 1)
                dsp._check_void("arm_cfft")
                torch.cuda.synchronize()
                got, pads_ok = d.fetch()
                if got.tobytes() != want.tobytes():
                    bad.append((fill, ifft, o, int((got != want).sum()), "words differ"))
                if not pads_ok:
                    bad.append((fill, ifft, o, "pad written"))
    assert not bad, "\n".join(str(b) for b in bad)


@pytest.mark.gpu
def test_mat_mult_q15_dropin_device_pointers_offset(dsp, torch_gpu):
    """arm_mat_mult_q15 with all three pData on the device at element offset 1 (pState on the host),
    a whole-tile and a ragged shape."""
    torch = torch_gpu
    bad = []
    for m, k, n in ((128, 64, 128), (65, 130, 67)):
        rng = np.random.default_rng(m + k)
        a, b = _rand("q15", (m, k), rng), _rand("q15", (k, n), rng)
        st, want = refs.ref_lib().mat_mult_fixed("q15", a, b)
        assert st == 0
        for fill in (FILL_A, FILL_B):
            for o in (0, 1):
                da = Padded(torch, np.int16, (m, k), o, fill).put(torch, a)
                db = Padded(torch, np.int16, (k, n), o, fill).put(torch, b)
                dc = Padded(torch, np.int16, (m, n), o, fill)
                inst = dsp.arm_matrix_instance_q15
                A, B, Cm = (inst(r, c, C.cast(p.ptr, _abi.c_i16p)) for r, c, p in ((m, k, da), (k, n, db), (m, n, dc)))
                state = np.zeros(k * n + 16, np.int16)
                assert dsp.lib.arm_mat_mult_q15(C.byref(A), C.byref(B), C.byref(Cm), _ptr(state)) == 0
                torch.cuda.synchronize()
                got, pads_ok = dc.fetch()
                if got.tobytes() != want.tobytes():
                    bad.append((m, k, n, fill, o, int((got != want).sum()), "words differ"))
                if not (pads_ok and da.fetch()[1] and db.fetch()[1]):
                    bad.append((m, k, n, fill, o, "pad written"))
    assert not bad, "\n".join(str(b) for b in bad)


# ------------------------------------------------------------------ the case table, on the CPU
_FAMILIES = sorted({c.family for c in CASES.values()})


@pytest.mark.parametrize("family", _FAMILIES)
def test_case_table_reference_ignores_pads(family):
    """Builds every case's inputs and reference outputs, and runs the reference again on operand
    views into two differently filled guarded buffers (CPU-backed, element offset 1): its words do
    not depend on the pads, it leaves the pads alone, and every row of the table has what the GPU
    runner needs (each operand named by inputs() or an output, every expected word set matching
    its operand's shape)."""
    import torch
    for cid in _ids(family):
        case = CASES[cid]
        x, calls, final = _built(cid)
        names = {op.name: op for op in case.ops}
        assert len(calls) == case.ncalls
        for d in calls + [final]:
            for name, w in d.items():
                w = w[0] if isinstance(w, tuple) else w
                assert w.shape == names[name].shape and w.dtype == names[name].dt, (cid, name, w.shape, w.dtype)
        for op in case.ops:
            assert (op.name in x) == (op.role in ("in", "io")), (cid, op.name)
            assert op.role != "out" or any(op.name in d for d in calls) or op.name == "work", (cid, op.name)
        modes = list(_modes(case))
        assert modes[0] == ("aligned", {}) and len(modes) == 1 + sum(len(op.offsets) for op in case.ops) + max(
            len(op.offsets) for op in case.ops)
        for i in range(2):
            held, views = [], {}
            for name, v in x.items():
                arrs = v if isinstance(v, list) else [v]
                fill = (NAN_FILL, F32_SENTINEL)[i] if names[name].dt == np.float32 else (FILL_A, FILL_B)[i]
                ps = [Padded(torch, names[name].dt, a.shape, 1, fill, device="cpu").put(torch, a) for a in arrs]
                held += ps
                vs = [p.t.numpy() for p in ps]
                views[name] = vs if isinstance(v, list) else vs[0]
            calls2, final2 = case.expect(views)
            for d, d2 in zip(calls + [final], calls2 + [final2]):
                for name, w in d.items():
                    w, w2 = (w[0], d2[name][0]) if isinstance(w, tuple) else (w, d2[name])
                    assert w.tobytes() == w2.tobytes(), (cid, i, name)
            # a forward transform overwrites its input in the reference too; the pads stay
            assert all(p.fetch()[1] for p in held), (cid, i)


# ------------------------------------------------------------------ the runner's negative controls, on the CPU
class Toy(Case):
    """dst = src + 1 on the CPU, with one planted defect: the runner must report each."""

    def __init__(self, kind, defect):
        self.kind, self.defect = kind, defect
        self.f32 = kind == "f32"
        super().__init__("toy", f"{kind}-{defect}", [Op("src", DT[kind], (3, 10), "in"), Op("dst", DT[kind], (3, 10), "out")])

    def inputs(self):
        return {"src": _rand(self.kind, (3, 10), np.random.default_rng(1)) // (1 if self.f32 else 2)}

    def expect(self, x):
        return [{"dst": (np.asarray(x["src"]) + np.asarray(1, DT[self.kind])).astype(DT[self.kind])}], {}

    def launch(self, dsp, torch, T, call):
        src, dst = T["src"], T["dst"]
        dst.t.copy_(src.t + 1)
        if self.defect == "store_after":
            dst.flat[dst.hi] = 7
        elif self.defect == "store_before" and dst.o == 2:    # only in some of the offset modes
            dst.flat[dst.lo - 1] = 7
        elif self.defect == "read_before":
            dst.t[0, 0] = src.flat[src.lo - 1] + 1
        elif self.defect == "read_after_weak":                # an outside word used, but barely
            dst.t[2, 9] += src.flat[src.hi] * 0


for _k in ("f32", "q15", "q7"):
    for _d in ("none", "store_after", "store_before", "read_before", "read_after_weak"):
        _TOYS[f"toy-{_k}-{_d}"] = Toy(_k, _d)


@pytest.mark.parametrize("kind", ["f32", "q15", "q7"])
def test_runner_reports_planted_defects(kind):
    """_run on CPU-backed operands: a clean toy kernel passes; a store one element after or (at one
    offset only) before dst is a written pad; a read of the element before src is a wrong word under
    both fills; an outside word multiplied by zero still poisons an f32 output through the NaN pad
    (an integer kernel that really ignores the word passes, as it should)."""
    import torch
    _run(_TOYS[f"toy-{kind}-none"], None, torch, device="cpu")
    for defect, what in (("store_after", "pad written"), ("store_before", "pad written"), ("read_before", "differ")):
        with pytest.raises(AssertionError, match=what) as e:
            _run(_TOYS[f"toy-{kind}-{defect}"], None, torch, device="cpu")
        if defect == "store_before":      # reported with the mode and offset it happened at, and only there
            assert "('dst', 2)" in str(e.value) and "'aligned'" not in str(e.value)
    if kind == "f32":
        with pytest.raises(AssertionError, match="differ"):
            _run(_TOYS["toy-f32-read_after_weak"], None, torch, device="cpu")
    else:
        _run(_TOYS[f"toy-{kind}-read_after_weak"], None, torch, device="cpu")
