"""The batched entry points at batch counts past 65,535.

The `_batch` entry points are meant for 2^16 .. 2^20 items per call; the other GPU tests pass a few
hundred at the most.  Here every row runs at B = 66,047 items: odd, 511 past 2^16 (at least one
whole 256-lane workgroup of a lane-per-item kernel lies beyond the 16-bit edge), no multiple of any
power-of-two items-per-workgroup, and past the 65,535 limit of grid y / z.

* A row has P = 251 distinct items (the family's own generators); item i of the batch is pattern
  i % 251.  65,536 mod 251 = 25 (and 2^k mod 251 != 0 for every k: 251 is an odd prime), so an item
  index wrapped at 2^16 or at any power of two above it lands on another pattern, and the patterns
  differ pairwise in an output word: the wrap shows.  A dropped item keeps its marker.
* The reference (the oracle the family's tests use: refs.ref_lib(); f32 GEMM: oracle.mat_mult_fmaf;
  MFCC f32: mfcc_cfg's parity rule; the numpy restatements of the later families) runs on the 251
  patterns only; its words are tiled to B (`tiled`) on the device the operands live on.
* Byte equality over all B items (f32: assert_same_words on every item whose bits differ), outputs
  pre-filled with the marker, every operand between guard words (tests/padded.py at offset 0).
  Streaming filters run two calls with the state carried; the state rows are compared too.
* Every row also runs at B = 0: success, no recorded error, every output, state and guard word still
  the marker.  Rows whose launch picks a kernel by the batch run once more below that threshold.
* A failure names the first failing items as (index, index % 65536, index % 251).

The distance and DTW rows use distance_ref.py, the log-domain statistics, SVMs, naive Bayes and vexp / vlog rows
ml_ref.py.  The rows whose reference words are the host libm's expf / logf (Case.libm) are skipped on a host whose
libm is not the one the kernels restate, as in test_ml.py.  dtw_init_window takes no per-item input, so every item of
its rows gets the same window (Case.uniform): a dropped item still keeps its marker, a wrapped index cannot show.

The row classes are those of test_gpu_pointer_offsets.py where that file has the family.  Beside the
table: the K > 32,704 fall-back GEMM kernels at 3 items (at B their operands would pass 4 GB) and the one
inherent limit, 2^31 - 1 workgroups, as a tested refusal.  Two tests are not marked gpu:
test_case_table_builds_on_cpu and test_runner_reports_planted_defects.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_ref
import basic_math_ref
import biquad_ref
import cmplx_mat_ref
import cmplx_math_ref
import distance_ref
import mat_basic_ref
import mat_solve_ref
import ml_ref
import refs
import statistics_ref
import support_ref
import test_gpu_pointer_offsets as po
from cmsisdsp_amd import _abi
from padded import F32_SENTINEL, FILL_A, Padded

B = 66047
P = 251
EDGE = 65536
GIB = 1 << 30
DT = refs.DTYPE
_CHUNK_BYTES = 32 << 20                     # device temporaries of the tiling and the comparison


def tiled(words, n):
    """The words of an n-item batch whose item i is pattern i % P."""
    return words[np.arange(n) % P]


def _per_item(op):
    return len(op.shape) >= 2 and op.shape[0] == P


class Row:
    """case: a row object of the pointer-offset table's kind, built with P items.  batches: the
    counts it runs at.  note: which kernel B reaches."""

    def __init__(self, case, note, batches=(B, 0)):
        self.case, self.note = case, note
        self.family = case.family
        self.id = case.id
        # a row that would take more than 1 GiB at B runs at the smallest batch above 65,535 instead
        big = B if B * self.item_bytes() <= GIB else EDGE
        self.batches = tuple(big if n == B else n for n in batches)

    def item_bytes(self):
        return sum(int(np.prod(op.shape[1:])) * op.dt.itemsize for op in self.case.ops if _per_item(op))

    def expect(self, n):
        """(per call: name -> words [n, ...] | (words, untouched mask), after the last call: name -> words)"""
        _, calls, final = _built(self.id)
        t = lambda w: tuple(tiled(v, n) for v in w) if isinstance(w, tuple) else tiled(w, n)
        return [{k: t(w) for k, w in d.items()} for d in calls], {k: t(w) for k, w in final.items()}


ROWS = {}
_TOYS = {}


def _add(case, note, batches=(B, 0)):
    assert case.id not in ROWS, case.id
    ROWS[case.id] = Row(case, note, batches)


# ------------------------------------------------------------------ CFFT
# f32 N <= 256, fixed-point N <= 128: the generic kernels (several transforms per workgroup, B leaves a
# ragged last one); fixed-point N = 256: the radix-16 kernel; f32 512 / 1024 / 2048: the wave-per-
# transform specialists (N = 1024: a grid that is no multiple of kN1024Split, the identity block order;
# N = 2048: 16 KiB per transform, 65,536 of them are the 1 GiB)
for _k in ("f32", "q31", "q15"):
    for _n in (16, 256) + ((512, 1024, 2048) if _k == "f32" else ()):
        for _ifft in (0, 1):
            _what = ("generic kernel" if _n == 16 or _k == "f32" and _n == 256 else
                     "radix-16 kernel" if _k != "f32" else f"N = {_n} specialist")
            _add(po.Cfft(_k, _n, _ifft, 1, P), _what)

# ------------------------------------------------------------------ RFFT
for _n in (32, 1024):
    for _ifft in (0, 1):
        for _s in (False, True):
            _add(po.RfftFast(_n, _ifft, _s, batch=P), "inner CFFT N / 2 and the split kernel")
for _k in ("q31", "q15"):
    for _n in (32, 512):
        for _ifft in (0, 1):
            _add(po.RfftFixed(_k, _n, _ifft, batch=P), "inner CFFT N / 2 (512: radix-16) and the split")

# ------------------------------------------------------------------ FIR
# The MFMA kernels take a call of >= 256 (item, chunk) pairs; q15 / fast_q15 / q7 also need blockSize >= 64,
# so at blocks 8 and 32 those kinds run their VALU kernels at every batch and (30, 64) is their MFMA row.
# q31 at B is on the MFMA kernel and at 255 items on the VALU kernel.  f32 and fast_q31 have no MFMA kernel.
# The MFMA kernels have no run-time opt-out (MI355X_FIR_*_MFMA are compile-time switches).
for _k in ("f32", "q15", "q31", "fast_q15", "fast_q31", "q7"):
    _even = lambda t: t + (t & 1 if _k.endswith("q15") else 0)
    for _t, _b in ((4, 8), (29, 32)):
        _add(po.Fir(_k, _even(_t), _b, batch=P), "MFMA kernel; 255: VALU kernel" if _k == "q31" else "VALU kernel",
             (B, 0, 255) if _k == "q31" else (B, 0))
    if _k in ("q15", "fast_q15", "q7"):
        _add(po.Fir(_k, 30, 64, batch=P), "MFMA kernel; 255: VALU kernel", (B, 0, 255))

# one decimator and one interpolator per type at the smallest legal shape: M / L = 2 is the FIR pass,
# 5 the multirate functions' own kernel
for _fn in ("decimate_f32", "decimate_q15", "decimate_fast_q15", "decimate_q31", "decimate_fast_q31"):
    for _m in (2, 5):
        _add(po.Multirate(_fn, 2 * _m, _m, 2 * _m, batch=P), "FIR pass" if _m == 2 else "decimator kernel")
for _fn in ("interpolate_f32", "interpolate_q15", "interpolate_q31"):
    for _l in (2, 5):
        _add(po.Multirate(_fn, 2 * _l, _l, 3, batch=P), "FIR pass" if _l == 2 else "interpolator kernel")
for _k in ("f32", "q31", "q15", "q7"):
    _add(po.Sparse(_k, 4, 20, 8, batch=P), "LDS-staged kernel")
for _k in ("f32", "q31", "q15"):
    _add(po.Lattice(_k, 3, 8, P), "lane-per-item kernel")


# ------------------------------------------------------------------ conv / correlate / conv_partial
class Conv(po.Conv):
    """The batched names of the conv family (the _opt names are drop-ins only).  conv_partial: a range
    that starts inside the head and ends among the tail outputs of these short operands."""
    batch = P

    def __init__(self, fn, la, lb):
        super().__init__(fn, la, lb)
        if self.partial:
            self.first, self.num = 2, la + lb - 1 - 4
            self.width = self.num
            self.ops[2] = po.Op("out", self.ops[2].dt, (P, self.width), "out")


for _fn in list(po._abi.CONV_FULL) + list(po._abi.CONV_PARTIAL):
    for _la, _lb in ((7, 5), (5, 7)):
        _add(Conv(_fn, _la, _lb), "conv_kernel, one chunk per item")


# ------------------------------------------------------------------ GEMMs
class Gemm(po.Gemm):
    batch = P


class CmplxGemm(po.Case):
    """arm_mat_cmplx_mult_{f32,q31,q15}_batch, complex m x k x n; the oracles of test_cmplx_mat.py."""

    def __init__(self, kind, m, k, n):
        self.kind, self.m, self.k, self.n, self.batch = kind, m, k, n, P
        self.f32 = kind == "f32"
        dt = DT[kind]
        super().__init__("cmplx_gemm", f"{kind}-{m}-{k}-{n}",
                         [po.Op("a", dt, (P, m, 2 * k), "in"), po.Op("b", dt, (P, k, 2 * n), "in"),
                          po.Op("c", dt, (P, m, 2 * n), "out")])

    def inputs(self):
        rng = np.random.default_rng([self.m, self.k, self.n, 11])
        a, b = cmplx_mat_ref.operands(self.kind, "uniform" if self.f32 else "full", self.m, self.k, self.n, rng, P)
        return {"a": a, "b": b}

    def expect(self, x):
        if not self.f32:
            return [{"c": cmplx_mat_ref.mult_fixed(self.kind, x["a"], x["b"])}], {}
        o = refs.oracle_lib()
        return [{"c": np.stack([o.mat_mult_fmaf(x["a"][i], cmplx_mat_ref.embed(x["b"][i]))[1] for i in range(P)])}], {}

    def launch(self, dsp, torch, T, call):
        dsp.mat_cmplx_mult_batch(T["a"].t, T["b"].t, T["c"].t)


# ragged 3 x 5 x 2: the guarded kernels, one workgroup per item
for _k in ("f32", "q7", "q15", "q31", "fast_q15", "fast_q31"):
    _add(Gemm(_k, 3, 5, 2), {"f32": "mat_mult_f32_kernel (guarded)", "fast_q31": "mat_mult_fast_q31_kernel",
                             "q7": "mat_mult_q7_kernel"}.get(_k, "matrix-core kernel, guarded"))
_add(Gemm("fast_q31", 64, 16, 64), "mat_mult_fast_q31_kernel, one whole tile")
# one whole tile per item: 24 KiB (fast_q31), 80 KiB (f32) and 64 KiB (q15) per item, 1.5, 5.0 and 4.0 GiB
# at 65,536 items.  No batch above 65,535 fits 1 GiB, so these three rows run at the smallest batch above
# 65,535 and are the exception to the 1-GiB budget (_BIG)
_add(Gemm("f32", 128, 16, 128), "mat_mult_f32_full_kernel (batch folded into grid x)")
_add(Gemm("q15", 128, 64, 128), "mat_mult_i8v2_kernel, whole tile")
for _k in ("f32", "q31", "q15"):
    _add(CmplxGemm(_k, 2, 3, 2), "mat_mult_f32_kernel<CX>" if _k == "f32" else "matrix-core kernel <CX>, guarded")
_BIG = {"gemm-f32-128-16-128", "gemm-q15-128-64-128", "gemm-fast_q31-64-16-64"}

# ------------------------------------------------------------------ MFCC
class Mfcc(po.Mfcc):
    """The generator's fixed-point frames 2 and 5 (words of magnitude <= 3 and <= 1) give the all-zero
    frame's output words; here they are full-scale frames shifted down by 3 and 6 bits, so that the
    patterns stay pairwise distinct."""

    def inputs(self):
        x = super().inputs()
        if not self.f32:
            f = x["frames"][0]
            f[2], f[5] = f[7] >> 3, f[8] >> 6
        return x


for _k in ("f32", "q31", "q15"):
    for _w in (False, True):
        _add(Mfcc(_k, 256, _w, batch=P), "front end + RFFT 256 + tail, a frame per wave / workgroup")
    _add(Mfcc(_k, 1024, False, batch=P), "fftLen 1024: the front end and tail around the RFFT 1024 kernels")


# ------------------------------------------------------------------ recursive and adaptive filters
def _stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _words32(a):
    """int64 words as the int32 pairs they are in memory (the guarded buffers hold 1-, 2- and 4-byte words)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32).reshape(a.shape[0], -1) if a.dtype == np.int64 else a


class Biquad(po.Case):
    """The eight cascade forms; the oracle of test_biquad.py (biquad_ref.run), two calls, the state carried."""
    ncalls = 2

    def __init__(self, func, stages, block):
        self.func, self.stages, self.block, self.batch = func, stages, block, P
        dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
        self.f32 = dt == np.float32
        self.ps = stages % 4 if func in biquad_ref.HAS_SHIFT else 0
        sw = ks * stages * (2 if sdt == np.int64 else 1)
        super().__init__("biquad", f"{func[4:]}-{stages}-{block}",
                         [po.Op("src", dt, (P, ch * block), "in"), po.Op("dst", dt, (P, ch * block), "out"),
                          po.Op("state", np.int32 if sdt == np.int64 else sdt, (P, sw), "state")])

    def inputs(self):
        dt, _, _, _, ch = biquad_ref.FUNCS[self.func]
        rng = np.random.default_rng(31 * self.stages + self.block)
        shape = (P, ch * self.block)
        if self.f32:
            return {"src": [rng.uniform(-1, 1, shape).astype(np.float32) for _ in range(2)]}
        i = np.iinfo(dt)
        return {"src": [rng.integers(i.min // 2, i.max // 2, shape, endpoint=True).astype(dt) for _ in range(2)]}

    def _coeffs(self):
        return biquad_ref.stable_coeffs(self.func, self.stages, self.ps, 1000 + self.stages)

    def expect(self, x):
        _, sdt, ks, _, _ = biquad_ref.FUNCS[self.func]
        st, calls = np.zeros((P, ks * self.stages), dtype=sdt), []
        for k in range(2):
            y, st = biquad_ref.run(self.func, self._coeffs(), self.ps, x["src"][k], st)
            calls.append({"dst": y, "state": _words32(st)})
        return calls, {}

    def launch(self, dsp, torch, T, call):
        c = self._coeffs()
        inst = _abi.BIQUAD_FUNCS[self.func][0]
        kw = {"postShift": self.ps} if any(f == "postShift" for f, _ in inst._fields_) else {}
        S = inst(numStages=self.stages, pState=None, pCoeffs=c.ctypes.data, **kw)
        st = getattr(dsp.lib, self.func + "_batch")(C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block,
                                                    self.batch, C.c_void_p(T["state"].ptr), _stream_of(torch))
        assert st == 0, dsp.last_error()


for _f in biquad_ref.FUNCS:
    for _s in (1, 5):
        _add(Biquad(_f, _s, 8), "biquad_kernel, lane = (stream, stage)")


class IirLattice(po.Case):
    """arm_iir_lattice_*; the oracle of test_adaptive.py (adaptive_ref), a distinct start state per item."""
    ncalls = 2

    def __init__(self, func, stages, block):
        self.func, self.stages, self.block, self.batch = func, stages, block, P
        dt = adaptive_ref.FUNCS[func][0]
        self.f32 = dt == np.float32
        super().__init__("iir_lattice", f"{func[4:]}-{stages}-{block}",
                         [po.Op("src", dt, (P, block), "in"), po.Op("dst", dt, (P, block), "out"),
                          po.Op("state", dt, (P, stages), "io")])

    def inputs(self):
        return {"src": [adaptive_ref.signal(self.func, (P, self.block), 7 * self.stages + self.block + i) for i in range(2)],
                "state": adaptive_ref.signal(self.func, (P, self.stages), 3 * self.stages + P, 0.25)}

    def expect(self, x):
        k, v = adaptive_ref.lattice_coeffs(self.func, self.stages, 1000 + self.stages)
        st, calls = x["state"], []
        for i in range(2):
            y, st = adaptive_ref.iir_lattice(self.func, k, v, x["src"][i], st)
            calls.append({"dst": y, "state": st})
        return calls, {}

    def launch(self, dsp, torch, T, call):
        k, v = (a.copy() for a in adaptive_ref.lattice_coeffs(self.func, self.stages, 1000 + self.stages))
        S = _abi.ADAPTIVE_FUNCS[self.func][0](numStages=self.stages, pState=None, pkCoeffs=k.ctypes.data,
                                              pvCoeffs=v.ctypes.data)
        st = getattr(dsp.lib, self.func + "_batch")(C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block,
                                                    self.batch, C.c_void_p(T["state"].ptr), _stream_of(torch))
        assert st == 0, dsp.last_error()


class Lms(po.Case):
    """arm_lms_* / arm_lms_norm_*; the oracle of test_adaptive.py: coefficients, history and energy / x0 per item."""
    ncalls = 2

    def __init__(self, func, taps, block):
        self.func, self.taps, self.block, self.batch = func, taps, block, P
        dt, self.fam = adaptive_ref.FUNCS[func]
        self.f32 = dt == np.float32
        self.mu, self.ps = adaptive_ref.default_mu(func), (taps % 4 if dt != np.float32 else 0)
        ops = [po.Op("src", dt, (P, block), "in"), po.Op("ref", dt, (P, block), "in"), po.Op("out", dt, (P, block), "out"),
               po.Op("err", dt, (P, block), "out"), po.Op("coeffs", dt, (P, taps), "io"),
               po.Op("state", dt, (P, taps - 1), "io")]
        if self.fam == "nlms":
            ops.append(po.Op("ex", dt, (P, 2), "io"))
        super().__init__("lms", f"{func[4:]}-{taps}-{block}", ops)

    def inputs(self):
        dt, taps = adaptive_ref.FUNCS[self.func][0], self.taps
        rng = np.random.default_rng(50 * taps + P)
        x = {"coeffs": adaptive_ref.quantise(rng.uniform(-0.3, 0.3, (P, taps)) / 2.0 ** self.ps, dt),
             "state": adaptive_ref.signal(self.func, (P, taps - 1), taps + P + 1, 0.3)}
        if self.fam == "nlms":
            x["ex"] = np.stack([adaptive_ref.quantise(rng.uniform(0.2, 0.6, P), dt),
                                adaptive_ref.quantise(rng.uniform(-0.2, 0.2, P), dt)], 1)
        x["src"] = [adaptive_ref.signal(self.func, (P, self.block), 9 * taps + self.block + i, 0.3) for i in range(2)]
        x["ref"] = [adaptive_ref.signal(self.func, (P, self.block), 11 * taps + self.block + i, 0.3) for i in range(2)]
        return x

    def expect(self, x):
        c, st, ex, calls = x["coeffs"], x["state"], x.get("ex"), []
        for i in range(2):
            y, e, c, st, ex = adaptive_ref.lms(self.func, self.mu, self.ps, x["src"][i], x["ref"][i], c, st, ex)
            calls.append(dict({"out": y, "err": e, "coeffs": c, "state": st}, **({"ex": ex} if self.fam == "nlms" else {})))
        return calls, {}

    def launch(self, dsp, torch, T, call):
        inst = _abi.ADAPTIVE_FUNCS[self.func][0]
        kw = {"postShift": self.ps} if any(n == "postShift" for n, _ in inst._fields_) else {}
        S = inst(numTaps=self.taps, pState=None, pCoeffs=None, mu=self.mu, **kw)
        ptr = lambda name: C.c_void_p(T[name].ptr)   # noqa: E731
        args = [C.byref(S), ptr("src"), ptr("ref"), ptr("out"), ptr("err"), self.block, self.batch, ptr("coeffs"), ptr("state")]
        st = getattr(dsp.lib, self.func + "_batch")(*args, *([ptr("ex")] if self.fam == "nlms" else []), _stream_of(torch))
        assert st == 0, dsp.last_error()


for _f, (_dt, _fam) in adaptive_ref.FUNCS.items():
    for _s in (3, 5):
        _add(IirLattice(_f, _s, 8) if _fam == "iir" else Lms(_f, _s, 8), "guarded register instance, 64 streams per wave")


# ------------------------------------------------------------------ matrix solves
class Solve(po.Case):
    """inverse / cholesky / ldlt / the triangular solves (f32); the oracle of test_mat_solve.py (mat_solve_ref).
    Pattern 7 fails (a structural zero) and its status word and partial outputs are compared; pattern 9 of
    ldlt is rank deficient.  The words a call leaves alone (cholesky's strict upper triangle, a failed item's
    unreached words) must keep the marker: they are the words in which two reference runs on differently
    pre-filled outputs differ."""
    f32 = True
    FAIL = 7

    def __init__(self, func, n, cols=2):
        self.func, self.n, self.cols, self.batch = func, n, cols, P
        f, i = np.float32, np.int32
        ops = {"inverse": [("src", f, (n, n), "io"), ("dst", f, (n, n), "out"), ("status", i, (1,), "out")],
               "cholesky": [("src", f, (n, n), "in"), ("dst", f, (n, n), "out"), ("status", i, (1,), "out")],
               "ldlt": [("src", f, (n, n), "in"), ("l", f, (n, n), "out"), ("d", f, (n, n), "out"), ("pp", np.int16, (n,), "out")],
               }.get(func, [("t", f, (n, n), "in"), ("a", f, (n, cols), "in"), ("dst", f, (n, cols), "out"),
                            ("status", i, (1,), "out")])
        super().__init__("mat_solve", f"{func}-{n}", [po.Op(name, dt, (P,) + shape, role) for name, dt, shape, role in ops])

    def inputs(self):
        rng = np.random.default_rng(100 * self.n + len(self.func))
        solve = self.func.startswith("solve")
        kinds = ("lower",) if self.func == "solve_lower" else ("upper",) if solve else mat_solve_ref.FILLS[self.func]
        if self.func == "ldlt":             # tiny_spd is rank 0 to arm_mat_ldlt_f32 (|a| < 1e-8), as the zero matrix
            kinds = ("spd",)
        m = np.stack([mat_solve_ref.fill(kinds[i % len(kinds)], self.n, rng) for i in range(P)])
        m[self.FAIL] = mat_solve_ref.failing(self.func, mat_solve_ref.FAILS[self.func][0], self.n, rng)
        if self.func == "ldlt":
            m[9] = mat_solve_ref.failing("ldlt", "rank", self.n, rng)
        if solve:
            return {"t": m, "a": np.stack([mat_solve_ref.rhs(self.n, self.cols, rng) for _ in range(P)])}
        return {"src": m}

    def _ref(self, x, fill):
        """name -> words [P, ...] with the outputs pre-filled with `fill`."""
        pre = lambda shape: np.full(shape, fill, np.float32)   # noqa: E731
        out = {}
        for i in range(P):
            if self.func == "inverse":
                st, s, d = mat_solve_ref.inverse(x["src"][i])
                r = {"src": s, "dst": d, "status": np.array([st], np.int32)}
            elif self.func == "cholesky":
                st, d = mat_solve_ref.cholesky(x["src"][i], pre((self.n, self.n)))
                r = {"dst": d, "status": np.array([st], np.int32)}
            elif self.func == "ldlt":
                st, l, d, pp = mat_solve_ref.ldlt(x["src"][i])
                r = {"l": l, "d": d, "pp": pp.view(np.int16)}
            else:
                st, d = mat_solve_ref.solve(x["t"][i], x["a"][i], self.func == "solve_lower", pre((self.n, self.cols)))
                r = {"dst": d, "status": np.array([st], np.int32)}
            for k, v in r.items():
                out.setdefault(k, []).append(v)
        return {k: np.stack(v) for k, v in out.items()}

    def expect(self, x):
        r1, r2 = self._ref(x, 1.0), self._ref(x, 2.0)
        if self.func != "ldlt":
            assert r1["status"][self.FAIL, 0] != 0 and (r1["status"][:, 0] == 0).sum() > P // 2
        return [{k: (w, w.view(np.uint8) .reshape(w.shape + (-1,)).__ne__(
            r2[k].view(np.uint8).reshape(w.shape + (-1,))).any(axis=-1)) for k, w in r1.items()}], {}

    def launch(self, dsp, torch, T, call):
        if self.func == "inverse":
            dsp.mat_inverse_batch(T["src"].t, T["dst"].t, status=T["status"].t)
        elif self.func == "cholesky":
            dsp.mat_cholesky_batch(T["src"].t, T["dst"].t, status=T["status"].t)
        elif self.func == "ldlt":
            dsp.mat_ldlt_batch(T["src"].t, T["l"].t, T["d"].t, T["pp"].t)
        else:
            dsp.mat_solve_triangular_batch(T["t"].t, T["a"].t, T["dst"].t, self.func == "solve_lower", status=T["status"].t)


# inverse / cholesky / ldlt pack ipw = 256 / L items into a workgroup (L: the lanes of one item, a power of two);
# ipw - 1 items leave the one workgroup partly filled
for _f in ("inverse", "cholesky", "ldlt"):
    for _n in (3, 4):
        _ipw = 256 // (8 if _f == "inverse" else 4)
        _add(Solve(_f, _n), f"items in LDS, {_ipw} per workgroup; {_ipw - 1}: one partly filled workgroup", (B, 0, _ipw - 1))
for _f in ("solve_lower", "solve_upper"):
    _add(Solve(_f, 3), "lane per (item, column), x in LDS")


# ------------------------------------------------------------------ transposes, matrix x vector
class Trans(po.Case):
    def __init__(self, kind, rows, cols, cmplx):
        self.kind, self.rows, self.cols, self.cmplx, self.batch = kind, rows, cols, cmplx, P
        self.f32 = kind == "f32"
        w = 2 if cmplx else 1
        super().__init__("mat_trans", f"{'cmplx_' if cmplx else ''}trans-{kind}-{rows}-{cols}",
                         [po.Op("src", DT[kind], (P, rows, w * cols), "in"), po.Op("dst", DT[kind], (P, cols, w * rows), "out")])

    def inputs(self):
        rng = np.random.default_rng(self.rows + 3 * self.cols)
        return {"src": mat_basic_ref.rand(self.kind, self.ops[0].shape, rng)}

    def expect(self, x):
        f = mat_basic_ref.cmplx_trans if self.cmplx else mat_basic_ref.trans
        return [{"dst": np.stack([f(m) for m in x["src"]])}], {}

    def launch(self, dsp, torch, T, call):
        (dsp.mat_cmplx_trans_batch if self.cmplx else dsp.mat_trans_batch)(T["src"].t, T["dst"].t)


class VecMult(po.Case):
    def __init__(self, kind, rows, cols):
        self.kind, self.rows, self.cols, self.batch = kind, rows, cols, P
        self.f32 = kind == "f32"
        dt = DT[kind]
        super().__init__("mat_vec", f"vec_mult-{kind}-{rows}-{cols}",
                         [po.Op("mat", dt, (P, rows, cols), "in"), po.Op("vec", dt, (P, cols), "in"),
                          po.Op("dst", dt, (P, rows), "out")])

    def inputs(self):
        rng = np.random.default_rng(self.rows + 5 * self.cols)
        return {"mat": mat_basic_ref.rand(self.kind, (P, self.rows, self.cols), rng),
                "vec": mat_basic_ref.rand(self.kind, (P, self.cols), rng)}

    def expect(self, x):
        return [{"dst": np.stack([mat_basic_ref.vec_mult(self.kind, x["mat"][i], x["vec"][i]) for i in range(P)])}], {}

    def launch(self, dsp, torch, T, call):
        dsp.mat_vec_mult_batch(T["mat"].t, T["vec"].t, T["dst"].t)


# 3 x 5: the pack kernel (items of <= 256 elements, 1024 / 15 = 68 to a workgroup); 3 x 86 = 258 elements: the
# smallest wide item of mat_trans_tile_kernel, whose grid y is clamped to 65,535 and strides over the rest
for _k in ("f32", "q31", "q15", "q7"):
    for _r, _c in ((3, 5), (3, 86)):
        _what = "mat_trans_pack_kernel" if _c == 5 else "mat_trans_tile_kernel, grid y 65,535 + a second trip"
        _add(Trans(_k, _r, _c, False), _what)
        if _k != "q7":
            _add(Trans(_k, _r, _c, True), _what)
    _add(VecMult(_k, 3, 5), "mat_vec_mult_kernel, one matrix per item")


# ------------------------------------------------------------------ reductions
_RES = {"f32": (np.float32, 1), "q63": (np.int32, 2), "q31": (np.int32, 1), "q15": (np.int16, 1), "q7": (np.int8, 1)}


def _res_words(v, rt):
    dt, w = _RES[rt]
    v = np.ascontiguousarray(v)
    return (v.view(np.int32) if rt == "q63" else v.astype(dt)).reshape(P, w)


class Reduce(po.Case):
    """One result word (or two, or a value and an index) per item.  what: ("stat", op) -- statistics_ref.run;
    ("search", op) -- arm_max / arm_min, cmplx_math_ref.extreme; ("dot", shared) -- arm_dot_prod, basic_math_ref.run;
    ("cdot", shared) -- arm_cmplx_dot_prod, cmplx_math_ref.dot_prod.  shared: one b for every item (bStride 0)."""

    def __init__(self, what, kind, n):
        self.what, self.kind, self.n, self.batch = what, kind, n, P
        self.f32 = kind == "f32"
        fam, arg = what
        dt = DT[kind]
        w = 2 * n if fam == "cdot" else n
        ops = [po.Op("a", dt, (P, w), "in")]
        if fam in ("dot", "cdot"):
            ops.append(po.Op("b", dt, (w,) if arg else (P, w), "in"))
            rt = (cmplx_math_ref.DOT_OUT if fam == "cdot" else basic_math_ref.DOT_OUT)[kind]
            self.outs = [("re", rt), ("im", rt)] if fam == "cdot" else [("result", rt)]
            name = f"{'cmplx_' if fam == 'cdot' else ''}dot_prod{'-shared' if arg else ''}"
        else:
            self.func = f"{arg}_{kind}"
            if fam == "stat" and arg == "mse":
                ops.append(po.Op("b", dt, (P, n), "in"))
            rt = statistics_ref.result_type(self.func) if fam == "stat" else kind
            self.outs = [("result", rt)] + ([("index", "q31")] if fam == "search" or arg in statistics_ref.SEARCH_IDX else [])
            name = arg
        ops += [po.Op(o, _RES[rt][0], (P, _RES[rt][1]), "out") for o, rt in self.outs]
        super().__init__("reduce", f"{name}-{kind}-{n}", ops)

    def inputs(self):
        fam, arg = self.what
        rng = np.random.default_rng([self.n, len(self.id)])
        shift = statistics_ref.amp_shift(self.func, self.n) if fam == "stat" and not self.f32 else 0
        x = {op.name: statistics_ref.rand(self.kind, op.shape, rng, shift) for op in self.ops if op.role == "in"}
        if fam in ("stat", "search") and not self.f32:      # a tie: the first index counts
            x["a"][3, -1] = x["a"][3, 0]
        return x

    def expect(self, x):
        fam, arg = self.what
        if fam == "dot":
            r = {"result": basic_math_ref.run(f"dot_prod_{self.kind}", x["a"], x["b"])["value"]}
        elif fam == "cdot":
            re, im = cmplx_math_ref.dot_prod(self.kind, x["a"], np.broadcast_to(x["b"], x["a"].shape))
            r = {"re": re, "im": im}
        elif fam == "search":
            v, i = cmplx_math_ref.extreme(arg, x["a"])
            r = {"result": v, "index": i.view(np.int32)}
        else:
            g = statistics_ref.run(self.func, x["a"], x.get("b"))
            r = {"result": g["value"]}
            if "index" in g:
                r["index"] = g["index"].view(np.int32)
        return [{o: _res_words(r[o], rt) for o, rt in self.outs}], {}

    def launch(self, dsp, torch, T, call):
        fam, arg = self.what
        if fam == "dot":
            dsp.dot_prod_batch(T["a"].t, T["b"].t, T["result"].t)
        elif fam == "cdot":
            dsp.cmplx_dot_prod_batch(T["a"].t, T["b"].t, T["re"].t, T["im"].t)
        elif fam == "stat" and arg == "mse":
            dsp.mse_batch(T["a"].t, T["b"].t, T["result"].t)
        else:
            getattr(dsp, f"{arg}_batch")(T["a"].t, *[T[o].t for o, _ in self.outs])


# n = 5 and n = 70 (a ragged 16-byte tail).  The f32 sums and dot products run one lane per item from 4,096 items
# on (kSumLaneMinBatch, kDotLaneMinBatch) and one wave per item below: B is the lane kernel, 4,095 the wave kernel.
# The integer kernels give an item 2^k lanes by its length, whatever the batch.
for _n in (5, 70):
    for _k in ("f32", "q31", "q15", "q7"):
        _bs = (B, 0, 4095) if _k == "f32" else (B, 0)
        _lane = "one lane per item; 4,095: one wave per item" if _k == "f32" else "sum_int_kernel / dot_int_kernel"
        for _shared in (False, True):
            _add(Reduce(("dot", _shared), _k, _n), _lane, _bs)
            if _k != "q7":
                _add(Reduce(("cdot", _shared), _k, _n), _lane, _bs)
        for _op in statistics_ref.SUM_OPS:
            if f"{_op}_{_k}" in statistics_ref.STAT_FUNCS:
                _add(Reduce(("stat", _op), _k, _n), _lane, _bs)
        for _op in statistics_ref.SEARCH_IDX + statistics_ref.SEARCH_NO_IDX:
            _add(Reduce(("stat", _op), _k, _n), "search kernel, lanes per item by length")
        for _op in ("max", "min"):
            _add(Reduce(("search", _op), _k, _n), "search kernel, lanes per item by length")


# ------------------------------------------------------------------ sort, barycenter, weighted average
class Support(po.Case):
    f32 = True

    def __init__(self, fn, shape, arg=None):
        self.fn, self.arg, self.batch = fn, arg, P
        f = np.float32
        ops = {"sort": [("src", shape, "in"), ("dst", shape, "out")],
               "barycenter": [("src", shape, "in"), ("w", shape[:1], "in"), ("out", shape[1:], "out")],
               "weighted_average": [("src", shape, "in"), ("w", shape, "in"), ("out", (1,), "out")]}[fn]
        super().__init__("support", f"{fn}-{'x'.join(map(str, shape))}" + (f"-dir{arg}" if arg is not None else ""),
                         [po.Op(name, f, (P,) + sh, role) for name, sh, role in ops])

    def inputs(self):
        rng = np.random.default_rng(len(self.id))
        x = {"src": rng.uniform(-1, 1, self.ops[0].shape).astype(np.float32)}
        if self.fn != "sort":
            x["w"] = rng.uniform(0.1, 1, self.ops[1].shape).astype(np.float32)
        else:
            x["src"][:, 1] = x["src"][:, 0]                 # a duplicate in every item
            x["src"][5, 2], x["src"][6, 2] = 0.0, -0.0
        return x

    def expect(self, x):
        if self.fn == "sort":
            return [{"dst": support_ref.total_order_sort(x["src"], bool(self.arg))}], {}
        if self.fn == "barycenter":
            return [{"out": support_ref.barycenter(x["src"], x["w"])}], {}
        return [{"out": support_ref.weighted_average(x["src"], x["w"]).reshape(P, 1)}], {}

    def launch(self, dsp, torch, T, call):
        if self.fn == "sort":
            dsp.sort_batch(T["src"].t, T["dst"].t, dir=self.arg)
        elif self.fn == "barycenter":
            dsp.barycenter_batch(T["src"].t, T["w"].t, T["out"].t)
        else:
            dsp.weighted_average_batch(T["src"].t, T["w"].t, T["out"].t)


for _n in (5, 70):
    for _dir in (1, 0):                                     # ARM_SORT_ASCENDING, ARM_SORT_DESCENDING
        _add(Support("sort", (_n,), _dir), "one wave per item")
_add(Support("barycenter", (3, 4)), "weights per item")
_add(Support("weighted_average", (5,)), "sum_f32_lane_kernel<kStWavg>, weights per item")


# ------------------------------------------------------------------ distances, DTW
_F = np.float32


class Distance(po.Case):
    """arm_<func>_distance_f32_batch; distance_ref.distance_f32 per item.  shared: one b for every item (bStride 0).
    jensenshannon's words are the host libm's logf's (libm: skipped where that is not the restated one)."""
    f32 = True

    def __init__(self, func, n, shared):
        self.func, self.n, self.shared, self.batch = func, n, shared, P
        self.libm = func == "jensenshannon"
        super().__init__("distance", f"{func}-{n}" + ("-shared" if shared else ""),
                         [po.Op("a", _F, (P, n), "in"), po.Op("b", _F, (n,) if shared else (P, n), "in"),
                          po.Op("result", _F, (P, 1), "out")])

    def inputs(self):
        rng = np.random.default_rng([self.n, len(self.func), int(self.shared), 41])

        def rand(shape):
            if self.func == "jensenshannon":            # normalised positive vectors, as distance_ref.f32_operands
                v = rng.uniform(0.01, 1.0, shape)
                return (v / v.sum(axis=-1, keepdims=True)).astype(_F)
            return rng.uniform(-1.0, 1.0, shape).astype(_F)
        return {"a": rand((P, self.n)), "b": rand(self.ops[1].shape)}

    def expect(self, x):
        b = np.broadcast_to(x["b"], x["a"].shape)
        r = [distance_ref.distance_f32(self.func, x["a"][i], b[i]) for i in range(P)]
        return [{"result": np.array([v[0] if isinstance(v, tuple) else v for v in r], _F).reshape(P, 1)}], {}

    def launch(self, dsp, torch, T, call):
        dsp.distance_batch(self.func, T["a"].t, T["b"].t, T["result"].t)


class BoolDistance(po.Case):
    """arm_<func>_distance_batch over `bits` booleans packed in 32-bit words; distance_ref.boolean_distance."""
    f32 = True

    def __init__(self, func, bits):
        self.func, self.bits, self.batch = func, bits, P
        w = distance_ref.bool_words(bits)
        super().__init__("bool_distance", f"{func}-{bits}",
                         [po.Op("a", np.int32, (P, w), "in"), po.Op("b", np.int32, (P, w), "in"),
                          po.Op("result", _F, (P, 1), "out")])

    def inputs(self):
        rng = np.random.default_rng([self.bits, 43])
        # the same operands for the nine functions; the bits past `bits` of the last word are random too
        return {k: rng.integers(0, 1 << 32, self.ops[0].shape, dtype=np.uint64).astype(np.uint32).view(np.int32) for k in "ab"}

    def expect(self, x):
        a, b = (np.ascontiguousarray(x[k]).view(np.uint32) for k in "ab")
        return [{"result": np.array([distance_ref.boolean_distance(self.func, a[i], b[i], self.bits) for i in range(P)],
                                    _F).reshape(P, 1)}], {}

    def launch(self, dsp, torch, T, call):
        dsp.boolean_distance_batch(self.func, T["a"].t, T["b"].t, self.bits, T["result"].t)


class DtwWindow(po.Case):
    """arm_dtw_init_window_q7_batch: the type and size are the call's, so every item gets the same window
    (uniform: the rule that the patterns differ cannot hold; a dropped item keeps its marker all the same)."""
    uniform = True

    def __init__(self, kind, size, q, t):
        self.kind, self.size, self.q, self.t, self.batch = kind, size, q, t, P
        super().__init__("dtw", f"init_window-{kind}-{size}-{q}x{t}", [po.Op("window", np.int8, (P, q, t), "out")])

    def inputs(self):
        return {}

    def expect(self, x):
        return [{"window": np.stack([distance_ref.init_window(self.kind, self.size, self.q, self.t)] * P)}], {}

    def launch(self, dsp, torch, T, call):
        dsp.dtw_init_window_batch(self.kind, self.size, T["window"].t)


def _sakoe(size, q, t):
    return distance_ref.init_window(distance_ref.SAKOE_CHIBA, size, q, t)


class DtwDistance(po.Case):
    """arm_dtw_distance_f32_batch: the cost matrix, the distance and the status word of every item;
    distance_ref.dtw_distance.  window: None, or the Sakoe-Chiba half width of one device-resident window for
    every item (wStride 0); the distances outside it are NaN (never read)."""
    f32 = True

    def __init__(self, q, t, window):
        self.q, self.t, self.window, self.batch = q, t, window, P
        ops = [po.Op("distance", _F, (P, q, t), "in")]
        if window is not None:
            ops.append(po.Op("window", np.int8, (q, t), "in"))
        ops += [po.Op("dtw", _F, (P, q, t), "out"), po.Op("result", _F, (P, 1), "out"), po.Op("status", np.int32, (P, 1), "out")]
        super().__init__("dtw", f"distance-{q}x{t}" + (f"-sakoe{window}" if window is not None else ""), ops)

    def inputs(self):
        rng = np.random.default_rng([self.q, self.t, 47])
        x = {"distance": rng.uniform(0.0, 1.0, (P, self.q, self.t)).astype(_F)}
        if self.window is not None:
            x["window"] = _sakoe(self.window, self.q, self.t)
            x["distance"][:, x["window"] != 1] = np.nan
        return x

    def expect(self, x):
        r = [distance_ref.dtw_distance(x["distance"][i], x.get("window")) for i in range(P)]
        assert all(st == 0 for st, _, _ in r)
        return [{"dtw": np.stack([c for _, _, c in r]), "result": np.array([v for _, v, _ in r], _F).reshape(P, 1),
                 "status": np.zeros((P, 1), np.int32)}], {}

    def launch(self, dsp, torch, T, call):
        dsp.dtw_distance_batch(T["distance"].t, T["window"].t if self.window is not None else None, T["dtw"].t,
                               T["result"].t, status=T["status"].t)


class DtwPath(po.Case):
    """arm_dtw_path_f32_batch on cost matrices of random distances: the path words up to the length, the words
    past it left alone, and the length; distance_ref.dtw_path."""

    def __init__(self, q, t):
        self.q, self.t, self.batch = q, t, P
        super().__init__("dtw", f"path-{q}x{t}", [po.Op("dtw", _F, (P, q, t), "in"), po.Op("path", np.int16, (P, q + t, 2), "out"),
                                                   po.Op("length", np.int32, (P, 1), "out")])

    def inputs(self):
        rng = np.random.default_rng([self.q, self.t, 53])
        d = rng.uniform(0.0, 1.0, (P, self.q, self.t)).astype(_F)
        return {"dtw": np.stack([distance_ref.dtw_distance(m, None)[2] for m in d])}

    def expect(self, x):
        path = np.zeros((P, self.q + self.t, 2), np.int16)
        alone = np.ones(path.shape, bool)
        length = np.zeros((P, 1), np.int32)
        for i in range(P):
            p = distance_ref.dtw_path(x["dtw"][i])
            path[i, :len(p)], alone[i, :len(p)], length[i, 0] = p, False, len(p)
        return [{"path": (path, alone), "length": length}], {}

    def launch(self, dsp, torch, T, call):
        dsp.dtw_path_batch(T["dtw"].t, T["path"].t, T["length"].t)


# n = 5 and n = 70 as the reductions.  The f32 distances are chains of sums like the statistics: one lane per item
# from kSumLaneMinBatch = 4,096 items on, one wave per item below (4,095).  The boolean distances at 33 bits (a
# second, partial word) and 2,049 bits (65 words: a second round of a wave's lanes).
for _n in (5, 70):
    for _fn in distance_ref.F32_FUNCS:
        for _shared in (False, True):
            _add(Distance(_fn, _n, _shared), "one lane per item; 4,095: one wave per item", (B, 0, 4095))
for _bits in (33, 2049):
    for _fn in distance_ref.BOOL_FUNCS:
        _add(BoolDistance(_fn, _bits), "counts per item, the epilogue per item")
_add(DtwWindow(distance_ref.SAKOE_CHIBA, 1, 3, 4), "every item the same window")
_add(DtwWindow(distance_ref.SLANTED_BAND, 2, 9, 7), "every item the same window")
for _q, _t in ((3, 4), (9, 7)):
    for _w in (None, 1 if _q == 3 else 2):
        _add(DtwDistance(_q, _t, _w), "one item per workgroup slot, the anti-diagonals in turn")
# 33 x 29: long enough that 251 random cost matrices give 251 different paths
_add(DtwPath(33, 29), "one lane per item walks back")


# ------------------------------------------------------------------ log-domain statistics, SVM, naive Bayes, vexp / vlog
class Logdom(po.Case):
    """arm_{entropy,kullback_leibler,logsumexp,logsumexp_dot_prod}_f32_batch; ml_ref.logdom (the host libm's expf / logf)."""
    f32 = libm = True

    def __init__(self, func, n):
        self.func, self.n, self.batch = func, n, P
        self.two = func in ("kullback_leibler", "logsumexp_dot_prod")
        super().__init__("logdom", f"{func}-{n}", [po.Op("a", _F, (P, n), "in")] +
                         ([po.Op("b", _F, (P, n), "in")] if self.two else []) + [po.Op("result", _F, (P, 1), "out")])

    def inputs(self):
        rng = np.random.default_rng([self.n, len(self.func), 59])

        def one():
            if self.func.startswith("logsumexp"):       # log probabilities
                return rng.uniform(-20.0, 20.0, (P, self.n)).astype(_F)
            v = rng.uniform(0.01, 1.0, (P, self.n))
            return (v / v.sum(axis=1, keepdims=True)).astype(_F)
        return dict({"a": one()}, **({"b": one()} if self.two else {}))

    def expect(self, x):
        b = x.get("b")
        return [{"result": np.array([ml_ref.logdom(self.func, x["a"][i], None if b is None else b[i]) for i in range(P)],
                                    _F).reshape(P, 1)}], {}

    def launch(self, dsp, torch, T, call):
        dsp.logdom_batch(self.func, T["a"].t, T["b"].t if self.two else None, T["result"].t)


class Svm(po.Case):
    """arm_svm_<kind>_predict_f32_batch against a device-resident model (dual coefficients, support vectors, classes):
    the class and the decision value of every item; ml_ref.svm_sums / svm_classes.  The intercept, degree, coef0 and
    gamma are the instance's own words."""
    f32 = True

    def __init__(self, kind, nsv, dim):
        self.kind, self.nsv, self.dim, self.batch = kind, nsv, dim, P
        self.libm = kind == "rbf"
        self.m = ml_ref.svm_model(kind, nsv, dim, 3 if kind == "polynomial" else 0, items=P)[0]
        super().__init__("svm", f"{kind}-{nsv}x{dim}",
                         [po.Op("x", _F, (P, dim), "in"), po.Op("dual", _F, (nsv,), "in"), po.Op("sv", _F, (nsv, dim), "in"),
                          po.Op("classes", np.int32, (2,), "in"), po.Op("result", np.int32, (P, 1), "out"),
                          po.Op("decision", _F, (P, 1), "out")])

    def inputs(self):
        m, x = ml_ref.svm_model(self.kind, self.nsv, self.dim, 3 if self.kind == "polynomial" else 0, items=P)
        return {"x": x, "dual": m["dual"], "sv": m["sv"], "classes": m["classes"]}

    def _model(self, x):
        m = dict(self.m)                     # the scalars of the instance
        m.update(dual=np.asarray(x["dual"]), sv=np.asarray(x["sv"]), classes=np.asarray(x["classes"]))
        return m

    def expect(self, x):
        m = self._model(x)
        sums = ml_ref.svm_sums(self.kind, m, x["x"])
        return [{"result": ml_ref.svm_classes(m, sums).reshape(P, 1), "decision": sums.reshape(P, 1)}], {}

    def launch(self, dsp, torch, T, call):
        m = self.m
        S, _keep = dsp.svm_instance(self.kind, m["intercept"], T["dual"].t, T["sv"].t, T["classes"].t,
                                    degree=int(m["degree"]), coef0=float(m["coef0"]), gamma=float(m["gamma"]))
        dsp.svm_predict_batch(self.kind, S, T["x"].t, T["result"].t, T["decision"].t)


class Bayes(po.Case):
    """arm_gaussian_naive_bayes_predict_f32_batch against a device-resident model; ml_ref.bayes_predict."""
    f32 = libm = True

    def __init__(self, c, d):
        self.c, self.d, self.batch = c, d, P
        super().__init__("bayes", f"{c}x{d}",
                         [po.Op("x", _F, (P, d), "in"), po.Op("theta", _F, (c, d), "in"), po.Op("sigma", _F, (c, d), "in"),
                          po.Op("priors", _F, (c,), "in"), po.Op("prob", _F, (P, c), "out"), po.Op("classes", np.int32, (P, 1), "out")])

    def inputs(self):
        m, x = ml_ref.bayes_model(self.c, self.d, items=P)
        return {"x": x, "theta": m["theta"], "sigma": m["sigma"], "priors": m["priors"]}

    def expect(self, x):
        prob, idx = ml_ref.bayes_predict({"theta": x["theta"], "sigma": x["sigma"], "priors": x["priors"], "eps": _F(1e-3)}, x["x"])
        return [{"prob": prob, "classes": idx.view(np.int32).reshape(P, 1)}], {}

    def launch(self, dsp, torch, T, call):
        S, _keep = dsp.bayes_instance(T["theta"].t, T["sigma"].t, T["priors"].t, 1e-3)
        dsp.bayes_predict_batch(S, T["x"].t, T["prob"].t, T["classes"].t)


class FastMath(po.Case):
    """arm_vexp_f32_batch / arm_vlog_f32_batch; the host libm's expf / logf (ml_ref)."""
    f32 = libm = True

    def __init__(self, name, n):
        self.name, self.n, self.batch = name, n, P
        super().__init__("fast_math", f"{name}-{n}", [po.Op("src", _F, (P, n), "in"), po.Op("dst", _F, (P, n), "out")])

    def inputs(self):
        rng = np.random.default_rng([self.n, len(self.name), 61])
        v = rng.uniform(-20.0, 20.0, (P, self.n))
        return {"src": (v if self.name == "vexp" else np.exp(v)).astype(_F)}

    def expect(self, x):
        with np.errstate(all="ignore"):
            return [{"dst": (ml_ref.expf if self.name == "vexp" else ml_ref.logf)(x["src"])}], {}

    def launch(self, dsp, torch, T, call):
        dsp.fast_math_batch(self.name, T["src"].t, T["dst"].t)


# the log-domain sums pick their kernel at kSumLaneMinBatch as the f32 distances do
for _n in (5, 70):
    for _fn in ml_ref.LOGDOM_FUNCS:
        _add(Logdom(_fn, _n), "one lane per item; 4,095: one wave per item", (B, 0, 4095))
for _k in ml_ref.SVM_KINDS:
    _add(Svm(_k, 3, 5), "model staged in LDS, one lane per item")
_add(Bayes(3, 5), "model staged in LDS, one lane per item")
_add(FastMath("vexp", 70), "element-wise, a grid stride over items x n")
_add(FastMath("vlog", 70), "element-wise, a grid stride over items x n")


@functools.lru_cache(maxsize=None)
def _host_libm_ok():
    """The host's expf and logf are the ones the kernels restate (as test_ml.py's host_libm_ok: the recorded words of
    tests/golden/ml.npz).  Where they are not, the rows whose reference words are the host libm's are skipped."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ml.npz"))
    with np.errstate(all="ignore"):
        return ml_ref.same_word(ml_ref.expf(ml_ref.vexp_inputs()), gold["vexp/out"]) and \
            ml_ref.same_word(ml_ref.logf(ml_ref.vlog_inputs()), gold["vlog/out"])


# ------------------------------------------------------------------ the runner
@functools.lru_cache(maxsize=None)
def _built(rid):
    """(inputs, expected words per call, expected words after the last call) of the P patterns, once."""
    case = (ROWS.get(rid) or _TOYS[rid]).case
    x = case.inputs()
    calls, final = case.expect(x)
    for d in calls + [final]:
        for w in d.values():
            for v in (w if isinstance(w, tuple) else (w,)):
                v.setflags(write=False)
    return x, calls, final


class _Empty:
    """An operand of a B = 0 call: zero items at the address of a marker-filled buffer (`full`)."""

    def __init__(self, p):
        self.t, self.ptr, self.full, self.flat, self.hi = p.t[:0], p.ptr, p.t, p.flat, p.hi


def _bits2d(p, n):
    return p._bits[p.lo:p.hi].view(p.shape[0], -1)[:n]


def _chunks(n, row_bytes):
    step = max(1, _CHUNK_BYTES // max(1, row_bytes))
    return [(lo, min(n, lo + step)) for lo in range(0, n, step)]


def _put_tiled(torch, p, pats, idx):
    src = torch.from_numpy(np.ascontiguousarray(pats, dtype=p.dt)).to(p.t.device)
    for lo, hi in _chunks(len(idx), pats[0].nbytes):
        p.t[lo:hi].copy_(src[idx[lo:hi]])


def _compare(case, torch, p, want, idx):
    """None, or what differs between the n items of operand p and pattern idx[i] of `want`."""
    n = len(idx)
    words, mask = want if isinstance(want, tuple) else (want, None)
    bits = f"int{8 * p.dt.itemsize}"
    dev = p.t.device
    w = torch.from_numpy(np.ascontiguousarray(words).view(bits).reshape(P, -1).copy()).to(dev)
    m = None if mask is None or not mask.any() else torch.from_numpy(np.array(mask).reshape(P, -1)).to(dev)
    got = _bits2d(p, n)
    bad = []
    for lo, hi in _chunks(n, 2 * words[0].nbytes):
        ne = got[lo:hi] != w[idx[lo:hi]]
        if m is not None:                    # the words the reference leaves alone keep the marker
            ne = torch.where(m[idx[lo:hi]], got[lo:hi] != p.word, ne)
        bad.append(torch.nonzero(ne.any(dim=1)).flatten() + lo)
    bad = torch.cat(bad).cpu().numpy() if bad else np.zeros(0, np.int64)
    if not len(bad):
        return None
    # the items whose bits differ, by the suite's own comparison (f32: NaNs by position)
    some = bad[:64]
    g = got[torch.from_numpy(some).to(dev)].cpu().numpy().view(p.dt).reshape((len(some),) + p.shape[1:])
    rule = copy.copy(case)                  # the f32 rule (NaNs by position) for f32 words only
    rule.f32 = p.dt == np.float32
    msg = po._diff(rule, g, (words[some % P], mask[some % P]) if mask is not None else words[some % P], p.word)
    if msg is None and len(bad) > len(some):
        msg = "bits differ"
    if msg is None:
        return None
    where = [(int(i), int(i) % EDGE, int(i) % P) for i in bad[:6]]
    return f"{len(bad)} of {n} items differ, the first as (item, item % 65536, item % {P}): {where}: {msg}"


def _pads_ok(p, whole=False):
    b = p._bits
    if whole:
        return bool((b == p.word).all())
    return bool((b[:p.lo] == p.word).all() and (b[p.hi:] == p.word).all())


def _run(row, dsp, torch, n, device="cuda"):
    """One run of `row` at n items; raises with every failure in one message."""
    case = row.case
    x, calls, final = _built(row.id)
    idx = torch.arange(n, device=device) % P
    run = copy.copy(case)
    run.batch = n
    assert row.id in _BIG or max(n, 1) * row.item_bytes() <= GIB, (row.id, n)
    T = {}
    for op in case.ops:
        shape = (max(n, 1),) + op.shape[1:] if _per_item(op) else op.shape
        T[op.name] = Padded(torch, op.dt, shape, 0, po._op_fill(op, FILL_A), device=device)
        if not _per_item(op):
            T[op.name].put(torch, x[op.name])
        elif n and op.role == "state":
            T[op.name].t.zero_()
        elif n and op.name in x and not isinstance(x[op.name], list):
            _put_tiled(torch, T[op.name], x[op.name], idx)
    V = T if n else {k: (_Empty(p) if _per_item(case_op) else p)
                     for (k, p), case_op in zip(T.items(), case.ops)}
    bad = []
    for k in range(case.ncalls):
        for op in case.ops:
            if not (n and _per_item(op)):
                continue
            if op.role == "out":
                T[op.name].reset()
            elif isinstance(x.get(op.name), list):
                _put_tiled(torch, T[op.name], x[op.name][k], idx)
        if dsp is not None:
            dsp.lib.arm_mi355x_clear_error()
        run.launch(dsp, torch, V, k)
        if device == "cuda":
            torch.cuda.synchronize()
        if dsp is not None and dsp.last_error()[0]:
            bad.append(f"call {k}: error recorded: {dsp.last_error()}")
        if not n:
            continue
        for name, want in list(calls[k].items()) + (list(final.items()) if k == case.ncalls - 1 else []):
            msg = _compare(case, torch, T[name], want, idx)
            if msg:
                bad.append(f"call {k} {name}: {msg}")
    for op in case.ops:
        touched = not n and _per_item(op) and not _pads_ok(T[op.name], whole=True)
        if touched:
            bad.append(f"{op.name}: written by a call of 0 items")
        elif not _pads_ok(T[op.name]):
            bad.append(f"{op.name}: guard words written")
    assert not bad, f"{row.id} at {n} items ({row.note}): {len(bad)} failures:\n" + "\n".join(bad[:12])


def _ids(family):
    return [(rid, n) for rid, r in ROWS.items() if r.family == family for n in r.batches]


def _family_test(family):
    @pytest.mark.gpu
    @pytest.mark.parametrize("rid,n", _ids(family), ids=[f"{r}-B{n}" for r, n in _ids(family)])
    def test(dsp, torch_gpu, rid, n):
        if getattr(ROWS[rid].case, "libm", False) and not _host_libm_ok():
            pytest.skip("host libm differs: the restatement's words are another expf's / logf's")
        _run(ROWS[rid], dsp, torch_gpu, n)
    test.__name__ = test.__qualname__ = f"test_{family}_batch_counts"
    test.__doc__ = f"Every row of the {family} family at B, at 0 and below its threshold: see the module docstring."
    return test


_FAMILIES = sorted({r.family for r in ROWS.values()})
for _f in _FAMILIES:
    globals()[f"test_{_f}_batch_counts"] = _family_test(_f)


# ------------------------------------------------------------------ the K > 32,704 fall-back GEMM kernels
# One thread per output with an int64 sum.  At B their operands alone would take over 4 GB, so the kernels, whose
# grid carries the batch on x like the others', run here at 3 items, with more than one row and more than one
# 256-column block per item.
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["q15", "q31", "fast_q15", "cmplx_q15", "cmplx_q31"])
def test_gemm_long_k_fallback_small_batch(dsp, torch_gpu, kind):
    """mat_mult_fixed_valu_kernel at 3 x 32705 x 300 and mat_cmplx_mult_fixed_valu_kernel at complex 2 x 16353 x 130
    (real depth 32706, 260 output words a row), 3 items: every word as the reference's, the guards untouched."""
    torch = torch_gpu
    base = po._base(kind)
    rng = np.random.default_rng(len(kind))
    if kind.startswith("cmplx"):
        a, b = cmplx_mat_ref.operands(base, "full", 2, 16353, 130, rng, 3)
        want = cmplx_mat_ref.mult_fixed(base, a, b)
    else:
        a, b = po._rand(base, (3, 3, 32705), rng), po._rand(base, (3, 32705, 300), rng)
        want = np.stack([refs.ref_lib().mat_mult_fixed(kind, a[i], b[i])[1] for i in range(3)])
    da, db = Padded(torch, DT[base], a.shape, 0, FILL_A).put(torch, a), Padded(torch, DT[base], b.shape, 0, FILL_A).put(torch, b)
    dc = Padded(torch, DT[base], want.shape, 0, FILL_A)
    if kind.startswith("cmplx"):
        dsp.mat_cmplx_mult_batch(da.t, db.t, dc.t)
    else:
        dsp.mat_mult_batch(da.t, db.t, dc.t, fast=kind.startswith("fast"))
    torch.cuda.synchronize()
    got, pads_ok = dc.fetch()
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    assert pads_ok and da.fetch()[1] and db.fetch()[1]


# ------------------------------------------------------------------ the one inherent limit: 2^31 - 1 workgroups
_MAT = {"f32": ("arm_matrix_instance_f32", "c_f32p"), "q31": ("arm_matrix_instance_q31", "c_i32p"),
        "q15": ("arm_matrix_instance_q15", "c_i16p"), "q7": ("arm_matrix_instance_q7", "c_i8p")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mat_mult_f32", "mat_mult_q7", "mat_mult_q15", "mat_mult_q31", "mat_mult_fast_q15",
                                  "mat_mult_fast_q31", "mat_cmplx_mult_f32", "mat_cmplx_mult_q31", "mat_cmplx_mult_q15"])
def test_gemm_grid_limit_is_refused(dsp, torch_gpu, name):
    """65535 x 16 x 65535 items are at least 256 x 256 = 65,536 tiles of any GEMM kernel, so 32,768 of them are
    at least 2^31 workgroups, one more than grid x takes: the call launches nothing (the operands are 64 marker
    words, untouched), returns ARM_MATH_ARGUMENT_ERROR and names the product and the limit."""
    torch = torch_gpu
    kind = name.split("_")[-1]
    inst, ptr = getattr(dsp, _MAT[kind][0]), getattr(_abi, _MAT[kind][1])
    bufs = [Padded(torch, DT[kind], (64,), 0, F32_SENTINEL if kind == "f32" else FILL_A) for _ in range(3)]
    A, Bm, Cm = (inst(r, c, C.cast(p.ptr, ptr)) for (r, c), p in zip(((65535, 16), (16, 65535), (65535, 65535)), bufs))
    dsp.lib.arm_mi355x_clear_error()
    st = getattr(dsp.lib, f"arm_{name}_batch")(C.byref(A), C.byref(Bm), C.byref(Cm), 32768, _stream_of(torch))
    torch.cuda.synchronize()
    code, msg = dsp.last_error()
    dsp.lib.arm_mi355x_clear_error()
    assert st == _abi.ARM_MATH_ARGUMENT_ERROR and code != 0
    assert msg.startswith(f"arm_{name}_batch") and "tiles x batch > 2147483647 workgroups" in msg, msg
    assert all(_pads_ok(p, whole=True) for p in bufs)


# ------------------------------------------------------------------ the table, on the CPU
@pytest.mark.parametrize("family", _FAMILIES)
def test_case_table_builds_on_cpu(family):
    """Builds every row's 251 patterns and reference words; checks their shapes and dtypes against the
    operands, that expect(n) is the patterns tiled (item i = pattern i % 251, across the 2^16 edge), that
    the patterns differ pairwise in an output word and from the pattern a wrap at 2^16 .. 2^32 would read (a
    wrapped index shows), and the device-memory budget."""
    rows = [r for r in ROWS.values() if r.family == family]
    assert rows
    for row in rows:
        case = row.case
        x, calls, final = _built(row.id)
        names = {op.name: op for op in case.ops}
        assert case.batch == P and len(calls) == case.ncalls and any(_per_item(op) for op in case.ops), row.id
        assert row.batches[:2] == (max(row.batches), 0) and row.batches[0] > 65535, row.id
        for name, v in x.items():
            for a in (v if isinstance(v, list) else [v]):
                assert a.shape == names[name].shape and a.dtype == names[name].dt, (row.id, name, a.shape, a.dtype)
        outs = []
        for d in calls + [final]:
            for name, w in d.items():
                w, mask = w if isinstance(w, tuple) else (w, None)
                assert w.shape == names[name].shape and w.dtype == names[name].dt and _per_item(names[name]), (row.id, name)
                assert mask is None or mask.shape == w.shape
                outs.append(np.ascontiguousarray(w).reshape(P, -1).view(np.uint8))
        for op in case.ops:
            assert (op.name in x) == (op.role in ("in", "io")), (row.id, op.name)
        outs = np.concatenate(outs, axis=1)
        # an entry point without a per-item input (dtw_init_window) gives every item the same words by definition
        uniform = getattr(case, "uniform", False)
        assert not uniform or (not x and not (outs != outs[0]).any()), row.id
        # a result of one word per item (at most four varying bytes) need not differ among all 251 patterns
        if (outs != outs[0]).any(axis=0).sum() > 4:
            assert len(np.unique(outs, axis=0)) == P, f"{row.id}: two patterns give the same words"
        # an index wrapped at 2^k reads pattern (i - 2^k) % 251; the 511 items of B past 2^16 hold every pattern
        # twice, so with half the patterns moving a wrap makes some 250 wrong items (the maximum of 70 q7 words
        # is 127 in a fifth of the patterns: not every one can move)
        for k in () if uniform else range(16, 33):
            moved = (outs != np.roll(outs, (1 << k) % P, axis=0)).any(axis=1)
            assert moved.sum() >= P // 2, f"{row.id}: a wrap at 2^{k} would show in {moved.sum()} patterns only"
        n = EDGE + 2 * P + 7
        calls_n, final_n = row.expect(n)
        probe = np.array([0, 1, P - 1, P, 65535, 65536, 65536 + P, n - 1])
        for d, dn in zip(calls + [final], calls_n + [final_n]):
            for name, w in d.items():
                for v, vn in zip(*((w, dn[name]) if isinstance(w, tuple) else ((w,), (dn[name],)))):
                    assert vn.shape == (n,) + v.shape[1:]
                    assert vn[probe].tobytes() == v[probe % P].tobytes(), (row.id, name)
        assert row.id in _BIG or max(row.batches) * row.item_bytes() <= GIB, (row.id, row.item_bytes())
    assert 65536 % P == 25 and all((1 << k) % P for k in range(16, 33))


# ------------------------------------------------------------------ the runner's negative controls, on the CPU
class Toy(po.Case):
    """dst[i] = src[i] + 1 over the batch on the CPU, with one planted defect."""
    kind = "q31"

    def __init__(self, defect):
        self.defect, self.batch = defect, P
        super().__init__("toy", defect, [po.Op("src", np.int32, (P, 3), "in"), po.Op("dst", np.int32, (P, 3), "out")])

    def inputs(self):
        return {"src": po._rand("q31", (P, 3), np.random.default_rng(3)) // 2}

    def expect(self, x):
        return [{"dst": (x["src"] + 1).astype(np.int32)}], {}

    def launch(self, dsp, torch, T, call):
        src, dst, n = T["src"], T["dst"], self.batch
        i = torch.arange(n)
        if self.defect == "wrap":           # a 16-bit item index
            i = i % EDGE
        if self.defect == "skip":           # a grid that stops at 65,535
            i = i[:65535]
        if self.defect == "zero_as_one" and n == 0:
            dst.full[0] = src.full[0] + 1
            return
        dst.t[:len(i)] = src.t[i] + 1
        if self.defect == "store_after":
            dst.flat[dst.hi] = 7


for _d in ("none", "wrap", "skip", "store_after", "zero_as_one"):
    _TOYS[f"toy-{_d}"] = Row(Toy(_d), "toy")


def test_runner_reports_planted_defects():
    """_run on CPU-backed operands at B and at 0: a clean toy kernel passes both; an item index wrapped at
    2^16 and a launch that drops the items from 65,535 on are wrong items, reported from the first such
    item with its index mod 65536; a store one word past the last item is a written guard; a call of 0
    items that processes one is reported."""
    import torch
    for n in (B, 0):
        _run(_TOYS["toy-none"], None, torch, n, device="cpu")
    with pytest.raises(AssertionError, match=r"511 of 66047 items differ.*\(65536, 0, 25\)"):
        _run(_TOYS["toy-wrap"], None, torch, B, device="cpu")
    with pytest.raises(AssertionError, match=r"512 of 66047 items differ.*\(65535, 65535, 24\)"):
        _run(_TOYS["toy-skip"], None, torch, B, device="cpu")
    with pytest.raises(AssertionError, match="guard words written"):
        _run(_TOYS["toy-store_after"], None, torch, B, device="cpu")
    with pytest.raises(AssertionError, match="written by a call of 0 items"):
        _run(_TOYS["toy-zero_as_one"], None, torch, 0, device="cpu")
    for d in ("wrap", "skip"):                  # neither shows at 0 items
        _run(_TOYS[f"toy-{d}"], None, torch, 0, device="cpu")
    _run(_TOYS["toy-zero_as_one"], None, torch, B, device="cpu")
