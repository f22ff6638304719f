"""The batched entry points under a caller who is not synchronised: "asynchronous, stream-ordered, no host
synchronisation" (INTEGRATION.md).

The other GPU tests call on the current stream with torch.cuda.synchronize() around the call; work the library put
on another stream, or an operand it read too early on the host, still gives the right words there.  Here every case
of the table runs on a non-blocking side stream behind a device-side delay, with operands that hold another valid
set of words (the decoy) until the stream itself overwrites them:

1. default stream: the case's own inputs() / expect() give the true words and the reference; the same inputs()
   under another seed (_reseeded) give the decoy, a second valid set of words for every operand, index tables
   included.  Every input, state and device-resident table holds its decoy, every output the marker.  One warm-up
   call on separate buffers (true words) gets the library's cached table uploads and the first growth of the
   stream-ordered memory pool out of the way.  torch.cuda.synchronize().
2. side stream: torch.cuda._sleep(delay); device-to-device copies of the true words into every input / state /
   table; case.launch(); a snapshot of every output and state operand (guards included); the decoy back over the
   inputs and tables, the marker back over the outputs.
3. side.query() and the host time of launch() are read as soon as launch() returns.
4. after a synchronise: no error was raised or recorded, the snapshots equal the reference (test_gpu_pointer_offsets'
   _diff: byte equality, assert_same_words for f32), the guards are intact, query() was False at 3 and launch() took
   less than half the delay.  (query() alone passes a call that waits for the stream and then launches: its own
   launch keeps the stream busy for a moment.  The toy control below showed exactly that, hence the second half.)

The late write fails any internal step on another stream and any early host read; the re-poisoning fails work that
was deferred to another stream without making the caller's stream wait; query() == False pins "no host
synchronisation" and shows that the delay outlasted the enqueue, so a pass is never luck.  A defective ordering
gives wrong words, never an out-of-range index: no operand ever holds a word the reference could not run on.
Streaming cases run their two calls this way, the state carried from the first call's snapshot.

MAY_SYNC is the closed set of cases that read a caller's device-resident table on the host and therefore wait for
the call's own stream (hipMemcpyAsync + hipStreamSynchronize on it): check 3 is not made for them,
everything else is.  test_may_sync_is_a_closed_set pins the set by name.

Decoys.  inputs() under _reseeded() is the decoy; an operand that no seed reaches gets a chosen one: library tables
loaded from files and the SVM class labels are rotated by one word (_ROLL: any words are valid there), and the
index-like tables are replaced by another valid table (SCase.fix): Mel filter positions one bin lower, filter lengths
one shorter (every mix of true and decoy stays within the spectrum), a bit-reversal table with other pairs made
no-ops, a wider Sakoe-Chiba window (the distances outside the true window are NaN: a stale window gives NaN costs, not
a missing path), the reciprocal table reversed.  test_stale_operand_is_visible shows, on the CPU, that for every
late-written operand of every case expect() with that operand alone replaced by its decoy differs from the true
reference in an output word.  expect() cannot take the zero start of a role-"state" operand (its decoy is random
words): test_stale_start_state_is_visible shows on the GPU that the first call on the decoy state gives other output
words than the reference.  Operands of zero size (the k == 0 GEMM) have no word that could be stale.

The streams.  HIP streams can share a hardware queue, the null stream included; work misplaced on a stream that shares
the delayed stream's queue would wait behind the delay, read the true words and pass.  So the module uses one set
of streams for every case, the pair and the negative controls (the `streams` fixture), and qualifies it first: while
side sleeps, an operation on the null stream, on third and on twin must complete (an event's query()), and the same
for twin against the null stream and side.  A candidate that fails is dropped and another drawn; the test fails if
none qualifies.  A green negative control therefore vouches for exactly the streams the cases run on.

Two streams at once (test_two_streams_*): the cases that allocate a stream-ordered temporary (Case.alloc) run
together with their decoy-seeded twin on two side streams from one thread, enqueued alternately behind one delay
each; both must give their own reference words.

The delay.  torch.cuda._sleep is calibrated once per module with a pair of events (its cycle unit is the device's
clock, which the test does not assume) and sized for 50 ms.  Nothing rests on the figure: check 3 fails the case if
the delay was too short.  Measured on an MI355X: 2.40 million cycles per millisecond (2,397,199 and 2,401,917 in two
runs), and 0.81 / 1.09 ms in two runs for the longest host-side launch() of the table (biquad_cascade_df1_q15 at 65
stages, two launches); no candidate stream had to be dropped; the `streams` fixture prints both when the module ends (pytest -s).  The bound that matters is per case:
launch() under half the delay, which a host stall of 25 ms on a busy machine would also trip.

Rows come from test_gpu_pointer_offsets.py (batch 5 or 37, 256 for the MFMA FIR floor) and test_gpu_batch_counts.py
(whose row classes carry 251 items); one case per distinct host-side launch sequence, at the smallest shape that
reaches it.  Beyond the obvious multi-operation sequences (in-place copies, tap images, work areas), reading api.cpp / api_vector.cpp and the *_launch functions gave:
the decimators' and interpolators' own kernels allocate a stream-ordered phase-row image (fir.hip mr_decim_rows /
mr_phase_coeffs) -- their M, L = 5 cases are in the two-stream set; biquad allocates only for a partial overlap
of src and dst (biquad-overlap); the f32 convolutions reverse the template into a stream-ordered copy for per-item
and for shared templates alike (both in the two-stream set).

Negative controls (gpu): toy "entry points" through the same runner on their own small buffers -- a copy on the
default stream, a copy on a third stream without an event wait, and a correct copy behind side.synchronize(); the
runner must report each.  They read stale words of their own buffers; nothing can fault.
"""
import contextlib
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

import adaptive_ref
import basic_math_ref
import biquad_ref
import cmplx_math_ref
import distance_ref
import mat_basic_ref
import refs
import support_ref
import test_gpu_batch_counts as bc
import test_gpu_pointer_offsets as po
from cmsisdsp_amd import _abi
from padded import FILL_A, Padded

Op = po.Op
DT = refs.DTYPE
TABLES = po.TABLES
SALT = 0x5EED
SLEEP_MS = 50.0
_ROLL = {"tw", "classes"}                   # operands whose decoy is the true words rotated by one: any words are valid
_SEEN = {"launch_ms": 0.0, "case": None, "cycles_per_ms": None}


@contextlib.contextmanager
def _reseeded(salt=SALT):
    """Every np.random.default_rng(seed) inside gives the generator of (salt, seed): the same case, another seed."""
    orig = np.random.default_rng

    def rng(seed=None):
        return orig([salt] + [int(v) for v in np.atleast_1d(np.asarray(seed)).reshape(-1)])
    np.random.default_rng = rng
    try:
        yield
    finally:
        np.random.default_rng = orig


class SCase:
    """A row: the case object (the pointer-offset table's kind), which launch sequence it reaches, whether it may
    synchronise on the call's stream (sync), whether the call allocates a stream-ordered temporary (alloc: it also
    runs in the two-stream test), element offsets of operands, and the chosen decoys (fix: operand -> f(true words))."""

    def __init__(self, case, note, sync=False, alloc=False, offsets=None, fix=None):
        self.case, self.note, self.sync, self.alloc = case, note, sync, alloc
        self.offsets, self.fix = offsets or {}, fix or {}
        self.id, self.family = case.id, case.family


CASES = {}
_TOYS = {}


def _add(case, note, **kw):
    assert case.id not in CASES, case.id
    CASES[case.id] = SCase(case, note, **kw)


def _retag(case, suffix):
    case.id += suffix
    return case


# ------------------------------------------------------------------ row classes this table adds
class InPlace(po.Case):
    """`base` with its output operand `dst` being its input `src` (the same device words)."""

    def __init__(self, base, src="src", dst="dst"):
        self.base, self.src, self.dst = base, src, dst
        self.ncalls, self.f32, self.compare = base.ncalls, base.f32, base.compare
        self.libm = getattr(base, "libm", False)
        ops = [Op(o.name, o.dt, o.shape, "io" if o.name == src else o.role) for o in base.ops if o.name != dst]
        super().__init__(base.family, base.id[len(base.family) + 1:] + "-inplace", ops)

    def inputs(self):
        return self.base.inputs()

    def expect(self, x):
        calls, final = self.base.expect(x)
        return [{(self.src if k == self.dst else k): w for k, w in d.items()} for d in calls], final

    def launch(self, dsp, torch, T, call):
        self.base.launch(dsp, torch, dict(T, **{self.dst: T[self.src]}), call)


class BiquadDev(bc.Biquad):
    """bc.Biquad with pCoeffs resident in device memory (an operand, so expect() takes the coefficients)."""

    def __init__(self, func, stages, block):
        super().__init__(func, stages, block)
        self.id += "-devcoeffs"
        c = self._coeffs()
        self.ops.append(Op("coeffs", c.dtype, c.shape, "in"))

    def inputs(self):
        return dict(super().inputs(), coeffs=biquad_ref.stable_coeffs(self.func, self.stages, self.ps, 1000 + self.stages))

    def expect(self, x):
        _, sdt, ks, _, _ = biquad_ref.FUNCS[self.func]
        st, calls = np.zeros((bc.P, ks * self.stages), dtype=sdt), []
        for k in range(2):
            y, st = biquad_ref.run(self.func, x["coeffs"], self.ps, x["src"][k], st)
            calls.append({"dst": y, "state": bc._words32(st)})
        return calls, {}

    def launch(self, dsp, torch, T, call):
        inst = _abi.BIQUAD_FUNCS[self.func][0]
        kw = {"postShift": self.ps} if any(f == "postShift" for f, _ in inst._fields_) else {}
        S = inst(numStages=self.stages, pState=None, pCoeffs=T["coeffs"].ptr, **kw)
        st = getattr(dsp.lib, self.func + "_batch")(C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block,
                                                    self.batch, C.c_void_p(T["state"].ptr), bc._stream_of(torch))
        assert st == 0, dsp.last_error()


class BiquadOverlap(bc.Biquad):
    """src and dst one sample row apart in one buffer of 252 rows: src = rows 0 .. 250, dst = rows 1 .. 251, a partial
    overlap, which the launch filters from a stream-ordered copy of the input.  Row 0 keeps the input's row 0."""

    def __init__(self, func, stages, block):
        super().__init__(func, stages, block)
        self.id += "-overlap"
        src = self.ops[0]
        self.ops = [Op("buf", src.dt, (bc.P + 1,) + src.shape[1:], "io"), self.ops[2]]

    def inputs(self):
        x = super().inputs()
        return {"buf": [np.concatenate([s, np.zeros_like(s[:1])]) for s in x["src"]]}

    def expect(self, x):
        calls, final = super().expect({"src": [b[:-1] for b in x["buf"]]})
        return [{"buf": np.concatenate([b[:1], d["dst"]]), "state": d["state"]} for b, d in zip(x["buf"], calls)], final

    def launch(self, dsp, torch, T, call):
        buf = T["buf"]
        row = buf.t.shape[1] * buf.dt.itemsize

        class View:
            def __init__(self, ptr):
                self.ptr = ptr
        super().launch(dsp, torch, {"src": View(buf.ptr), "dst": View(buf.ptr + row), "state": T["state"]}, call)


class IirLatticeDev(bc.IirLattice):
    """bc.IirLattice with pkCoeffs / pvCoeffs resident in device memory."""

    def __init__(self, func, stages, block):
        super().__init__(func, stages, block)
        self.id += "-devcoeffs"
        dt = adaptive_ref.FUNCS[func][0]
        self.ops += [Op("k", dt, (stages,), "in"), Op("v", dt, (stages + 1,), "in")]

    def inputs(self):
        k, v = adaptive_ref.lattice_coeffs(self.func, self.stages, 1000 + self.stages)
        return dict(super().inputs(), k=k, v=v)

    def expect(self, x):
        st, calls = x["state"], []
        for i in range(2):
            y, st = adaptive_ref.iir_lattice(self.func, x["k"], x["v"], x["src"][i], st)
            calls.append({"dst": y, "state": st})
        return calls, {}

    def launch(self, dsp, torch, T, call):
        S = _abi.ADAPTIVE_FUNCS[self.func][0](numStages=self.stages, pState=None, pkCoeffs=T["k"].ptr, pvCoeffs=T["v"].ptr)
        st = getattr(dsp.lib, self.func + "_batch")(C.byref(S), C.c_void_p(T["src"].ptr), C.c_void_p(T["dst"].ptr), self.block,
                                                    self.batch, C.c_void_p(T["state"].ptr), bc._stream_of(torch))
        assert st == 0, dsp.last_error()


class LmsRecip(bc.Lms):
    """arm_lms_norm_q15 with a device-resident recipTable."""

    def __init__(self, taps, block):
        super().__init__("arm_lms_norm_q15", taps, block)
        self.id += "-devrecip"
        self.ops.append(Op("recip", np.int16, (64,), "in"))

    def inputs(self):
        return dict(super().inputs(), recip=adaptive_ref.recip_table())

    def expect(self, x):
        c, st, ex, calls = x["coeffs"], x["state"], x["ex"], []
        for i in range(2):
            y, e, c, st, ex = adaptive_ref.lms(self.func, self.mu, self.ps, x["src"][i], x["ref"][i], c, st, ex,
                                               table=np.asarray(x["recip"]))
            calls.append({"out": y, "err": e, "coeffs": c, "state": st, "ex": ex})
        return calls, {}

    def launch(self, dsp, torch, T, call):
        S = _abi.ADAPTIVE_FUNCS[self.func][0](numTaps=self.taps, pState=None, pCoeffs=None, mu=self.mu, postShift=self.ps,
                                              recipTable=T["recip"].ptr)
        ptr = lambda name: C.c_void_p(T[name].ptr)   # noqa: E731
        st = getattr(dsp.lib, self.func + "_batch")(C.byref(S), ptr("src"), ptr("ref"), ptr("out"), ptr("err"), self.block,
                                                    self.batch, ptr("coeffs"), ptr("state"), ptr("ex"), bc._stream_of(torch))
        assert st == 0, dsp.last_error()


def _bitrev_table(kind, n):
    name = f"armBitRevIndexTable{n}.bin" if kind == "f32" else f"armBitRevIndexTable_fixed_{n}.bin"
    return np.fromfile(os.path.join(TABLES, name), dtype=np.uint16)


def _bitrev_without(table, first):
    """The library's swap table with four of its pairs, from pair `first` on, made (0, 0): a valid table that induces
    another permutation than the reference's own (and than the table with other pairs removed)."""
    t = table.copy()
    t[2 * first:2 * first + 8] = 0
    return t.view(np.int16)


class CfftBitrev(po.Cfft):
    """arm_cfft_*_batch with a user bit-reversal table (not the reference's permutation) resident in device memory."""

    def __init__(self, kind, n, batch):
        super().__init__(kind, n, 0, 1, batch)
        self.id += "-devbitrev"
        self.table = _bitrev_table(kind, n)
        self.ops.append(Op("bitrev", np.int16, self.table.shape, "in"))

    def inputs(self):
        return dict(super().inputs(), bitrev=_bitrev_without(self.table, 1))

    def expect(self, x):
        r = refs.ref_lib()
        S = r.cfft_instance(self.kind, self.n)
        assert S.bitRevLength == len(self.table)
        tab = np.ascontiguousarray(x["bitrev"])
        S.pBitRevTable = C.cast(po._ptr(tab), type(S.pBitRevTable))
        out = np.ascontiguousarray(x["data"][0]).copy()
        f = r.fn(f"arm_cfft_{self.kind}")
        for row in out:
            f(C.byref(S), po._ptr(row), self.ifft, self.bitrev)
        return [{"data": out}], {}

    def launch(self, dsp, torch, T, call):
        S = getattr(dsp, f"arm_cfft_instance_{self.kind}")()
        assert getattr(dsp, f"arm_cfft_init_{self.kind}")(S, self.n) == 0
        S.pBitRevTable = C.cast(T["bitrev"].ptr, type(S.pBitRevTable))
        dsp.cfft_batch(S, T["data"].t, self.ifft, self.bitrev)


class RfftFixedAB(po.RfftFixed):
    """arm_rfft_{q31,q15}_batch with altered realCoefA / realCoefB tables resident in device memory (the case of
    test_rfft_fixed.py's test_rfft_fixed_device_tables_written_on_the_call_stream)."""

    def __init__(self, kind, n, ifft, batch=5):
        super().__init__(kind, n, ifft, batch)
        self.id += "-devAB"
        self.ops += [Op("ta", DT[kind], (8192,), "in"), Op("tb", DT[kind], (8192,), "in")]

    def inputs(self):
        x = super().inputs()
        rng = np.random.default_rng([self.n, self.ifft, 77])
        info = np.iinfo(DT[self.kind])
        for name, f in (("ta", "realCoefAQ"), ("tb", "realCoefBQ")):
            t = np.fromfile(os.path.join(TABLES, f"{f}{self.kind[1:]}.bin"), dtype=DT[self.kind])
            t[::5] = rng.integers(info.min, info.max, t[::5].size, dtype=DT[self.kind])
            x[name] = t
        return x

    def _with_tables(self, init, pa, pb):
        S, keep = self._instance(init, None)
        assert S.twidCoefRModifier * self.n == 8192
        S.pTwiddleAReal = C.cast(pa, type(S.pTwiddleAReal))
        S.pTwiddleBReal = C.cast(pb, type(S.pTwiddleBReal))
        return S, keep

    def expect(self, x):
        r = refs.ref_lib()
        ta, tb = np.ascontiguousarray(x["ta"]), np.ascontiguousarray(x["tb"])
        S, _keep = self._with_tables(r.fn(f"arm_rfft_init_{self.kind}"), po._ptr(ta), po._ptr(tb))
        src = np.ascontiguousarray(x["src"][0]).copy()
        dst = np.zeros((self.batch, self.wout), DT[self.kind])
        f = r.fn(f"arm_rfft_{self.kind}")
        for i in range(self.batch):
            f(C.byref(S), po._ptr(src[i]), po._ptr(dst[i]))
        return [dict({"dst": dst}, **({"src": src} if self.ifft != 1 else {}))], {}

    def launch(self, dsp, torch, T, call):
        S, _keep = self._with_tables(getattr(dsp.lib, f"arm_rfft_init_{self.kind}"), T["ta"].ptr, T["tb"].ptr)
        dsp.rfft_fixed_batch(S, T["src"].t, T["dst"].t)


class GemmK0(po.Case):
    """k == 0: the product is the zero matrix, written by one hipMemsetAsync on the call's stream."""

    def __init__(self, kind, m, n, batch=5):
        self.kind, self.m, self.n, self.batch = kind, m, n, batch
        self.f32 = kind == "f32"
        dt = DT[po._base(kind)]
        super().__init__("gemm", f"{kind}-{m}-0-{n}", [Op("a", dt, (batch, m, 0), "in"), Op("b", dt, (batch, 0, n), "in"),
                                                        Op("c", dt, (batch, m, n), "out")])

    def inputs(self):
        dt = DT[po._base(self.kind)]
        return {"a": np.zeros((self.batch, self.m, 0), dt), "b": np.zeros((self.batch, 0, self.n), dt)}

    def expect(self, x):
        return [{"c": np.zeros((self.batch, self.m, self.n), DT[po._base(self.kind)])}], {}

    def launch(self, dsp, torch, T, call):
        dsp.mat_mult_batch(T["a"].t, T["b"].t, T["c"].t, fast=self.kind.startswith("fast"))


class MfccDev(bc.Mfcc):
    """The MFCC rows with the five instance tables resident in device memory (filterPos / filterLengths as the int32
    words they are in memory)."""

    def __init__(self, kind, n, batch):
        super().__init__(kind, n, True, batch)
        self.id += "-devtables"
        c, dt = self.cfg, DT[kind]
        self.ops += [Op("dct", dt, c["dct"].shape, "in"), Op("pos", np.int32, c["pos"].shape, "in"),
                     Op("len", np.int32, c["len"].shape, "in"), Op("coefs", dt, c["coefs"].shape, "in"),
                     Op("window", dt, c["window"].shape, "in")]

    def inputs(self):
        c = self.cfg
        return dict(super().inputs(), dct=c["dct"], pos=c["pos"].view(np.int32), len=c["len"].view(np.int32), coefs=c["coefs"],
                    window=c["window"])

    def expect(self, x):
        cfg = dict(self.cfg, dct=x["dct"], pos=np.ascontiguousarray(x["pos"]).view(np.uint32),
                   len=np.ascontiguousarray(x["len"]).view(np.uint32), coefs=x["coefs"], window=x["window"])
        r = refs.ref_lib()
        fn = {"f32": r.mfcc, "q31": r.mfcc_q31, "q15": r.mfcc_q15}[self.kind]
        return [{"out": fn(cfg, x["frames"][0])}], {}

    def launch(self, dsp, torch, T, call):
        cls = {"f32": dsp.MfccF32, "q31": dsp.MfccQ31, "q15": dsp.MfccQ15}[self.kind]
        m = cls(self.n, T["dct"].t, T["pos"].t, T["len"].t, T["coefs"].t, T["window"].t)
        m.batch(T["frames"].t, T["out"].t, T["work"].t)


_MFCC_FIX = {"dct": lambda v: np.ascontiguousarray(v[:, ::-1]), "coefs": lambda v: np.ascontiguousarray(v[::-1]),
             "window": lambda v: np.roll(v, len(v) // 4), "pos": lambda v: np.maximum(v - 1, 0).astype(v.dtype),
             "len": lambda v: np.where(v > 1, v - 1, v).astype(v.dtype)}


class MfccBitrev(bc.Mfcc):
    """MFCC whose inner CFFT has a user bit-reversal table (host memory) that is not the reference's permutation: the
    three-launch path (pre, RFFT / CFFT, post) of mfcc_run."""

    def __init__(self, kind, n, batch):
        super().__init__(kind, n, True, batch)
        self.id += "-bitrev"
        self.table = _bitrev_without(_bitrev_table(kind, n // 2), 1)

    def _patched(self, S):
        """Points the instance's inner CFFT at self.table; returns what must stay alive with S."""
        if self.f32:
            inner = S.rfft.Sint
        else:                                # the fixed-point RFFT points at a constant CFFT instance: a private copy
            inner = type(S.rfft.pCfft.contents)()
            C.memmove(C.byref(inner), S.rfft.pCfft, C.sizeof(inner))
            S.rfft.pCfft = C.pointer(inner)
        assert inner.fftLen == self.n // 2 and inner.bitRevLength == len(self.table)
        inner.pBitRevTable = C.cast(po._ptr(self.table), type(inner.pBitRevTable))
        return inner

    def expect(self, x):
        r, c, n, dt = refs.ref_lib(), self.cfg, self.n, DT[self.kind]
        keep = [np.ascontiguousarray(c["dct"], dt), np.ascontiguousarray(c["pos"], np.uint32),
                np.ascontiguousarray(c["len"], np.uint32), np.ascontiguousarray(c["coefs"], dt),
                np.ascontiguousarray(c["window"], dt)]
        S = getattr(_abi, f"arm_mfcc_instance_{self.kind}")()
        assert r.fn(f"arm_mfcc_init_{self.kind}")(C.byref(S), n, keep[1].size, keep[0].shape[0],
                                                  *[k.ctypes.data for k in keep]) == 0
        _inner = self._patched(S)
        frames = x["frames"][0]
        out = np.zeros((frames.shape[0], keep[0].shape[0]), dt)
        f = r.fn(f"arm_mfcc_{self.kind}")
        for i in range(frames.shape[0]):
            src, tmp = frames[i].copy(), np.zeros(2 * n, np.float32 if self.f32 else np.int32)
            f(C.byref(S), src.ctypes.data, out[i].ctypes.data, tmp.ctypes.data)
        return [{"out": out}], {}

    def launch(self, dsp, torch, T, call):
        cls = {"f32": dsp.MfccF32, "q31": dsp.MfccQ31, "q15": dsp.MfccQ15}[self.kind]
        c = self.cfg
        m = cls(self.n, c["dct"], c["pos"], c["len"], c["coefs"], c["window"])
        _inner = self._patched(m.S)
        m.batch(T["frames"].t, T["out"].t, T["work"].t)


class ConvShared(po.Conv):
    """One template (srcB) for every item: stride 0."""

    def __init__(self, fn, la, lb):
        super().__init__(fn, la, lb)
        self.id += "-shared"
        self.ops[1] = Op("b", self.ops[1].dt, (lb,), "in")

    def inputs(self):
        x = super().inputs()
        return dict(x, b=x["b"][0].copy())

    def expect(self, x):
        return super().expect(dict(x, b=np.stack([np.asarray(x["b"])] * self.batch)))


class Ew(po.Case):
    """An element-wise entry point: ins name -> (dtype, shape); ref(x) -> the dst words; call(dsp, T)."""

    def __init__(self, family, cid, ins, out, ref, call):
        self.ref, self.call = ref, call
        self.f32 = np.dtype(out[0]) == np.float32
        super().__init__(family, cid, [Op(k, dt, sh, "in") for k, (dt, sh) in ins.items()] + [Op("dst", out[0], out[1], "out")])

    def inputs(self):
        rng = np.random.default_rng([len(self.id), 83])
        return {op.name: (rng.uniform(-1, 1, op.shape).astype(np.float32) if op.dt == np.float32 else
                          rng.integers(np.iinfo(op.dt).min, np.iinfo(op.dt).max, op.shape, endpoint=True).astype(op.dt))
                for op in self.ops if op.role == "in"}

    def expect(self, x):
        return [{"dst": np.ascontiguousarray(self.ref(x))}], {}

    def launch(self, dsp, torch, T, call):
        self.call(dsp, T)


# ------------------------------------------------------------------ the table
_even = lambda k, t: t + (t & 1 if k.endswith("q15") else 0)   # noqa: E731

# CFFT: the plain call per type; the twiddle table resident in device memory; q15 at a 2-byte-aligned twiddle address
# (cfft_prepare copies it to an aligned stream-ordered buffer); a user bit-reversal table in device memory
for _k in ("f32", "q31", "q15"):
    _add(po.Cfft(_k, 64, 0, 1, 37), "one launch, generic kernel")
    _add(po.Cfft(_k, 1024, 1, 1, 5), "one launch, specialist kernel")
    _add(po.Cfft(_k, 256, 0, 1, 5, tw=True), "device-resident pTwiddle")
    _add(CfftBitrev(_k, 64, 5), "device-resident pBitRevTable read on the host (device_perm), permutation blob", sync=True,
         fix={"bitrev": lambda v, _k=_k: _bitrev_without(_bitrev_table(_k, 64), 9)})
_add(_retag(po.Cfft("q15", 256, 0, 1, 5, tw=True), "-odd"), "pTwiddle at 2 mod 4: stream-ordered aligned copy", alloc=True,
     offsets={"tw": 1})

# RFFT: arm_rfft_fast_f32 both ways; the fixed real FFT plain and with the caller's device A / B tables
for _ifft in (0, 1):
    _add(po.RfftFast(256, _ifft, False), "inner CFFT + split")
    for _k in ("q31", "q15"):
        _add(po.RfftFixed(_k, 512, _ifft), "radix-16 CFFT with the fused split / merge")
        _add(RfftFixedAB(_k, 1024, _ifft), "device realCoefA / B read on the host (device_split_records)", sync=True)

# FIR: plain (f32 at 5 items: the small kernel; at 37: the chunked one), in place (a stream-ordered copy of the input),
# blockSize < numTaps - 1 (a stream-ordered copy of the history), the MFMA kernels at their floor (tap image)
for _k in ("f32", "q15", "q31", "fast_q15", "fast_q31", "q7"):
    _add(po.Fir(_k, _even(_k, 29), 32), "VALU kernel" if _k != "f32" else "fir_f32_small_kernel")
    _add(InPlace(po.Fir(_k, _even(_k, 29), 32, batch=37)), "src == dst: stream-ordered input copy", alloc=True)
    _add(po.Fir(_k, _even(_k, 29), 8, batch=37), "blockSize < numTaps - 1: stream-ordered history copy", alloc=True)
_add(po.Fir("f32", 130, 2049, batch=37), "chunked f32 pass, a second chunk")
for _k in ("q15", "fast_q15", "q7"):
    _add(po.Fir(_k, 30, 64, batch=256), "MFMA kernel at its floor: stream-ordered tap image", alloc=True)
_add(_retag(po.Fir("q31", 29, 32, batch=256), "-b256"), "q31 MFMA kernel at 256 (item, chunk) pairs: stream-ordered tap image", alloc=True)

# decimate / interpolate through the FIR pass (factor 2) and their own kernels (factor 5: a stream-ordered phase image)
for _fn in ("decimate_f32", "decimate_q15", "decimate_fast_q15", "decimate_q31", "decimate_fast_q31"):
    _add(po.Multirate(_fn, 30, 2, 100), "FIR pass")
    _add(po.Multirate(_fn, 30, 5, 100), "decimator kernel", alloc=_fn != "decimate_f32")
for _fn in ("interpolate_f32", "interpolate_q15", "interpolate_q31"):
    _add(po.Multirate(_fn, 32, 2, 50), "FIR pass")
    _add(po.Multirate(_fn, 30, 5, 50), "interpolator kernels: stream-ordered phase image", alloc=True)
for _k in ("f32", "q31", "q15", "q7"):
    _add(po.Sparse(_k, 16, 20, 100), "device-resident pCoeffs and pTapDelay")

# FIR lattice, IIR lattice, biquad: plain, in place, device-resident coefficients; biquad at 65 stages (two launches)
for _k in ("f32", "q31", "q15"):
    _add(po.Lattice(_k, 8, 100, 5), "device-resident pkCoeffs")
    _add(InPlace(po.Lattice(_k, 8, 100, 37)), "src == dst: stream-ordered state and input copies", alloc=True)
for _f, (_dt, _fam) in adaptive_ref.FUNCS.items():
    if _fam == "iir":
        _add(bc.IirLattice(_f, 5, 8), "host coefficients (content-cached upload)")
        _add(InPlace(bc.IirLattice(_f, 5, 8)), "src == dst")
        _add(IirLatticeDev(_f, 5, 8), "device-resident pkCoeffs / pvCoeffs")
for _f in biquad_ref.FUNCS:
    _add(bc.Biquad(_f, 5, 8), "one launch, host coefficients")
    _add(InPlace(bc.Biquad(_f, 5, 8)), "src == dst exactly: no copy")
    _add(BiquadDev(_f, 5, 8), "device-resident pCoeffs")
_add(bc.Biquad("arm_biquad_cascade_df1_f32", 65, 8), "65 stages: two launches of at most 64 stages")
_add(bc.Biquad("arm_biquad_cascade_df1_q15", 65, 8), "65 stages: two launches of at most 64 stages")
_add(BiquadOverlap("arm_biquad_cascade_df1_f32", 5, 8), "src and dst overlap partly: stream-ordered input copy", alloc=True)

# LMS / normalised LMS at the register, LDS and global tiers; d_out == d_src; the device-resident recipTable
for _f, (_dt, _fam) in adaptive_ref.FUNCS.items():
    if _fam != "iir":
        for _t, _what in ((8, "register tier"), (40, "LDS tier"), (65, "global tier: stream-ordered work area")):
            _add(bc.Lms(_f, _t, 8), _what, alloc=_t == 65)
        _add(InPlace(bc.Lms(_f, 8, 8), dst="out"), "d_out == d_src")
_add(LmsRecip(8, 8), "device-resident recipTable", fix={"recip": lambda v: np.ascontiguousarray(v[::-1])})

# the batched convolution names, per-item and shared templates (f32 conv: a stream-ordered reversed template)
for _fn in list(_abi.CONV_FULL) + list(_abi.CONV_PARTIAL):
    _f32conv = _fn in ("conv_f32", "conv_partial_f32")
    _add(po.Conv(_fn, 50, 7), "per-item template", alloc=_f32conv)
    _add(ConvShared(_fn, 50, 7), "shared template", alloc=_f32conv)

# GEMMs, real and complex, and k == 0
for _k, _s in (("f32", (65, 77, 33)), ("q15", (65, 130, 67)), ("q31", (65, 130, 67)), ("fast_q15", (65, 130, 67)),
               ("fast_q31", (65, 130, 67)), ("q7", (256, 80, 272))):
    _add(po.Gemm(_k, *_s), "one launch, guarded kernel")
for _k in ("f32", "q31", "q15"):
    _add(bc.CmplxGemm(_k, 2, 3, 2), "complex product, one launch")
for _k in ("f32", "q15", "q7"):
    _add(GemmK0(_k, 3, 2), "k == 0: hipMemsetAsync")

# the solves with the status word
for _f in ("inverse", "cholesky", "ldlt", "solve_lower", "solve_upper"):
    _add(bc.Solve(_f, 3), "one launch, per-item status")

# MFCC: host tables (content-cached blob), device-resident tables (read on the host), the three-launch path
for _k in ("f32", "q31", "q15"):
    _add(bc.Mfcc(_k, 256, False, batch=37), "host tables: cached blob, one or two launches")
    _add(MfccDev(_k, 256, 37), "device-resident tables read on the host (host_copy)", sync=True, fix=_MFCC_FIX)
    _add(MfccBitrev(_k, 256, 37), "user bit-reversal table: pre, RFFT / CFFT, post")

# one element-wise, one reduction and one search per vector family
_F = np.float32
_add(bc.Trans("q15", 3, 5, False), "mat_basic: transpose")
_add(bc.VecMult("f32", 3, 5), "mat_basic: matrix x vector")
_add(Ew("mat_basic", "add-f32", {"a": (_F, (37, 3, 5)), "b": (_F, (37, 3, 5))}, (_F, (37, 3, 5)),
        lambda x: mat_basic_ref.add("f32", x["a"], x["b"]), lambda dsp, T: dsp.mat_add_batch(T["a"].t, T["b"].t, T["dst"].t)),
     "mat_basic: element-wise")
_add(Ew("cmplx_math", "mult_cmplx-q15", {"a": (np.int16, (37, 10)), "b": (np.int16, (37, 10))}, (np.int16, (37, 10)),
        lambda x: cmplx_math_ref.mult_cmplx("q15", x["a"], x["b"]),
        lambda dsp, T: dsp.cmplx_mult_cmplx_batch(T["a"].t, T["b"].t, T["dst"].t)), "cmplx_math: element-wise")
_add(bc.Reduce(("cdot", False), "q31", 5), "cmplx_math: reduction")
_add(bc.Reduce(("search", "max"), "q15", 70), "cmplx_math: search")
_add(bc.Reduce(("stat", "mean"), "f32", 70), "statistics: reduction (one wave per item below 4,096 items)")
_add(bc.Reduce(("stat", "mse"), "q15", 70), "statistics: two-source reduction")
_add(bc.Reduce(("stat", "absmax"), "q7", 70), "statistics: search")
_add(Ew("basic_math", "add-q31", {"a": (np.int32, (37, 70)), "b": (np.int32, (37, 70))}, (np.int32, (37, 70)),
        lambda x: basic_math_ref.run("add_q31", x["a"], x["b"])["dst"], lambda dsp, T: dsp.add_batch(T["a"].t, T["b"].t, T["dst"].t)),
     "basic_math: element-wise")
_add(bc.Reduce(("dot", True), "f32", 70), "basic_math: reduction, shared b")
_add(Ew("support", "q15_to_float", {"src": (np.int16, (37, 70))}, (_F, (37, 70)),
        lambda x: support_ref.convert("q15", "f32", x["src"]), lambda dsp, T: dsp.convert_batch(T["src"].t, T["dst"].t)),
     "support: element-wise")
_add(bc.Support("sort", (70,), 1), "sort: one wave per item")
_add(bc.Support("barycenter", (3, 4)), "support: reduction")
_add(bc.Support("weighted_average", (5,)), "support: reduction")
_add(bc.Distance("euclidean", 70, True), "distance: reduction, shared b")
_add(bc.Distance("chebyshev", 5, False), "distance: search")
_add(bc.BoolDistance("yule", 2049), "distance: boolean counts")
_add(bc.DtwDistance(9, 7, 2), "dtw_distance with a device-resident window", fix={"window": lambda v: bc._sakoe(3, *v.shape)})
_add(bc.DtwPath(33, 29), "dtw_path")
_add(bc.FastMath("vexp", 70), "ml: element-wise")
_add(bc.Logdom("logsumexp", 70), "ml: reduction")
_add(bc.Logdom("logsumexp_dot_prod", 70), "logsumexp_dot_prod on the wave kernel (251 items < 4,096)")
for _k in bc.ml_ref.SVM_KINDS:
    _add(bc.Svm(_k, 3, 5), "device-resident model")
_add(bc.Bayes(3, 5), "device-resident model; ml: search (the class index)")

# the cases that may synchronise on the call's stream: a closed set
MAY_SYNC = sorted(cid for cid, sc in CASES.items() if sc.sync)
_ALLOC = [cid for cid, sc in CASES.items() if sc.alloc]


# ------------------------------------------------------------------ building a case
def _per_call(v, k):
    return v[k] if isinstance(v, list) else v


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _decoy_of(sc, name, true, seeded):
    """The decoy of one operand (one array): the chosen table, the reseeded words, or (where no seed reaches the
    operand and any words are valid) the true words rotated by one."""
    if name in sc.fix:
        return np.ascontiguousarray(sc.fix[name](np.asarray(true)))
    if true.size and _same(true, seeded):
        assert name in _ROLL, f"{sc.id}: operand {name} has no decoy (add a fix: another valid table)"
        return np.roll(true.reshape(-1), 1).reshape(true.shape)
    return seeded


@functools.lru_cache(maxsize=None)
def _built(cid):
    """(true inputs, expected words per call, after the last call, decoy inputs), once per case."""
    sc = CASES.get(cid) or _TOYS[cid]
    x = sc.case.inputs()
    calls, final = sc.case.expect(x)
    with _reseeded():
        seeded = sc.case.inputs()
    decoy = {}
    for name, v in x.items():
        if isinstance(v, list):
            decoy[name] = [_decoy_of(sc, name, a, b) for a, b in zip(v, seeded[name])]
        else:
            decoy[name] = _decoy_of(sc, name, v, seeded[name])
    return x, calls, final, decoy


@functools.lru_cache(maxsize=None)
def _twin(cid):
    """The reference words of the decoy-seeded twin of a case."""
    sc = CASES[cid]
    return sc.case.expect(_built(cid)[3])


def _state_decoy(op):
    rng = np.random.default_rng([SALT, len(op.name), int(np.prod(op.shape))])
    if op.dt == np.float32:
        return rng.uniform(-1, 1, op.shape).astype(np.float32)
    i = np.iinfo(op.dt)
    return rng.integers(i.min, i.max, op.shape, endpoint=True).astype(op.dt)


# ------------------------------------------------------------------ the runner
def _dev(torch, arr, op):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=op.dt).reshape(op.shape).copy()).cuda()


def _alloc(sc, torch):
    return {op.name: Padded(torch, op.dt, op.shape, sc.offsets.get(op.name, 0), po._op_fill(op, FILL_A)) for op in sc.case.ops}


def _region(p, bits):
    """The operand's words inside a snapshot of p's whole buffer, as a device tensor of the operand's type and shape."""
    return bits.view(p.flat.dtype)[p.lo:p.hi].view(p.shape)


def _snapshot_words(p, bits):
    h = bits.cpu().numpy()
    return h[p.lo:p.hi].view(p.dt).reshape(p.shape).copy()


class _Staged:
    """The device copies of one input set: words(op, k, carried) -> the tensor operand `op` must hold for call k."""

    def __init__(self, torch, case, x, state_words):
        self.case, self.t = case, {}
        for op in case.ops:
            if op.name in x:
                v = x[op.name]
                self.t[op.name] = [_dev(torch, a, op) for a in v] if isinstance(v, list) else _dev(torch, v, op)
            elif op.role == "state":
                self.t[op.name] = _dev(torch, state_words(op), op)

    def words(self, op, k, carried=None):
        v = self.t[op.name]
        if isinstance(v, list):
            return v[k]
        if k and carried is not None and op.role in ("io", "state"):
            return carried[op.name]
        return v


def _late_ops(case):
    return [op for op in case.ops if op.role in ("in", "io", "state") and int(np.prod(op.shape))]


def _compare(case, T, snaps, want_sets, k, bad, tag=""):
    for name, want in want_sets:
        got = _snapshot_words(T[name], snaps[name])
        msg = po._diff(case, got, want, T[name].word)
        if msg:
            bad.append(f"{tag}call {k} {name}: {msg}")


def _run(sc, dsp, torch, streams):
    """One case through the protocol of the module docstring on the module's qualified side stream; raises with every
    failure in one message."""
    case = sc.case
    x, calls, final, decoy = _built(sc.id)
    late = _late_ops(case)
    outs = [op for op in case.ops if op.role == "out"]
    kept = [op for op in case.ops if op.role != "in"]
    true_w = _Staged(torch, case, x, lambda op: np.zeros(op.shape, op.dt))
    decoy_w = _Staged(torch, case, decoy, _state_decoy)
    T, W = _alloc(sc, torch), _alloc(sc, torch)
    side, delay = streams.side, streams.delay
    bad, carried = [], None
    for k in range(case.ncalls):
        for op in late:
            T[op.name].t.copy_(decoy_w.words(op, k))
        for op in outs:
            T[op.name].reset()
        snaps = {op.name: torch.empty_like(T[op.name]._bits) for op in kept}
        if k == 0:                              # the warm-up: separate buffers, true words, the default stream
            for op in late:
                W[op.name].t.copy_(true_w.words(op, 0))
            case.launch(dsp, torch, W, 0)
        torch.cuda.synchronize()
        if dsp is not None:
            dsp.lib.arm_mi355x_clear_error()
        raised = None
        with torch.cuda.stream(side):
            torch.cuda._sleep(delay)
            for op in late:
                T[op.name].t.copy_(true_w.words(op, k, carried), non_blocking=True)
            t0 = time.perf_counter()
            try:
                case.launch(dsp, torch, T, k)
            except (RuntimeError, AssertionError, ValueError) as e:
                raised = e
            ms = (time.perf_counter() - t0) * 1e3
            busy = not side.query()
            for op in kept:
                snaps[op.name].copy_(T[op.name]._bits, non_blocking=True)
            for op in late:
                T[op.name].t.copy_(decoy_w.words(op, k), non_blocking=True)
            for op in outs:
                T[op.name].reset()
        torch.cuda.synchronize()
        if ms > _SEEN["launch_ms"] and sc.id in CASES and not sc.sync:
            _SEEN["launch_ms"], _SEEN["case"] = ms, sc.id
        if raised is not None:
            bad.append(f"call {k}: launch raised {raised!r}")
        if dsp is not None and dsp.last_error()[0]:
            bad.append(f"call {k}: error recorded: {dsp.last_error()}")
        # a call that waits for the stream and then launches leaves the stream busy with its own launch, so query()
        # alone would pass it: the host must also be back long before the delay can have ended
        if not sc.sync and (not busy or ms >= SLEEP_MS / 2):
            bad.append(f"call {k}: launch() returned after {ms:.2f} ms with the side stream {'busy' if busy else 'idle'}: "
                       "the call synchronised with the host (or the delay was too short, or the host itself stalled)")
        _compare(case, T, snaps, list(calls[k].items()) + (list(final.items()) if k == case.ncalls - 1 else []), k, bad)
        carried = {op.name: _region(T[op.name], snaps[op.name]) for op in kept}
    for op in case.ops:
        if not T[op.name].fetch()[1]:
            bad.append(f"{op.name}: guard words written")
    assert not bad, f"{sc.id} ({sc.note}): {len(bad)} failures:\n" + "\n".join(bad[:12])


def _run_pair(sc, dsp, torch, streams):
    """The case and its decoy-seeded twin on two side streams from one thread, enqueued alternately behind one delay
    each: operands late-written on their own stream, both must give their own reference words."""
    case = sc.case
    x, calls, final, decoy = _built(sc.id)
    sets = [(x, calls, final), (decoy,) + tuple(_twin(sc.id))]
    late = _late_ops(case)
    outs = [op for op in case.ops if op.role == "out"]
    kept = [op for op in case.ops if op.role != "in"]
    zeros = lambda op: np.zeros(op.shape, op.dt)   # noqa: E731
    own = [_Staged(torch, case, s[0], zeros) for s in sets]
    other = [_Staged(torch, case, sets[1 - i][0], _state_decoy) for i in range(2)]
    T = [_alloc(sc, torch), _alloc(sc, torch)]
    W = _alloc(sc, torch)
    sides, delay = [streams.side, streams.twin], streams.delay
    snaps = [[{op.name: torch.empty_like(T[i][op.name]._bits) for op in kept} for _ in range(case.ncalls)] for i in range(2)]
    for i in range(2):
        for op in late:                         # every operand starts with the other stream's words
            T[i][op.name].t.copy_(other[i].words(op, 0))
    for op in late:
        W[op.name].t.copy_(own[0].words(op, 0))
    case.launch(dsp, torch, W, 0)
    torch.cuda.synchronize()
    dsp.lib.arm_mi355x_clear_error()
    bad = []
    for i in range(2):
        with torch.cuda.stream(sides[i]):
            torch.cuda._sleep(delay)
    for k in range(case.ncalls):
        for i in range(2):
            with torch.cuda.stream(sides[i]):
                for op in late:
                    if k == 0 or isinstance(own[i].t[op.name], list):
                        T[i][op.name].t.copy_(own[i].words(op, k), non_blocking=True)
                for op in outs:
                    T[i][op.name].reset()
                try:
                    case.launch(dsp, torch, T[i], k)
                except (RuntimeError, AssertionError, ValueError) as e:
                    bad.append(f"stream {i} call {k}: launch raised {e!r}")
                for op in kept:
                    snaps[i][k][op.name].copy_(T[i][op.name]._bits, non_blocking=True)
    torch.cuda.synchronize()
    if dsp.last_error()[0]:
        bad.append(f"error recorded: {dsp.last_error()}")
    for i in range(2):
        _, c, f = sets[i]
        for k in range(case.ncalls):
            _compare(case, T[i], snaps[i][k], list(c[k].items()) + (list(f.items()) if k == case.ncalls - 1 else []), k, bad,
                     tag=f"stream {i} ({'case' if i == 0 else 'twin'}) ")
        for op in case.ops:
            if not T[i][op.name].fetch()[1]:
                bad.append(f"stream {i} {op.name}: guard words written")
    assert not bad, f"{sc.id} ({sc.note}): {len(bad)} failures:\n" + "\n".join(bad[:12])


def _calibrate(torch):
    """The torch.cuda._sleep argument of SLEEP_MS, from one timed probe between two events."""
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    probe = 20_000_000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(probe)
    e1.record()
    torch.cuda.synchronize()
    per_ms = probe / e0.elapsed_time(e1)
    _SEEN["cycles_per_ms"] = per_ms
    return int(SLEEP_MS * per_ms)


def _runs_ahead(torch, sleeper, others, delay):
    """True if a small operation enqueued on each of `others` (None: the null stream) after `sleeper` began its delay
    completes while `sleeper` is still busy: work misplaced on those streams really overtakes the delayed stream
    (streams can share a hardware queue, and then it would wait behind the delay and read the true words)."""
    probes = [torch.zeros(16, device="cuda") for _ in others]
    torch.cuda.synchronize()
    with torch.cuda.stream(sleeper):
        torch.cuda._sleep(delay)
    events = []
    for s, p in zip(others, probes):
        with torch.cuda.stream(torch.cuda.default_stream() if s is None else s):
            p.add_(1)
            e = torch.cuda.Event()
            e.record()
            events.append(e)
    deadline = time.perf_counter() + SLEEP_MS / 2e3
    while time.perf_counter() < deadline and not all(e.query() for e in events):
        pass
    ok = all(e.query() for e in events) and not sleeper.query()
    torch.cuda.synchronize()
    return ok


class _Streams:
    """The streams every case, the two-stream pair and the negative controls use: side (the caller's delayed stream),
    twin (the pair's second stream) and third (where the controls misplace work)."""


@pytest.fixture(scope="module")
def streams(torch_gpu):
    """One set of streams for the whole module, shown to be independent before use: while side sleeps, work on the null
    stream, on third and on twin completes; while twin sleeps, work on the null stream and on side completes.  A
    candidate that fails is dropped and the next stream of torch's pool tried; the test fails if none qualifies.  At
    the end the calibration and the longest host-side launch() (the MAY_SYNC cases aside) are printed."""
    torch = torch_gpu
    st = _Streams()
    st.delay = _calibrate(torch)
    st.third = torch.cuda.Stream()
    dropped = []

    def draw(ok):
        for _ in range(64):
            s = torch.cuda.Stream()
            if ok(s):
                return s
            dropped.append(s)
        pytest.fail(f"no stream independent of the null stream and of each other among 64 candidates ({len(dropped)} dropped)")
    st.side = draw(lambda s: _runs_ahead(torch, s, [None, st.third], st.delay))
    st.twin = draw(lambda s: _runs_ahead(torch, s, [None, st.side], st.delay) and
                   _runs_ahead(torch, st.side, [None, st.third, s], st.delay))
    st.dropped = len(dropped)
    Toy.third = st.third
    yield st
    print(f"\nstream-order figures: sleep cycles per ms = {_SEEN['cycles_per_ms']:.0f}, delay = {st.delay} cycles "
          f"({SLEEP_MS} ms), candidate streams dropped = {st.dropped}, longest launch() = {_SEEN['launch_ms']:.3f} ms "
          f"({_SEEN['case']})")


def _skip_unless_assessable(case):
    if getattr(case, "libm", False) and not bc._host_libm_ok():
        pytest.skip("host libm differs: the restatement's words are another expf's / logf's")


_FAMILIES = sorted({sc.family for sc in CASES.values()})


def _ids(family):
    return [cid for cid, sc in CASES.items() if sc.family == family]


def _family_test(family):
    @pytest.mark.gpu
    @pytest.mark.parametrize("cid", _ids(family))
    def test(dsp, torch_gpu, streams, cid):
        sc = CASES[cid]
        _skip_unless_assessable(sc.case)
        _run(sc, dsp, torch_gpu, streams)
        if sc.case.compare == "mfcc_f32" and not po.mfcc_cfg.host_libm_status()[0]:
            pytest.skip("host libm differs: suite tolerance checked, bit-exactness not assessable on this host")
    test.__name__ = test.__qualname__ = f"test_{family}_stream_order"
    test.__doc__ = f"Every case of the {family} rows behind a delayed side stream: see the module docstring."
    return test


for _f in _FAMILIES:
    globals()[f"test_{_f}_stream_order"] = _family_test(_f)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _ALLOC)
def test_two_streams_with_stream_ordered_temporaries(dsp, torch_gpu, streams, cid):
    """The cases whose call allocates a stream-ordered temporary, together with their decoy-seeded twin on two side
    streams: see the module docstring."""
    _skip_unless_assessable(CASES[cid].case)
    _run_pair(CASES[cid], dsp, torch_gpu, streams)


# ------------------------------------------------------------------ the runner's negative controls, on the GPU
class Toy(po.Case):
    """dst = src, a device-to-device copy, with one planted ordering defect."""
    f32 = False

    def __init__(self, defect):
        self.defect = defect
        super().__init__("toy", defect, [Op("src", np.int32, (3, 10), "in"), Op("dst", np.int32, (3, 10), "out")])

    def inputs(self):
        return {"src": po._rand("q31", (3, 10), np.random.default_rng(5))}

    def expect(self, x):
        return [{"dst": np.asarray(x["src"]).copy()}], {}

    def launch(self, dsp, torch, T, call):
        cur = torch.cuda.current_stream()
        if self.defect == "default_stream" and cur != torch.cuda.default_stream():
            with torch.cuda.stream(torch.cuda.default_stream()):
                T["dst"].t.copy_(T["src"].t, non_blocking=True)
            return
        if self.defect == "third_stream" and cur != torch.cuda.default_stream():
            with torch.cuda.stream(self.third):
                T["dst"].t.copy_(T["src"].t, non_blocking=True)
            return
        if self.defect == "host_sync":
            cur.synchronize()
        T["dst"].t.copy_(T["src"].t, non_blocking=True)


for _d in ("none", "default_stream", "third_stream", "host_sync"):
    _TOYS[f"toy-{_d}"] = SCase(Toy(_d), "toy")


@pytest.mark.gpu
def test_runner_reports_planted_ordering_defects(torch_gpu, streams):
    """On the very streams the cases use: a clean toy passes.  A copy put on the default stream, or on the third stream
    without an event wait, reads the stale words and is reported as differing words; a correct copy behind a host
    synchronisation of the call's stream is reported by the no-host-synchronisation check alone (its own copy keeps
    the stream busy when query() is read: the host time of launch() gives it away)."""
    torch = torch_gpu
    _run(_TOYS["toy-none"], None, torch, streams)
    for defect in ("default_stream", "third_stream"):
        with pytest.raises(AssertionError, match="words differ"):
            _run(_TOYS[f"toy-{defect}"], None, torch, streams)
    with pytest.raises(AssertionError, match="synchronised with the host") as e:
        _run(_TOYS["toy-host_sync"], None, torch, streams)
    assert "words differ" not in str(e.value)
    torch.cuda.synchronize()


_STATEFUL = [cid for cid, sc in CASES.items() if any(op.role == "state" for op in sc.case.ops)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", _STATEFUL)
def test_stale_start_state_is_visible(dsp, torch_gpu, cid):
    """expect() starts a role-"state" operand at zero and cannot take another start, so the CPU proof of
    test_stale_operand_is_visible does not reach it.  Here the first call runs, synchronised on the default stream,
    on the true inputs with the state operands holding their decoy: an output (not a state) word must differ from the
    reference, so a stale read of the start state shows in the stream-order run."""
    torch = torch_gpu
    sc = CASES[cid]
    case = sc.case
    _skip_unless_assessable(case)
    x, calls, final, _ = _built(cid)
    true_w = _Staged(torch, case, x, _state_decoy)
    T = _alloc(sc, torch)
    for op in _late_ops(case):
        T[op.name].t.copy_(true_w.words(op, 0))
    case.launch(dsp, torch, T, 0)
    torch.cuda.synchronize()
    roles = {op.name: op.role for op in case.ops}
    outs = [(name, want) for name, want in calls[0].items() if roles[name] != "state"]
    assert outs and any(po._diff(case, T[name].fetch()[0], want, T[name].word) for name, want in outs), \
        f"{cid}: the decoy start state gives the reference's output words"


# ------------------------------------------------------------------ the table, on the CPU
def test_may_sync_is_a_closed_set():
    """The cases that may wait for the call's stream: device-resident MFCC tables, the fixed real FFT with the caller's
    device A / B tables, a device-resident user bit-reversal table.  Anything else that synchronises is a defect."""
    assert MAY_SYNC == sorted(
        [f"cfft-{k}-64-ifft0-brev1-devbitrev" for k in ("f32", "q31", "q15")] +
        [f"mfcc-{k}-256-work-devtables" for k in ("f32", "q31", "q15")] +
        [f"rfft_fixed-{k}-1024-ifft{i}-devAB" for k in ("q31", "q15") for i in (0, 1)])


@pytest.mark.parametrize("family", _FAMILIES)
def test_case_table_builds(family):
    """Every case builds its true words, reference and decoy; the decoy has the operands' shapes and types and differs
    from the true words in every operand of non-zero size."""
    for cid in _ids(family):
        sc = CASES[cid]
        x, calls, final, decoy = _built(cid)
        names = {op.name: op for op in sc.case.ops}
        assert len(calls) == sc.case.ncalls and set(decoy) == set(x), cid
        assert set(sc.fix) <= set(x) and set(sc.offsets) <= set(names), cid
        for op in sc.case.ops:
            assert (op.name in x) == (op.role in ("in", "io")), (cid, op.name)
        for name, v in x.items():
            for k in range(len(v) if isinstance(v, list) else 1):
                a, d = np.asarray(_per_call(v, k)), np.asarray(_per_call(decoy[name], k))
                assert a.shape == d.shape == names[name].shape and a.dtype == d.dtype == names[name].dt, (cid, name)
                assert not a.size or not _same(a, d), (cid, name, "the decoy is the true words")
        for d in calls + [final]:
            for name, w in d.items():
                w = w[0] if isinstance(w, tuple) else w
                assert w.shape == names[name].shape and w.dtype == names[name].dt, (cid, name, w.shape, w.dtype)
        if sc.alloc:
            assert len(_twin(cid)[0]) == sc.case.ncalls


def _words_of(calls, final):
    out = []
    for d in calls + [final]:
        for name in sorted(d):
            w = d[name]
            out.append(np.ascontiguousarray(w[0] if isinstance(w, tuple) else w).tobytes())
            if isinstance(w, tuple):
                out.append(np.ascontiguousarray(w[1]).tobytes())
    return out


@pytest.mark.parametrize("family", _FAMILIES)
def test_stale_operand_is_visible(family):
    """For every late-written operand that inputs() names, expect() with that operand alone replaced by its decoy
    differs from the true reference in an output word: a stale read of it shows."""
    for cid in _ids(family):
        sc = CASES[cid]
        x, calls, final, decoy = _built(cid)
        want = _words_of(calls, final)
        for name, v in x.items():
            if not np.asarray(_per_call(v, 0)).size:
                continue
            got = sc.case.expect(dict(x, **{name: decoy[name]}))
            assert _words_of(*got) != want, f"{cid}: a stale {name} would not show"
