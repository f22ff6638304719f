"""The reference's own suites (tests/suite_replay.py) replayed against the GPU library.

One case per test method of a suite, its `Test` lines looped inside.  The library is cmsisdsp_amd's drop-ins, called
through ctypes on host buffers exactly as the suite calls arm_math.h.  Every row must pass the suite's own thresholds
against the double-precision pattern, give the words the reference build gave for that row (<row>/ref_words) and leave
the output's tail alone.  The Basic, Stats, BIQUAD, FIR, DECIM, MISC, Transform and MFCC suites run every row a second
time through the _batch form on device buffers, as a batch of three copies of the row: every item must equal the
drop-in's words, a const source must be unchanged and the marker words behind the batch intact."""
import ctypes as C
import types

import numpy as np
import pytest

import basic_math_ref as br
import biquad_ref as bq
import suite_replay as sr

ITEMS = 3


def dropins(dsp):
    def after(name):
        assert dsp.last_error()[0] == 0, (name, dsp.last_error())
    return sr.CtypesLibrary(dsp.lib, dsp._abi, after)


def _up(torch, x, n):
    """ITEMS copies of the first n words of x, one after the other on the device."""
    return torch.from_numpy(np.tile(x[:n], (ITEMS, 1)).view(np.uint8)).cuda()


def _results(torch, t, m):
    """A marked device buffer for ITEMS results of m words of type t, TAIL marker words behind them."""
    return torch.from_numpy(br.marked(t, ITEMS * m + sr.TAIL).view(np.uint8)).cuda()


def _items(name, dev, t, m):
    """The ITEMS results, after checking the words behind them and that the items agree -> the first."""
    got = dev.cpu().numpy().view(br.MDT[t])
    assert got[ITEMS * m:].tobytes() == br.marked(t, sr.TAIL).tobytes(), (name, "words after the batch")
    items = got[:ITEMS * m].reshape(ITEMS, m)
    for k in range(1, ITEMS):
        assert items[k].tobytes() == items[0].tobytes(), (name, "item", k)
    return items[0]


class BasicBatch:
    """arm_<func> of the basic math family served by arm_<func>_batch on device buffers: ITEMS copies of the operands,
    the items' outputs one after the other and TAIL marker words behind the last.  The items must agree among
    themselves; the first is handed back."""

    def __init__(self, dsp, torch):
        self.dsp, self.torch = dsp, torch

    def __getattr__(self, name):
        func = name[len("arm_"):]
        fn = getattr(self.dsp.lib, name + "_batch")
        torch = self.torch

        def call(*args):
            a, b, scalars, out, n = sr.basic_args(func, args)
            srcs = [x for x in (a, b) if x is not None]
            dev = [_up(torch, x, n) for x in srcs]
            rt, m = br.result_type(func), (1 if br.is_dot(func) else n)
            dout = _results(torch, rt, m)
            ptrs = [d.data_ptr() for d in dev]
            if br.is_dot(func):
                st = fn(*ptrs, n, n, dout.data_ptr(), ITEMS, None)
            elif br.split(func)[0] == "clip":
                st = fn(*ptrs, dout.data_ptr(), *scalars, n, ITEMS, None)
            else:
                st = fn(*ptrs, *scalars, dout.data_ptr(), n, ITEMS, None)
            torch.cuda.synchronize()
            assert st == 0, (name, st, self.dsp.last_error())
            for d, x in zip(dev, srcs):
                assert d.cpu().numpy().tobytes() == np.tile(x[:n], (ITEMS, 1)).tobytes(), (name, "a source changed")
            out[:m] = _items(name, dout, rt, m)
        return call


class StatsBatch:
    """The statistics, max / min and log-domain functions served by their _batch forms (see BasicBatch)."""

    def __init__(self, dsp, torch):
        self.dsp, self.torch = dsp, torch

    def __getattr__(self, name):
        func = name[len("arm_"):]
        op, t = func.rsplit("_", 1)
        fn = getattr(self.dsp.lib, name + "_batch")
        torch = self.torch

        def call(*args):
            two = op in ("mse", "kullback_leibler", "logsumexp_dot_prod")
            n = args[2 if two else 1]
            srcs = [_up(torch, x, n) for x in args[:2 if two else 1]]
            ptrs = [d.data_ptr() for d in srcs]
            rt = "f32" if op in sr.LOGDOM else sr.stat_result_type(func)
            res = _results(torch, rt, 1)
            idx = _results(torch, "u32", 1) if op in sr.INDEXED else None
            if op in ("kullback_leibler", "logsumexp_dot_prod"):
                st = fn(*ptrs, n, n, res.data_ptr(), ITEMS, None)          # bStride = n: every item its own b
            elif idx is not None:
                st = fn(*ptrs, n, res.data_ptr(), idx.data_ptr(), ITEMS, None)
            else:
                st = fn(*ptrs, n, res.data_ptr(), ITEMS, None)
            torch.cuda.synchronize()
            assert st == 0, (name, st, self.dsp.last_error())
            for d, x in zip(srcs, args):
                assert d.cpu().numpy().tobytes() == np.tile(x[:n], (ITEMS, 1)).tobytes(), (name, "a source changed")
            value = _items(name, res, rt, 1)
            if op in sr.LOGDOM:
                return float(value[0])
            args[3 if op == "mse" else 2][0] = value[0]
            if idx is not None:
                args[3][0] = _items(name, idx, "u32", 1)[0]
        return call


class BiquadBatch:
    """The biquad cascades served by arm_<func>_batch: ITEMS streams of the same samples, their states [ITEMS, words]
    on the device, carried from call to call; the coefficients stay on the host, as the instance has them.  The first
    stream's output and state are handed back."""

    def __init__(self, dsp, torch):
        self.dsp, self.torch = dsp, torch

    def instance(self, func):
        return types.SimpleNamespace(func=func)

    def __getattr__(self, name):
        torch, abi = self.torch, self.dsp._abi
        if "_init_" in name:
            def init(S, stages, coeffs, state, post_shift=0):
                dt, sdt, ks, nc, ch = bq.FUNCS[S.func]
                S.stages, S.coeffs, S.post_shift, S.host = stages, coeffs, post_shift, state[:ks * stages]
                S.host[:] = 0                                # the init zeroes the state
                S.state = torch.from_numpy(np.zeros((ITEMS, S.host.size), dtype=sdt).view(np.uint8)).cuda()
            return init
        fn = getattr(self.dsp.lib, name + "_batch")

        def call(S, src, dst, n):
            dt, sdt, ks, nc, ch = bq.FUNCS[name]
            inst = abi.BIQUAD_FUNCS[name][0]
            kw = {"postShift": S.post_shift} if any(f == "postShift" for f, _ in inst._fields_) else {}
            c = inst(numStages=S.stages, pState=None, pCoeffs=C.cast(S.coeffs.ctypes.data, dict(inst._fields_)["pCoeffs"]),
                     **kw)
            t = {np.float32: "f32", np.int32: "q31", np.int16: "q15"}[dt]
            x = _up(torch, src, ch * n)
            y = _results(torch, t, ch * n)
            st = fn(C.byref(c), x.data_ptr(), y.data_ptr(), n, ITEMS, S.state.data_ptr(), None)
            torch.cuda.synchronize()
            assert st == 0, (name, st, self.dsp.last_error())
            assert x.cpu().numpy().tobytes() == np.tile(src[:ch * n], (ITEMS, 1)).tobytes(), (name, "the source changed")
            dst[:ch * n] = _items(name, y, t, ch * n)
            states = S.state.cpu().numpy().view(sdt).reshape(ITEMS, -1)
            for k in range(1, ITEMS):
                assert states[k].tobytes() == states[0].tobytes(), (name, "state of item", k)
            S.host[:] = states[0]
        return call


TYPE_OF = {np.dtype(np.float32): "f32", np.dtype(np.int32): "q31", np.dtype(np.int16): "q15", np.dtype(np.int8): "q7"}


def _host_words(pointer, n, dtype):
    """n words at a pointer member of an instance structure (its pState)."""
    addr = C.cast(pointer, C.c_void_p).value
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype).copy()


def _up_onto(torch, t, words):
    """ITEMS copies of words (what the caller's output buffer holds before the call), TAIL marker words behind."""
    return torch.from_numpy(np.concatenate([np.tile(words, ITEMS), br.marked(t, sr.TAIL)]).view(np.uint8)).cuda()


class FirBatch:
    """arm_fir_* / arm_fir_decimate_* / arm_fir_interpolate_* served twice per call: by the drop-in on the suite's host
    buffers (the instance, its coefficients and its state are the drop-in's), and by arm_<func>_batch on ITEMS device
    copies of the block.  The per-item history [ITEMS, numTaps - 1] (interpolator: phaseLength - 1) lives on the
    device, is zeroed where the suite inits the filter and carried across the suite's two calls.  After every call
    the three items' outputs and histories must agree and equal the drop-in's output and the head of its state."""

    def __init__(self, dsp, torch):
        self.dsp, self.torch, self.host, self.hist = dsp, torch, dropins(dsp), None

    def instance(self, func):
        return self.host.instance(func)

    def __getattr__(self, name):
        host, torch = getattr(self.host, name), self.torch
        if "_init_" in name:
            def init(S, *args):
                self.hist = None                             # arm_fir_init_*: a new stream
                return host(S, *args)
            return init
        fn = getattr(self.dsp.lib, name + "_batch")

        def call(S, src, dst, n):
            t = TYPE_OF[src.dtype]
            if "decimate" in name:
                m, words = n // S.M, S.numTaps - 1
            elif "interpolate" in name:
                m, words = n * S.L, S.phaseLength - 1
            else:
                m, words = n, S.numTaps - 1
            if self.hist is None:                            # at least a word, so that the pointer is one
                self.hist = torch.zeros(ITEMS * max(words, 1) * src.itemsize, dtype=torch.uint8, device="cuda")
            host(S, src, dst, n)
            x, y = _up(torch, src, n), _results(torch, t, m)
            st = fn(C.byref(S), x.data_ptr(), y.data_ptr(), n, ITEMS, self.hist.data_ptr(), None)
            torch.cuda.synchronize()
            assert st == 0, (name, st, self.dsp.last_error())
            assert x.cpu().numpy().tobytes() == np.tile(src[:n], (ITEMS, 1)).tobytes(), (name, "the source changed")
            sr.same_words(_items(name, y, t, m), dst[:m], (name, n, "the _batch form against the drop-in"))
            if words:
                hist = self.hist.cpu().numpy().view(src.dtype).reshape(ITEMS, words)
                for k in range(1, ITEMS):
                    assert hist[k].tobytes() == hist[0].tobytes(), (name, "history of item", k)
                sr.same_words(hist[0], _host_words(S.pState, words, src.dtype), (name, n, "the history against the state"))
        return call


class ConvBatch:
    """arm_conv_* / arm_correlate_* / arm_conv_partial_* served by arm_<func>_batch: ITEMS pairs of the row's
    operands, every item with its own pSrcB.  The full forms write each item over a copy of what the suite's output
    held (the words a correlation leaves alone must stay); the partial forms write numPoints words per item,
    compactly.  The scratch-buffer (opt) forms have no batched form."""

    def __init__(self, dsp, torch):
        self.dsp, self.torch = dsp, torch

    def __getattr__(self, name):
        fn = getattr(self.dsp.lib, name + "_batch")
        torch = self.torch

        def call(a, la, b, lb, dst, first=None, num=None):
            t = TYPE_OF[dst.dtype]
            da, db = _up(torch, a, la), _up(torch, b, lb)
            if first is None:
                m = 2 * max(la, lb) - 1 if "correlate" in name else la + lb - 1
                assert dst.size == m, (name, dst.size, m)
                y = _up_onto(torch, t, dst)
                st = fn(da.data_ptr(), la, la, db.data_ptr(), lb, lb, y.data_ptr(), ITEMS, None)
            else:
                m = num
                y = _results(torch, t, m)
                st = fn(da.data_ptr(), la, la, db.data_ptr(), lb, lb, y.data_ptr(), first, num, ITEMS, None)
            torch.cuda.synchronize()
            assert st == 0, (name, st, self.dsp.last_error())
            for d, x, n in ((da, a, la), (db, b, lb)):
                assert d.cpu().numpy().tobytes() == np.tile(x[:n], (ITEMS, 1)).tobytes(), (name, "a source changed")
            got = _items(name, y, t, m)
            if first is None:
                dst[:] = got
            else:
                dst[first:first + num] = got
                return 0
        return call


class TransformBatch:
    """arm_cfft_* / arm_rfft_* / arm_mfcc_* served by their _batch forms on ITEMS device copies of the row, in place
    where the suite is in place; the instances come from the drop-ins' init functions, their tables stay on the host."""

    def __init__(self, dsp, torch):
        self.dsp, self.torch, self.host = dsp, torch, dropins(dsp)

    def instance(self, func):
        return self.host.instance(func)

    def _run(self, name, *args):
        st = getattr(self.dsp.lib, name + "_batch")(*args)
        self.torch.cuda.synchronize()
        assert st == 0, (name, st, self.dsp.last_error())

    def _in_place(self, p, n):
        """ITEMS copies of the first n words of p, marker words behind; back(): the agreeing items -> p[:n]."""
        t = TYPE_OF[p.dtype]
        dev = _up_onto(self.torch, t, p[:n])
        return dev, lambda name: p.__setitem__(slice(0, n), _items(name, dev, t, n))

    def __getattr__(self, name):
        if "_init_" in name:
            return getattr(self.host, name)
        torch = self.torch

        def cfft(S, p, ifft, bitrev):
            dev, back = self._in_place(p, 2 * S.fftLen)
            self._run(name, C.byref(S), dev.data_ptr(), ITEMS, ifft, bitrev, None)
            back(name)

        def rfft_fast(S, p, out, ifft):
            n = S.fftLenRFFT
            dev, back = self._in_place(p, n)
            res, back_out = self._in_place(out, n)
            self._run(name, C.byref(S), dev.data_ptr(), res.data_ptr(), ITEMS, ifft, None)
            back(name), back_out(name)

        def rfft_fixed(S, src, dst):
            n = S.fftLenReal
            inverse = S.ifftFlagR == 1
            dev, back = self._in_place(src, 2 * n if inverse else n)
            res, back_out = self._in_place(dst, n if inverse else 2 * n)
            self._run(name, C.byref(S), dev.data_ptr(), res.data_ptr(), ITEMS, None)
            back(name), back_out(name)

        def mfcc(S, src, dst, tmp):
            n, t = S.fftLen, TYPE_OF[src.dtype]
            dev, _ = self._in_place(src, n)
            res, back_out = self._in_place(dst, S.nbDctOutputs)
            work = {"f32": n * 4, "q31": 2 * n * 4, "q15": 2 * n * 2}[t]        # arm_math_mi355x.h: d_tmp per frame
            scratch = torch.zeros(ITEMS * work + 64, dtype=torch.uint8, device="cuda")
            self._run(name, C.byref(S), dev.data_ptr(), res.data_ptr(), scratch.data_ptr(), ITEMS, None)
            _items(name, dev, t, n)                          # the frames are work space: the items agree, the tail stays
            back_out(name)
            return 0

        if name.startswith("arm_cfft_"):
            return cfft
        if name == "arm_rfft_fast_f32":
            return rfft_fast
        return rfft_fixed if name.startswith("arm_rfft_") else mfcc


BATCH = {"basic": BasicBatch, "stats": StatsBatch, "biquad": BiquadBatch, "fir": FirBatch, "decim": FirBatch,
         "misc": ConvBatch, "transform_c": TransformBatch, "transform_r": TransformBatch, "mfcc": TransformBatch}


@pytest.mark.gpu
@pytest.mark.parametrize("suite,method", sr.methods(), ids=lambda v: v)
def test_suite_method_on_the_gpu(dsp, torch_gpu, suite, method):
    lib = dropins(dsp)
    batch = BATCH.get(sr.FAMILIES[suite])
    for row in (r for r in sr.ROWS if (r.suite, r.method) == (suite, method)):
        pats = sr.patterns(row)
        outs, failed = sr.run_row(row, lib, pats)
        assert not failed, (row.id, row.cite, failed)
        for name, words in outs.items():
            if row.exact and name not in sr.SCRATCH:
                sr.same_words(words, pats[sr.ref_key(row, name)], (row.id, name))
        if row.func in sr.RESTATED:                          # the k-ordered fmaf chain's words (oracle/src)
            want, _ = sr.run_row(row, sr.RestatementLibrary(), pats)
            sr.same_words(outs["output"], want["output"], (row.id, "the fmaf chain"))
        if batch is ConvBatch and not hasattr(dsp.lib, row.func + "_batch"):
            continue                                         # the scratch-buffer forms: drop-in only
        if batch:
            again, failed = sr.run_row(row, batch(dsp, torch_gpu), pats)
            assert not failed, (row.id, "batch", failed)
            for k, v in outs.items():
                if k not in sr.SCRATCH:
                    sr.same_words(again[k], v, (row.id, "the _batch form against the drop-in"))
