"""The reference's own suites (tests/suite_replay.py) replayed against the GPU library.

One case per test method of a suite, its `Test` lines looped inside.  The library is cmsisdsp_amd's drop-ins, called
through ctypes on host buffers exactly as the suite calls arm_math.h.  Every row must pass the suite's own thresholds
against the double-precision pattern, give the words the reference build gave for that row (<row>/ref_words) and leave
the output's tail alone.  The Basic, Stats and BIQUAD suites run every row a second time through the _batch form on
device buffers, as a batch of three copies of the row: every item must equal the drop-in's words."""
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


BATCH = {"basic": BasicBatch, "stats": StatsBatch, "biquad": BiquadBatch}


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
        if batch:
            again, failed = sr.run_row(row, batch(dsp, torch_gpu), pats)
            assert not failed, (row.id, "batch", failed)
            for k, v in outs.items():
                if k not in sr.SCRATCH:
                    sr.same_words(again[k], v, (row.id, "the _batch form against the drop-in"))
