"""The f32 functions on subnormals, signed zeros, sums that overflow, infinities and NaNs.

The f32 kernels claim the reference's words bit for bit (same operations, same association order,
no FMA).  The other f32 tests draw well-scaled inputs; here every function runs on the value
classes of tests/f32_classes.py, where a denormal flush, a wrong-signed zero (an accumulator seeded
with the first product, a - b as a + (-b), a skipped trivial twiddle) or a zero-padded 0 * Inf show.

CPU part (every case of the GPU part): the reference build's own output must show the class
(conditions below: a GPU case can then never pass vacuously), and the C restatement (oracle/src)
equals the reference build under assert_same_words wherever refs.oracle_lib() wraps the function.

GPU part: the batched device entry points (the drop-ins where noted) against the reference build,
per stream, under assert_same_words: finite words by their bits, NaNs by position.  Every batch
holds ordinary uniform(-1, 1) streams (the last one and every eighth) next to the extreme ones,
each stream with a seed of its own; filters run consecutive calls with the state carried (a
non-finite or subnormal word in the carried history) and compare the state too.

Two conditions of the reference cannot hold as first written and are narrowed here, by reasoning
and not by what the kernels return:
  * a 1030-tap FIR spreads one non-finite sample over 1030 outputs, so that shape runs five calls of
    300 samples instead of two: only then is there a finite word after the affected run;
  * a biquad is recursive: once a state word is NaN every later output is NaN, so the affected run
    has no far side; the condition there is a finite word before the run and a non-finite one in it.

The one known divergence (conv.hip, the windowed f32 convolution: a non-finite word in the input
that the kernel runs as taps meets the window's padding zeros, 0 * Inf = NaN, where the reference has
no such term) is pinned in test_conv_nonfinite: outputs at which every tap meets a sample equal the
reference, the others hold the reference's word or NaN.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import biquad_ref
import mfcc_cfg
import refs
from cmsisdsp_amd import _abi
from f32_classes import CLASSES, assert_same_words, classes_of, f32_class_input

FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------ inputs
def is_ordinary(r, batch):
    """The last stream of a batch and every eighth are ordinary uniform(-1, 1) (a lone stream is not)."""
    return batch > 1 and (r == batch - 1 or r % 8 == 7)


def extreme_rows(batch):
    return [r for r in range(batch) if not is_ordinary(r, batch)]


def stream_rows(cls, batch, words, seed, scale=None, positions=None):
    """[batch, words], one seed per stream."""
    x = np.stack([f32_class_input("uniform" if is_ordinary(r, batch) else cls, words, seed * 4099 + r, scale, positions)
                  for r in range(batch)])
    x.setflags(write=False)
    return x


def transform_rows(cls, batch, words, seed, scale=None):
    """As stream_rows; the non-finite words of a transform's batch are spread over its streams (one
    +Inf in stream 0, one -Inf and the NaN in stream 1, or the NaN in stream 2 when there is one),
    since a single NaN turns every word of its own transform into NaN and would hide the Infs."""
    if cls != "nonfinite":
        return stream_rows(cls, batch, words, seed, scale)
    ext = extreme_rows(batch)
    assert ext == list(range(len(ext))) and len(ext) >= 2
    pos = (5, words + 11, (2 if len(ext) > 2 else 1) * words + 17)
    x = stream_rows("uniform", batch, words, seed).copy()
    x[:len(ext)] = f32_class_input("nonfinite", (len(ext), words), seed, positions=pos)
    x.setflags(write=False)
    return x


def split(x, blocks):
    """[batch, sum(blocks)] -> per stream the list of its consecutive blocks."""
    cuts = np.cumsum(blocks)[:-1]
    return [np.split(row, cuts) for row in x]


def filter_positions(block0, hist):
    """+Inf, -Inf, NaN of a stream's concatenated input: all in the first call, the NaN in its last
    min(hist, 2) samples, so that the carried history holds a non-finite word."""
    p = block0 - min(max(hist, 1), 2)
    assert p >= 7
    return (p - 7, p - 3, p)


# ------------------------------------------------------------------ conditions on the reference's output
def conditions(cls, y, kind, n=0):
    """The reference's own output words y [streams, words] (extreme streams only) must show the class.
    kind: "fwd" / "inv" (transforms), "filter" (finite impulse response), "iir", "conv"."""
    s = classes_of(y)
    if cls == "subnormal":
        assert s["subnormal"] >= 0.5, s
    elif cls in ("negzero", "signzero"):
        assert s["pzero"] + s["nzero"] == 1.0, s
        if kind == "fwd":
            assert s["nzero"] > 0 and s["pzero"] > 0, s
        elif kind == "inv":
            assert s["nzero"] >= 0.25 and s["pzero"] >= 0.25, s
        elif kind in ("filter", "conv"):                # the sum starts at +0.0f
            assert s["nzero"] == 0, s
    elif cls == "mixed":
        assert s["inf"] + s["nan"] == 0 and s["normal"] >= 0.5, s
    elif cls == "overflow":
        assert s["inf"] > 0 and s["inf"] + s["nan"] <= 0.5, s
    elif cls == "inftap":
        assert s["inf"] + s["nan"] > 0, s
    elif cls == "nonfinite":
        assert s["inf"] + s["nan"] > 0, s
        if kind in ("fwd", "inv"):
            if n >= 1024:
                assert s["inf"] > 0 and s["nan"] > 0, s
        elif kind in ("filter", "iir"):
            for row in np.atleast_2d(y):
                bad = np.flatnonzero(~np.isfinite(row))
                assert bad.size and bad[0] > 0, "no finite word before the affected run"
                if kind == "filter":
                    assert bad[-1] < row.size - 1, "no finite word after the affected run"
    else:
        raise ValueError(cls)


def carried_shows(cls, x, block, hist):
    """The history that the second call starts from (the last `hist` samples of the first block of
    every extreme stream) holds a non-finite word / only subnormals."""
    h = x[:, max(0, block - hist):block]
    if cls == "nonfinite":
        assert (~np.isfinite(h)).any(axis=1).all()
    elif cls == "subnormal":
        assert classes_of(h)["subnormal"] == 1.0


def same(got, want, what):
    """Dicts of arrays with the same keys, each under assert_same_words."""
    assert got.keys() == want.keys()
    for k in want:
        assert_same_words(got[k], want[k], f"{what} {k}")


def frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


# The conditions above are met by construction, not by luck at run time: where a case's default seed
# or overflow scale leaves the reference's output short of its condition (no -0.0 among the zeros of a
# forward transform, no sum past FLT_MAX, or more than half of them), the case gets another seed
# (SALT) or another scale 2^e (EXP) here.  Keys: (family, shape ..., class).
SALT = {
    ("cfft", 32, 0, 1, 5, "signzero"): 1,
    ("rfft", 256, 0, "signzero"): 1,
    ("rfft", 1024, 0, "signzero"): 1,
}
EXP = {
    ("rfft", 32, 1, "overflow"): 125.5,
    ("rfft", 32, 2, "overflow"): 125.0,
    ("rfft", 256, 1, "overflow"): 123.25,
    ("rfft", 1024, 2, "overflow"): 122.25,
    ("decimate_f32", 29, 2, "overflow"): 127.25,
    ("decimate_f32", 29, 5, "overflow"): 127.25,
    ("interpolate_f32", 32, 2, "overflow"): 127.25,
    ("lattice", 33, "overflow"): 125.25,
    ("conv", 50, 7, "overflow"): 126.85,
    ("conv", 7, 50, "overflow"): 126.85,
    ("conv", 1100, 1030, "overflow"): 122.5,
    # three sections of peak gain 1: only words next to FLT_MAX overflow (2^127.99 < FLT_MAX)
    ("arm_biquad_cascade_df2T_f32", 3, "overflow"): 127.99,
    ("arm_biquad_cascade_stereo_df2T_f32", 3, "overflow"): 127.99,
}


def seed_of(base, *key):
    return base + 7919 * SALT.get(key, 0)


def scale_of(default_exp, *key):
    """Overflow scale 2^e: finite words whose sums overflow."""
    return 2.0 ** EXP.get(key, default_exp)


# ================================================================== CFFT
CFFT_SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
CFFT_CASES = [(n, ifft, 1) for n in CFFT_SIZES for ifft in (0, 1)] + [(256, 0, 0), (256, 1, 0)]


@functools.lru_cache(maxsize=None)
def cfft_case(n, ifft, bitrev, cls, batch):
    # 2^(127 - log2(N)/2): about 1 % Inf from N = 64 on
    key = ("cfft", n, ifft, bitrev, batch, cls)
    x = transform_rows(cls, batch, 2 * n, seed_of(7 * n + ifft + 3 * bitrev + 31 * CLASSES.index(cls), *key),
                       scale_of(127.0 - np.log2(n) / 2, *key))
    want = refs.ref_lib().cfft_many("f32", n, x, ifft, bitrev)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n,ifft,bitrev,batch", [c + (5,) for c in CFFT_CASES] +
                         [(n, ifft, 1, 4) for n in (1024, 64) for ifft in (0, 1)])     # batch 4: the drop-in's transforms
def test_cfft_reference_shows_class_and_restatement_agrees(oracle, n, ifft, bitrev, batch, cls):
    x, want = cfft_case(n, ifft, bitrev, cls, batch)
    conditions(cls, want[extreme_rows(batch)], "inv" if ifft else "fwd", n)
    assert_same_words(oracle.cfft_many("f32", n, x, ifft, bitrev), want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n,ifft,bitrev", CFFT_CASES)
def test_cfft_batch(dsp, torch_gpu, n, ifft, bitrev, cls):
    x, want = cfft_case(n, ifft, bitrev, cls, 5)
    d = torch_gpu.from_numpy(x.copy()).cuda()
    dsp.cfft_batch(dsp.const_instance(f"arm_cfft_sR_f32_len{n}"), d, ifft, bitrev)
    got = d.cpu().numpy()
    for r in range(5):
        assert_same_words(got[r], want[r], f"stream {r}")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n", [1024, 64])
def test_cfft_dropin(dsp, torch_gpu, n, cls):
    """One transform per call (N = 1024: the 2-wave latency kernel), host buffers."""
    S = dsp.arm_cfft_instance_f32()
    assert dsp.arm_cfft_init_f32(S, n) == 0
    for ifft in (0, 1):
        x, want = cfft_case(n, ifft, 1, cls, 4)
        for r in range(4):
            assert_same_words(dsp.arm_cfft_f32(S, x[r], ifft, 1), want[r], f"ifft {ifft} transform {r}")


# ================================================================== RFFT fast
RFFT_CASES = [(n, ifft) for n in (32, 256, 1024, 4096) for ifft in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def rfft_case(n, ifft, cls):
    batch = 3
    x = transform_rows(cls, batch, n, seed_of(11 * n + ifft + 37 * CLASSES.index(cls), "rfft", n, ifft, cls),
                       scale_of(127.0 - np.log2(n) / 2, "rfft", n, ifft, cls))
    ref = refs.ref_lib()
    res = [ref.rfft(n, x[r], ifft) for r in range(batch)]
    return x, frozen({"out": np.stack([o for o, _ in res]), "p": np.stack([p for _, p in res])})


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n,ifft", RFFT_CASES)
def test_rfft_reference_shows_class_and_restatement_agrees(oracle, n, ifft, cls):
    x, want = rfft_case(n, ifft, cls)
    # ifftFlag 2 (merge, then a forward inner CFFT) is neither direction: its zeros carry no sign condition
    conditions(cls, want["out"][extreme_rows(3)], {0: "fwd", 1: "inv", 2: "other"}[ifft], n)
    res = [oracle.rfft(n, x[r], ifft) for r in range(3)]
    same({"out": np.stack([o for o, _ in res]), "p": np.stack([p for _, p in res])}, want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n,ifft", RFFT_CASES)
def test_rfft_batch(dsp, torch_gpu, n, ifft, cls):
    """out always; p (the forward leaves the inner CFFT's output there, the inverse leaves it alone)
    whenever test_rfft_batch_bitexact compares it."""
    torch = torch_gpu
    x, want = rfft_case(n, ifft, cls)
    S = dsp.const_instance(f"arm_rfft_fast_sR_f32_len{n}")
    for p_scratch in (False, True):
        p = torch.from_numpy(x.copy()).cuda()
        out = torch.zeros_like(p)
        dsp.rfft_fast_batch(S, p, out, ifft, p_scratch=p_scratch)
        got, got_p = out.cpu().numpy(), p.cpu().numpy()
        for r in range(3):
            assert_same_words(got[r], want["out"][r], f"out, p_scratch {p_scratch}, stream {r}")
            if not p_scratch or ifft:
                assert_same_words(got_p[r], want["p"][r], f"p, p_scratch {p_scratch}, stream {r}")


# ================================================================== FIR
# (numTaps, block, calls, batch): the small kernel; R = 8; R = 16 with numTaps % 8 != 0; tap segments
FIR_SHAPES = [(29, 32, 2, 5), (29, 100, 2, 9), (130, 4096, 2, 9), (1030, 300, 5, 9)]
FIR_CLASSES = CLASSES + ("inftap",)


def fir_taps(taps, seed, inf_tap=False):
    """Normalised random taps with two +0.0 and one -0.0 among them."""
    c = (np.random.default_rng(seed).standard_normal(taps) / np.sqrt(taps)).astype(np.float32)
    c[[3, 7]] = 0.0
    c[11] = -0.0
    if inf_tap:
        c[5] = np.inf
    return c


@functools.lru_cache(maxsize=None)
def fir_case(taps, block, calls, batch, cls):
    blocks = [block] * calls
    c = fir_taps(taps, taps + block, inf_tap=cls == "inftap")
    x = stream_rows("uniform" if cls == "inftap" else cls, batch, block * calls,
                    seed_of(taps * 13 + block + 41 * FIR_CLASSES.index(cls), "fir", taps, block, cls),
                    scale_of(127.0, "fir", taps, block, cls), filter_positions(block, taps - 1))
    return c, blocks, x, fir_host(refs.ref_lib(), c, blocks, x)


def fir_host(host, c, blocks, x):
    res = [host.fir("f32", c, b) for b in split(x, blocks)]
    return frozen({"y": np.stack([np.concatenate(o) for o, _ in res]), "hist": np.stack([s[:len(c) - 1] for _, s in res])})


@pytest.mark.parametrize("cls", FIR_CLASSES)
@pytest.mark.parametrize("taps,block,calls,batch", FIR_SHAPES)
def test_fir_reference_shows_class_and_restatement_agrees(oracle, taps, block, calls, batch, cls):
    c, blocks, x, want = fir_case(taps, block, calls, batch, cls)
    conditions(cls, want["y"][extreme_rows(batch)], "filter")
    carried_shows(cls, x[extreme_rows(batch)], block, taps - 1)
    same(fir_host(oracle, c, blocks, x), want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", FIR_CLASSES)
@pytest.mark.parametrize("taps,block,calls,batch", FIR_SHAPES)
def test_fir_batch(dsp, torch_gpu, taps, block, calls, batch, cls):
    torch = torch_gpu
    c, blocks, x, want = fir_case(taps, block, calls, batch, cls)
    S = dsp.arm_fir_instance_f32()
    S.numTaps = taps
    dc = torch.from_numpy(c.copy()).cuda()
    S.pCoeffs = C.cast(dc.data_ptr(), S._fields_[2][1])
    hist = torch.zeros((batch, taps - 1), dtype=torch.float32, device="cuda")
    outs = []
    for k in range(calls):
        src = torch.from_numpy(x[:, k * block:(k + 1) * block].copy()).cuda()
        dst = torch.empty_like(src)
        dsp.fir_batch(S, src, dst, hist, kind="f32")
        outs.append(dst.cpu().numpy())
    got = {"y": np.concatenate(outs, axis=1), "hist": hist.cpu().numpy()}
    for r in range(batch):
        same({k: v[r] for k, v in got.items()}, {k: v[r] for k, v in want.items()}, f"stream {r}")


# ================================================================== decimator / interpolator
MR_CLASSES = ("subnormal", "signzero", "overflow", "nonfinite")
# (fn, numTaps, factor, block): the decimator through the FIR pass (M = 2, 3: M <= 4) and through its own
# kernel (M = 5); the interpolator's 4-output kernel with 2 and 3 phases and the general one (L = 5)
MR_SHAPES = [("decimate_f32", 29, 2, 96), ("decimate_f32", 29, 3, 96), ("decimate_f32", 29, 5, 100),
             ("interpolate_f32", 32, 2, 50), ("interpolate_f32", 30, 3, 50), ("interpolate_f32", 30, 5, 50)]


@functools.lru_cache(maxsize=None)
def mr_case(fn, taps, factor, block, cls):
    batch, blocks = 5, [block, block]
    decim = fn.startswith("decimate")
    per_out = taps if decim else taps // factor               # products per output
    H = taps - 1 if decim else taps // factor - 1
    c = (np.random.default_rng(taps + factor).standard_normal(taps) / np.sqrt(per_out)).astype(np.float32)
    c[3] = 0.0
    c[4] = -0.0
    x = stream_rows(cls, batch, 2 * block, seed_of(taps * 17 + factor + 43 * MR_CLASSES.index(cls), fn, taps, factor, cls),
                    scale_of(127.0, fn, taps, factor, cls), filter_positions(block, H))
    return c, blocks, H, x, mr_host(refs.ref_lib(), fn, factor, c, blocks, H, x)


def mr_host(host, fn, factor, c, blocks, H, x):
    res = [host.multirate(fn, factor, c, b) for b in split(x, blocks)]
    assert all(st == 0 for st, _, _ in res)
    return frozen({"y": np.stack([np.concatenate(o) for _, o, _ in res]), "hist": np.stack([s[:H] for _, _, s in res])})


@pytest.mark.parametrize("cls", MR_CLASSES)
@pytest.mark.parametrize("fn,taps,factor,block", MR_SHAPES)
def test_multirate_reference_shows_class_and_restatement_agrees(oracle, fn, taps, factor, block, cls):
    c, blocks, H, x, want = mr_case(fn, taps, factor, block, cls)
    conditions(cls, want["y"][extreme_rows(5)], "filter")
    carried_shows(cls, x[extreme_rows(5)], block, H)
    same(mr_host(oracle, fn, factor, c, blocks, H, x), want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", MR_CLASSES)
@pytest.mark.parametrize("fn,taps,factor,block", MR_SHAPES)
def test_multirate_batch(dsp, torch_gpu, fn, taps, factor, block, cls):
    torch = torch_gpu
    batch = 5
    c, blocks, H, x, want = mr_case(fn, taps, factor, block, cls)
    dc = torch.from_numpy(c.copy()).cuda()
    if fn.startswith("decimate"):
        S = _abi.arm_fir_decimate_instance(M=factor, numTaps=taps, pCoeffs=dc.data_ptr(), pState=None)
        nout = block // factor
    else:
        S = _abi.arm_fir_interpolate_instance(L=factor, phaseLength=taps // factor, pCoeffs=dc.data_ptr(), pState=None)
        nout = block * factor
    hist = torch.zeros((batch, H), dtype=torch.float32, device="cuda")
    f = getattr(dsp.lib, f"arm_fir_{fn}_batch")
    outs = []
    for k in range(2):
        src = torch.from_numpy(x[:, k * block:(k + 1) * block].copy()).cuda()
        dst = torch.empty((batch, nout), dtype=torch.float32, device="cuda")
        st = f(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), block, batch,
               C.c_void_p(hist.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, dsp.last_error()
        outs.append(dst.cpu().numpy())
    got = {"y": np.concatenate(outs, axis=1), "hist": hist.cpu().numpy()}
    for r in range(batch):
        same({k: v[r] for k, v in got.items()}, {k: v[r] for k, v in want.items()}, f"stream {r}")


# ================================================================== sparse FIR
SP_CLASSES = ("subnormal", "signzero", "nonfinite")
# (numTaps, maxDelay, block): the LDS-staged kernel, the direct-read kernel (4 (maxDelay + 4096) bytes
# above 64 KiB of LDS); the drop-in runs the circular-state kernel
SP_SHAPES = [(16, 20, 100), (16, 12300, 100)]


@functools.lru_cache(maxsize=None)
def sparse_case(taps, max_delay, block, cls, batch):
    rng = np.random.default_rng(taps + max_delay)
    c = (rng.standard_normal(taps) / np.sqrt(taps)).astype(np.float32)
    # delays that the two calls reach, short enough for a finite word after the last non-finite one
    d = rng.integers(0, min(max_delay, block - 10), taps, endpoint=True).astype(np.int32)
    d[0], d[1], d[2] = max_delay, 0, max_delay
    blocks = [block, block]
    x = stream_rows(cls, batch, 2 * block,
                    seed_of(taps * 19 + max_delay + batch + 47 * SP_CLASSES.index(cls), "sparse", max_delay, batch, cls),
                    positions=filter_positions(block, max_delay))
    return c, d, blocks, x, sparse_host(refs.ref_lib(), c, d, max_delay, blocks, x)


def sparse_host(host, c, d, max_delay, blocks, x):
    res = [host.sparse("f32", c, d, max_delay, b) for b in split(x, blocks)]
    return frozen({"y": np.stack([np.concatenate(o) for o, _, _ in res]), "state": np.stack([s for _, s, _ in res]),
                   "index": np.array([i for _, _, i in res], dtype=np.float32)})


@pytest.mark.parametrize("cls", SP_CLASSES)
@pytest.mark.parametrize("taps,max_delay,block,batch", [s + (5,) for s in SP_SHAPES] + [SP_SHAPES[0] + (1,)])
def test_sparse_reference_shows_class_and_restatement_agrees(oracle, taps, max_delay, block, batch, cls):
    c, d, blocks, x, want = sparse_case(taps, max_delay, block, cls, batch)
    conditions(cls, want["y"][extreme_rows(batch)], "filter")
    same(sparse_host(oracle, c, d, max_delay, blocks, x), want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", SP_CLASSES)
@pytest.mark.parametrize("taps,max_delay,block", SP_SHAPES)
def test_sparse_batch(dsp, torch_gpu, taps, max_delay, block, cls):
    torch = torch_gpu
    batch = 5
    c, d, blocks, x, want = sparse_case(taps, max_delay, block, cls, batch)
    dc, dd = torch.from_numpy(c.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    S = _abi.arm_fir_sparse_instance(numTaps=taps, pCoeffs=dc.data_ptr(), maxDelay=max_delay, pTapDelay=dd.data_ptr())
    hist = torch.zeros((batch, max_delay), dtype=torch.float32, device="cuda")
    outs = []
    for k in range(2):
        src = torch.from_numpy(x[:, k * block:(k + 1) * block].copy()).cuda()
        dst = torch.empty_like(src)
        st = dsp.lib.arm_fir_sparse_f32_batch(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), block,
                                              batch, C.c_void_p(hist.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, dsp.last_error()
        outs.append(dst.cpu().numpy())
    got, h = np.concatenate(outs, axis=1), hist.cpu().numpy()
    for r in range(batch):
        assert_same_words(got[r], want["y"][r], f"stream {r}")
        tail = np.concatenate([np.zeros(max_delay, np.float32), x[r]])[-max_delay:]
        assert_same_words(h[r], tail, f"history of stream {r}")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", SP_CLASSES)
def test_sparse_dropin(dsp, torch_gpu, cls):
    """One stream through arm_fir_sparse_f32 on host buffers (the circular-state kernel): outputs, the
    circular state and stateIndex."""
    taps, max_delay, block = SP_SHAPES[0]
    c, d, blocks, x, want = sparse_case(taps, max_delay, block, cls, 1)
    same(sparse_host(refs.Host(dsp.lib, ""), c, d, max_delay, blocks, x), want, "drop-in")


# ================================================================== FIR lattice
LAT_CLASSES = ("subnormal", "signzero", "overflow", "nonfinite")
LAT_SHAPES = [(8, 100, 5), (33, 257, 70)]


@functools.lru_cache(maxsize=None)
def lattice_case(stages, block, batch, cls):
    c = np.random.default_rng(stages).uniform(-0.9, 0.9, stages).astype(np.float32)
    blocks = [block, block]
    x = stream_rows(cls, batch, 2 * block, seed_of(stages * 23 + block + 53 * LAT_CLASSES.index(cls), "lattice", stages, cls),
                    scale_of(126.0, "lattice", stages, cls), filter_positions(block, stages))
    return c, blocks, x, lattice_host(refs.ref_lib(), c, blocks, x)


def lattice_host(host, c, blocks, x):
    res = [host.lattice("f32", c, b) for b in split(x, blocks)]
    return frozen({"y": np.stack([np.concatenate(o) for o, _ in res]), "state": np.stack([s for _, s in res])})


@pytest.mark.parametrize("cls", LAT_CLASSES)
@pytest.mark.parametrize("stages,block,batch", LAT_SHAPES)
def test_lattice_reference_shows_class_and_restatement_agrees(oracle, stages, block, batch, cls):
    c, blocks, x, want = lattice_case(stages, block, batch, cls)
    conditions(cls, want["y"][extreme_rows(batch)], "filter")
    same(lattice_host(oracle, c, blocks, x), want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("cls", LAT_CLASSES)
@pytest.mark.parametrize("stages,block,batch", LAT_SHAPES)
def test_lattice_batch(dsp, torch_gpu, stages, block, batch, cls):
    torch = torch_gpu
    c, blocks, x, want = lattice_case(stages, block, batch, cls)
    dc = torch.from_numpy(c.copy()).cuda()
    S = _abi.arm_fir_lattice_instance(numStages=stages, pState=None, pCoeffs=dc.data_ptr())
    state = torch.zeros((batch, stages), dtype=torch.float32, device="cuda")
    outs = []
    for k in range(2):
        src = torch.from_numpy(x[:, k * block:(k + 1) * block].copy()).cuda()
        dst = torch.empty_like(src)
        st = dsp.lib.arm_fir_lattice_f32_batch(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), block,
                                               batch, C.c_void_p(state.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0, dsp.last_error()
        outs.append(dst.cpu().numpy())
    got = {"y": np.concatenate(outs, axis=1), "state": state.cpu().numpy()}
    for r in range(batch):
        same({k: v[r] for k, v in got.items()}, {k: v[r] for k, v in want.items()}, f"stream {r}")


# ================================================================== convolution family
CONV_CLASSES = ("subnormal", "signzero", "mixed", "overflow")
# windowed kernel in both length orders; the direct kernel (srcBLen > 1024)
CONV_SHAPES = [(50, 7), (7, 50), (1100, 1030)]
CONV_FNS = ("conv_f32", "correlate_f32", "conv_partial_f32")


def partial_range(la, lb):
    """Starts inside the head (the first min - 1 outputs) and ends among the full overlaps."""
    return 3, min(la, lb) + 14


def conv_want(fn, a, b, first, num):
    y, st = refs.ref_lib().conv_family(fn, a, b, first, num, fill=3)
    assert st == 0
    return y


def conv_operands(la, lb, cls, seed, where="a"):
    """[3, la], [3, lb]: the class in the first operand (both for `mixed`; `where` for `nonfinite`),
    the other one ordinary and normalised; the last pair ordinary."""
    batch = 3
    if cls == "nonfinite":
        A, B = stream_rows("uniform", batch, la, seed), stream_rows("uniform", batch, lb, seed + 1)
        n = la if where == "a" else lb
        X = stream_rows(cls, batch, n, seed + 2, positions=(n // 3, n // 2, n - 2))
        return (X, B) if where == "a" else (A, X)
    # overflow: a sum of min(la, lb) products of about scale / 2 each
    A = stream_rows(cls, batch, la, seed, scale_of(127.0 - np.log2(min(la, lb)) / 2, "conv", la, lb, cls))
    B = stream_rows("mixed" if cls == "mixed" else "uniform", batch, lb, seed + 1)
    return A, B


@functools.lru_cache(maxsize=None)
def conv_case(la, lb, cls, fn, where="a"):
    A, B = conv_operands(la, lb, cls, seed_of(la * 29 + lb + 59 * len(cls) + len(fn), "conv", la, lb, cls, fn), where)
    first, num = partial_range(la, lb) if fn == "conv_partial_f32" else (0, 0)
    want = np.stack([conv_want(fn, A[i], B[i], first, num) for i in range(3)])
    want.setflags(write=False)
    return A, B, first, num, want


def conv_gpu(dsp, torch, fn, A, B, first, num, width):
    """The batched call -> [3, width] with the reference's layout (partial: placed at `first`, the
    words outside the range holding the fill 3)."""
    dA, dB = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
    if fn == "conv_f32":
        out = torch.full((3, width), 3, dtype=torch.float32, device="cuda")
        dsp.conv_batch(dA, dB, out)
        return out.cpu().numpy()
    if fn == "correlate_f32":
        out = torch.full((3, width), 3, dtype=torch.float32, device="cuda")
        dsp.conv_family_batch(fn, dA, dB, out)
        return out.cpu().numpy()
    out = torch.full((3, num), 3, dtype=torch.float32, device="cuda")
    dsp.conv_family_batch(fn, dA, dB, out, first, num)
    got = np.full((3, width), 3, dtype=np.float32)
    got[:, first:first + num] = out.cpu().numpy()
    return got


@pytest.mark.parametrize("fn", CONV_FNS)
@pytest.mark.parametrize("cls", CONV_CLASSES)
@pytest.mark.parametrize("la,lb", CONV_SHAPES)
def test_conv_reference_shows_class_and_restatement_agrees(oracle, la, lb, cls, fn):
    A, B, first, num, want = conv_case(la, lb, cls, fn)
    written = np.stack([conv_want(fn, np.ones(la, np.float32), np.ones(lb, np.float32), first, num) != 3] * 2)
    conditions(cls, want[:2][written], "conv")
    for i in range(3):
        assert_same_words(oracle.conv_family(fn, A[i], B[i], first, num, fill=3)[0], want[i], f"restatement {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("fn", CONV_FNS)
@pytest.mark.parametrize("cls", CONV_CLASSES)
@pytest.mark.parametrize("la,lb", CONV_SHAPES)
def test_conv_batch(dsp, torch_gpu, la, lb, cls, fn):
    A, B, first, num, want = conv_case(la, lb, cls, fn)
    got = conv_gpu(dsp, torch_gpu, fn, A, B, first, num, want.shape[1])
    for i in range(3):
        assert_same_words(got[i], want[i], f"pair {i}")
    if fn == "conv_f32":
        assert_same_words(dsp.arm_conv("f32", A[0], B[0]), want[0], "drop-in")


def conv_taps(fn, la, lb):
    """(operand, length) of the input that the windowed kernel runs as FIR taps over the zero-padded window
    of the other one (api.cpp conv_plan): pSrcB for arm_conv_f32 / arm_conv_partial_f32 in either length
    order, the shorter input for arm_correlate_f32."""
    if fn == "correlate_f32" and la < lb:
        return "a", la
    return "b", lb


def all_taps_meet_samples(fn, la, lb, first, num):
    """Per word of pDst: does the reference sum as many products there as the kernel has taps (so that no
    tap meets a padding zero)?  Counted by the reference itself on all-ones inputs (untouched words hold
    the fill 0)."""
    y, _ = refs.ref_lib().conv_family(fn, np.ones(la, np.float32), np.ones(lb, np.float32), first, num, fill=0)
    return y == conv_taps(fn, la, lb)[1]


@pytest.mark.parametrize("fn", CONV_FNS)
@pytest.mark.parametrize("where", ["a", "b"])
@pytest.mark.parametrize("la,lb", CONV_SHAPES)
def test_conv_nonfinite_reference_and_restatement(oracle, la, lb, where, fn):
    """A non-finite word in the longer input reaches a bounded run of outputs; in either input the
    restatement follows the reference.  The outputs at which every tap meets a sample are srcBLen - 1 ..
    srcALen - 1 of the convolution (none when srcALen < srcBLen), and the max - min + 1 full overlaps
    of the correlation."""
    A, B, first, num, want = conv_case(la, lb, "nonfinite", fn, where)
    assert (~np.isfinite(want[:2])).any(axis=1).all()
    if (la if where == "a" else lb) == max(la, lb) and fn != "conv_partial_f32":
        assert np.isfinite(want[:2]).any(axis=1).all()
    safe = all_taps_meet_samples(fn, la, lb, first, num)
    taps = conv_taps(fn, la, lb)[1]
    lo, hi = taps - 1, la + lb - 1 - taps                      # as indices of the convolution
    if fn == "conv_partial_f32":
        lo, hi = max(lo, first), min(hi, first + num - 1)
    assert safe.sum() == max(0, hi - lo + 1)
    if fn != "correlate_f32":
        assert safe[lo:hi + 1].all()
    for i in range(3):
        assert_same_words(oracle.conv_family(fn, A[i], B[i], first, num, fill=3)[0], want[i], f"restatement {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("fn", CONV_FNS)
@pytest.mark.parametrize("where", ["a", "b"])
@pytest.mark.parametrize("la,lb", CONV_SHAPES)
def test_conv_nonfinite(dsp, torch_gpu, la, lb, where, fn):
    """Non-finite words in the input that the kernel slides its window over, or in either input of the
    direct kernel (more than 1024 taps: the exact overlap): the reference's words at every output.
    Non-finite words in the taps of the windowed kernel (conv_taps: pSrcB of arm_conv_f32 and
    arm_conv_partial_f32, also when it is the longer input; the shorter input of arm_correlate_f32):
    the reference's words wherever every tap meets a sample; at the other outputs the kernel also
    multiplies the window's padding zeros by the non-finite tap, where the reference has no such term,
    so each word there is the reference's or NaN.  The ordinary pair of the batch is exact."""
    A, B, first, num, want = conv_case(la, lb, "nonfinite", fn, where)
    got = conv_gpu(dsp, torch_gpu, fn, A, B, first, num, want.shape[1])
    operand, taps = conv_taps(fn, la, lb)
    if where != operand or taps > 1024:
        for i in range(3):
            assert_same_words(got[i], want[i], f"pair {i}")
        return
    safe = all_taps_meet_samples(fn, la, lb, first, num)
    for i in range(2):
        assert_same_words(got[i][safe], want[i][safe], f"pair {i}, every tap on a sample")
        rest = np.where(np.isnan(got[i]) & ~safe, want[i], got[i])        # NaN allowed only where a tap meets padding
        assert_same_words(rest, want[i], f"pair {i}, taps on padding")
    assert_same_words(got[2], want[2], "the ordinary pair")


# ================================================================== biquad cascades
BQ_FUNCS = ("arm_biquad_cascade_df1_f32", "arm_biquad_cascade_df2T_f32", "arm_biquad_cascade_stereo_df2T_f32")
BQ_CLASSES = ("subnormal", "signzero", "overflow", "nonfinite")
# (numStages, blocks, batch): one stream per lane; two streams per lane
BQ_SHAPES = [(3, (33, 31), 65), (32, (17, 40), 4097)]


@functools.lru_cache(maxsize=None)
def biquad_case(func, stages, blocks, batch, cls):
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    c = biquad_ref.stable_coeffs(func, stages, 0, 1000 + stages)
    words = ch * sum(blocks)
    p = ch * blocks[0] - 2
    x = stream_rows(cls, batch, words, seed_of(stages * 31 + len(func) + 61 * BQ_CLASSES.index(cls), func, stages, cls),
                    scale_of(127.9, func, stages, cls), (p - 9, p - 5, p))
    st = np.zeros((batch, ks * stages), dtype=sdt)
    ys, sts, at = [], [], 0
    with np.errstate(invalid="ignore"):                      # Inf - Inf is part of the classes
        for b in blocks:
            y, st = biquad_ref.run(func, c, 0, x[:, at:at + ch * b], st)
            ys.append(y), sts.append(st)
            at += ch * b
    for a in ys + sts:
        a.setflags(write=False)
    return c, x, ys, sts


@pytest.mark.parametrize("func", BQ_FUNCS)
@pytest.mark.parametrize("stages,blocks,batch", BQ_SHAPES)
@pytest.mark.parametrize("cls", BQ_CLASSES)
def test_biquad_checker_shows_class(func, stages, blocks, batch, cls):
    """biquad_ref.run (numpy float32) is the checker here: it must not flush subnormals itself, and
    its output must show each class."""
    c, x, ys, sts = biquad_case(func, stages, blocks, batch, cls)
    ext = extreme_rows(batch)
    conditions(cls, np.concatenate(ys, axis=1)[ext], "iir")
    if cls in ("subnormal", "nonfinite"):
        s = classes_of(sts[0][ext])
        assert s["subnormal"] >= 0.5 if cls == "subnormal" else s["inf"] + s["nan"] > 0, s


@pytest.mark.gpu
@pytest.mark.parametrize("func", BQ_FUNCS)
@pytest.mark.parametrize("stages,blocks,batch", BQ_SHAPES)
@pytest.mark.parametrize("cls", BQ_CLASSES)
def test_biquad_batch(dsp, torch_gpu, func, stages, blocks, batch, cls):
    torch = torch_gpu
    dt, sdt, ks, nc, ch = biquad_ref.FUNCS[func]
    c, x, ys, sts = biquad_case(func, stages, blocks, batch, cls)
    S = _abi.BIQUAD_FUNCS[func][0](numStages=stages, pState=None, pCoeffs=c.ctypes.data)
    state = torch.zeros((batch, ks * stages), dtype=torch.float32, device="cuda")
    f = getattr(dsp.lib, func + "_batch")
    at = 0
    for b, y, st in zip(blocks, ys, sts):
        src = torch.from_numpy(x[:, at:at + ch * b].copy()).cuda()
        dst = torch.zeros_like(src)
        rc = f(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), b, batch, C.c_void_p(state.data_ptr()),
               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, dsp.last_error()
        assert_same_words(dst.cpu().numpy(), y, f"block {b}")
        assert_same_words(state.cpu().numpy(), st, f"state after block {b}")
        at += ch * b


# ================================================================== MFCC
MFCC_FRAMES = ("pzero", "nzero", "subnormal", "huge", "nan", "uniform")


@functools.lru_cache(maxsize=None)
def mfcc_case(n):
    cfg = mfcc_cfg.make_cfg(n)
    frames = np.stack([f32_class_input("uniform", n, 5 * n + i) for i in range(len(MFCC_FRAMES))])
    frames[0] = 0.0
    frames[1] = -0.0
    frames[2] = f32_class_input("subnormal", n, 5 * n + 2)
    frames[3] *= np.float32(FLT_MAX / n)                  # near FLT_MAX / fftLen
    frames[4, n // 3] = np.nan
    want = refs.ref_lib().mfcc(cfg, frames)
    for a in (frames, want):
        a.setflags(write=False)
    return cfg, frames, want


@pytest.mark.parametrize("n", [256, 1024])
def test_mfcc_reference_and_restatement(oracle, n):
    cfg, frames, want = mfcc_case(n)
    # the reference's magnitude goes through arm_sqrt_f32, which returns 0 for a NaN as for a negative
    # input: the NaN frame ends as the all-zero frames do, and the frames of the batch still differ
    assert np.isfinite(want).all() and want[4].tobytes() == want[0].tobytes() != want[5].tobytes()
    assert_same_words(oracle.mfcc(cfg, frames), want, "restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [256, 1024])
def test_mfcc_batch(dsp, torch_gpu, n):
    """One frame of each kind in one batch, compared as mfcc_cfg.assert_parity does (bit-exact when
    the host's logf is the restated one, else the suite's tolerance and "libm differs"), NaN by position."""
    cfg, frames, want = mfcc_case(n)
    m = dsp.MfccF32(n, cfg["dct"], cfg["pos"], cfg["len"], cfg["coefs"], cfg["window"])
    got = m.batch(torch_gpu.from_numpy(frames.copy()).cuda()).cpu().numpy()
    ok, bad, glibc = mfcc_cfg.host_libm_status()
    if ok:
        for i, kind in enumerate(MFCC_FRAMES):
            assert_same_words(got[i], want[i], f"frame {kind}")
        return
    assert (np.isnan(got) == np.isnan(want)).all()
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-5 + 1.2e-3 * np.abs(want[fin]))
    pytest.skip(f"host libm differs ({glibc}: {bad} sampled mismatches): suite tolerance checked")
