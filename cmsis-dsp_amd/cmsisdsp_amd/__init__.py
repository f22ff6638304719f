"""cmsisdsp_amd — Python face of the MI355X CMSIS-DSP backend (libcmsisdsp_mi355x.so).

Two layers, both thin over the C ABI (include/arm_math.h, include/arm_math_mi355x.h):

* drop-in, numpy in / numpy out, named and shaped like the reference's PythonWrapper
  (`cmsisdsp.arm_cfft_f32(inst, x, ifft, bitrev)` -> new array; PythonWrapper/cmsisdsp_pkg/
  src/cmsisdsp_transform.c:2074):  arm_cfft_f32 / _q31 / _q15, arm_rfft_fast_f32,
  arm_fir_f32 / _q15, arm_mat_mult_f32 with their *_init functions;
* batched, torch device tensors in place on a HIP stream: cfft_batch, rfft_fast_batch,
  fir_batch, mat_mult_batch.

The library is REQUIRED: importing works without a GPU, but every compute call goes to
the HIP kernels; there is no CPU fallback (a missing .so raises at import).
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (arm_cfft_instance_f32, arm_cfft_instance_q15, arm_cfft_instance_q31,  # noqa: F401
                   arm_fir_instance_f32, arm_fir_instance_q15, arm_fir_instance_q31, arm_fir_instance_q7,
                   arm_matrix_instance_f32,
                   arm_rfft_fast_instance_f32, arm_mfcc_instance_f32, arm_mfcc_instance_q31, arm_mfcc_instance_q15,
                   arm_matrix_instance_q15, arm_matrix_instance_q7,
                   arm_matrix_instance_q31, arm_rfft_instance_q31, arm_rfft_instance_q15, ARM_MATH_SUCCESS,
                   ARM_MATH_ARGUMENT_ERROR, ARM_MATH_SIZE_MISMATCH)
from ._abi import arm_sort_instance_f32, arm_merge_sort_instance_f32  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CMSISDSP_MI355X_LIB",
                          os.path.join(os.path.dirname(_HERE), "lib", "libcmsisdsp_mi355x.so"))


def _load():
    # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME
    # libamdhip64.so.7, same as ROCm's).  Loading torch first makes our library bind to
    # that already-loaded runtime instead of pulling in a second ROCr instance (two in
    # one process fail with "no ROCm-capable device").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"cmsisdsp_amd: native library missing at {LIB_PATH} "
                          f"(build it with `make -C cmsis-dsp_amd` or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    _abi.bind(lib, _abi.DROPIN)
    _abi.bind(lib, _abi.MFCC_LEN)
    _abi.bind(lib, _abi.RFFTQ_LEN)
    _abi.bind(lib, _abi.PARTIAL_FAST)
    _abi.bind(lib, _abi.BIQUAD)
    _abi.bind(lib, _abi.ADAPTIVE)
    _abi.bind(lib, _abi.CMPLX_MAT)
    _abi.bind(lib, _abi.MAT_SOLVE)
    _abi.bind(lib, _abi.MAT_BASIC)
    _abi.bind(lib, _abi.CMPLX_MATH)
    _abi.bind(lib, _abi.STATISTICS)
    _abi.bind(lib, _abi.BASIC_MATH)
    _abi.bind(lib, _abi.SUPPORT)
    _abi.bind(lib, _abi.DISTANCE)
    _abi.bind(lib, _abi.ML)
    _abi.bind(lib, _abi.QUATERNION)
    _abi.bind(lib, _abi.INTERP)
    _abi.bind(lib, _abi.BATCHED)
    return lib


lib = _load()


def version():
    return lib.arm_mi355x_version().decode()


def last_error():
    return lib.arm_mi355x_last_error(), lib.arm_mi355x_last_error_string().decode()


def _check_void(what):
    code, msg = last_error()
    if code:
        lib.arm_mi355x_clear_error()
        raise RuntimeError(f"{what}: device error {code}: {msg}")


def const_instance(name):
    """A pre-initialised const instance exported by the library (arm_const_structs.h)."""
    kind = {"f32": arm_cfft_instance_f32, "q31": arm_cfft_instance_q31, "q15": arm_cfft_instance_q15}
    if name.startswith("arm_rfft_fast_sR_f32"):
        return arm_rfft_fast_instance_f32.in_dll(lib, name)
    return kind[name.split("_")[3]].in_dll(lib, name)


# ------------------------------------------------------------------ drop-in (numpy)
def arm_cfft_init_f32(S, n):
    return lib.arm_cfft_init_f32(C.byref(S), n)


def arm_cfft_init_q31(S, n):
    return lib.arm_cfft_init_q31(C.byref(S), n)


def arm_cfft_init_q15(S, n):
    return lib.arm_cfft_init_q15(C.byref(S), n)


def _cfft(fn, dtype, S, x, ifft, bitrev):
    buf = np.ascontiguousarray(x, dtype=dtype).copy()
    fn(C.byref(S), buf.ctypes.data, ifft, bitrev)
    _check_void(fn.__name__)
    return buf


def arm_cfft_f32(S, x, ifftFlag, bitReverseFlag):
    return _cfft(lib.arm_cfft_f32, np.float32, S, x, ifftFlag, bitReverseFlag)


def arm_cfft_q31(S, x, ifftFlag, bitReverseFlag):
    return _cfft(lib.arm_cfft_q31, np.int32, S, x, ifftFlag, bitReverseFlag)


def arm_cfft_q15(S, x, ifftFlag, bitReverseFlag):
    return _cfft(lib.arm_cfft_q15, np.int16, S, x, ifftFlag, bitReverseFlag)


def arm_rfft_fast_init_f32(S, n):
    return lib.arm_rfft_fast_init_f32(C.byref(S), n)


def arm_rfft_fast_f32(S, x, ifftFlag):
    """Returns the output; like the reference, the forward transform also destroys the
    input buffer (here a private copy)."""
    p = np.ascontiguousarray(x, dtype=np.float32).copy()
    out = np.zeros(S.fftLenRFFT, dtype=np.float32)
    lib.arm_rfft_fast_f32(C.byref(S), p.ctypes.data, out.ctypes.data, ifftFlag)
    _check_void("arm_rfft_fast_f32")
    return out


def arm_rfft_init_q31(S, n, ifftFlagR, bitReverseFlag):
    return lib.arm_rfft_init_q31(C.byref(S), n, ifftFlagR, bitReverseFlag)


def arm_rfft_init_q15(S, n, ifftFlagR, bitReverseFlag):
    return lib.arm_rfft_init_q15(C.byref(S), n, ifftFlagR, bitReverseFlag)


def _rfft_fixed(kind, S, x):
    dt = np.int32 if kind == "q31" else np.int16
    src = np.ascontiguousarray(x, dtype=dt).copy()
    n = S.fftLenReal
    out = np.zeros(n if S.ifftFlagR == 1 else 2 * n, dtype=dt)
    fn = getattr(lib, f"arm_rfft_{kind}")
    fn(C.byref(S), src.ctypes.data, out.ctypes.data)
    _check_void(fn.__name__)
    return out


def arm_rfft_q31(S, x):
    """Forward: N samples -> 2N-word spectrum; inverse: spectrum (>= N+2 words) -> N samples
    (arm_rfft_q31.c:148-183; the input copy is consumed as in the reference)."""
    return _rfft_fixed("q31", S, x)


def arm_rfft_q15(S, x):
    return _rfft_fixed("q15", S, x)


def rfft_fixed_batch(S, src, dst, stream=None):
    """Batched arm_rfft_q31 / _q15 on device tensors: forward src [batch, N] (overwritten)
    -> dst [batch, 2N]; inverse src [batch, 2N] -> dst [batch, N]."""
    kind = "q31" if isinstance(S, arm_rfft_instance_q31) else "q15"
    fn = getattr(lib, f"arm_rfft_{kind}_batch")
    st = fn(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), dst.shape[0], _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


class FirF32:
    """Streaming FIR f32 (arm_fir_init_f32 + arm_fir_f32): state carried across calls."""

    def __init__(self, coeffs, block_size):
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.float32)
        self.block_size = block_size
        self.state = np.zeros(len(self.coeffs) + block_size - 1, dtype=np.float32)
        self.S = arm_fir_instance_f32()
        lib.arm_fir_init_f32(C.byref(self.S), len(self.coeffs), self.coeffs.ctypes.data,
                             self.state.ctypes.data, block_size)

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert len(x) <= self.block_size
        y = np.empty_like(x)
        lib.arm_fir_f32(C.byref(self.S), x.ctypes.data, y.ctypes.data, len(x))
        _check_void("arm_fir_f32")
        return y


class FirQ15(FirF32):
    def __init__(self, coeffs, block_size):
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
        self.block_size = block_size
        self.state = np.zeros(len(self.coeffs) + block_size - 1, dtype=np.int16)
        self.S = arm_fir_instance_q15()
        lib.arm_fir_init_q15(C.byref(self.S), len(self.coeffs), self.coeffs.ctypes.data,
                             self.state.ctypes.data, block_size)

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.int16)
        y = np.empty_like(x)
        lib.arm_fir_q15(C.byref(self.S), x.ctypes.data, y.ctypes.data, len(x))
        _check_void("arm_fir_q15")
        return y


class FirQ31(FirF32):
    """Streaming arm_fir_q31 (fast=False) or arm_fir_fast_q31 (fast=True)."""

    def __init__(self, coeffs, block_size, fast=False):
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.int32)
        self.block_size = block_size
        self.fn = lib.arm_fir_fast_q31 if fast else lib.arm_fir_q31
        self.state = np.zeros(len(self.coeffs) + block_size - 1, dtype=np.int32)
        self.S = arm_fir_instance_q31()
        lib.arm_fir_init_q31(C.byref(self.S), len(self.coeffs), self.coeffs.ctypes.data,
                             self.state.ctypes.data, block_size)

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.int32)
        y = np.empty_like(x)
        self.fn(C.byref(self.S), x.ctypes.data, y.ctypes.data, len(x))
        _check_void(self.fn.__name__)
        return y


class FirQ7(FirF32):
    """Streaming arm_fir_q7."""

    def __init__(self, coeffs, block_size):
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.int8)
        self.block_size = block_size
        self.state = np.zeros(len(self.coeffs) + block_size - 1, dtype=np.int8)
        self.S = arm_fir_instance_q7()
        lib.arm_fir_init_q7(C.byref(self.S), len(self.coeffs), self.coeffs.ctypes.data,
                            self.state.ctypes.data, block_size)

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.int8)
        y = np.empty_like(x)
        lib.arm_fir_q7(C.byref(self.S), x.ctypes.data, y.ctypes.data, len(x))
        _check_void("arm_fir_q7")
        return y


class FirFastQ15(FirQ15):
    """Streaming arm_fir_fast_q15."""

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.int16)
        y = np.empty_like(x)
        lib.arm_fir_fast_q15(C.byref(self.S), x.ctypes.data, y.ctypes.data, len(x))
        _check_void("arm_fir_fast_q15")
        return y


def arm_mat_mult_f32(a, b):
    """(status, C) = A @ B through arm_mat_mult_f32 (row-major f32)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    c = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    A, B, Cm = arm_matrix_instance_f32(), arm_matrix_instance_f32(), arm_matrix_instance_f32()
    lib.arm_mat_init_f32(C.byref(A), a.shape[0], a.shape[1], a.ctypes.data)
    lib.arm_mat_init_f32(C.byref(B), b.shape[0], b.shape[1], b.ctypes.data)
    lib.arm_mat_init_f32(C.byref(Cm), c.shape[0], c.shape[1], c.ctypes.data)
    st = lib.arm_mat_mult_f32(C.byref(A), C.byref(B), C.byref(Cm))
    _check_void("arm_mat_mult_f32")
    return st, c


class MfccF32:
    """arm_mfcc_init_f32 + arm_mfcc_f32 with the instance's tables kept alive.
    dct: [nbDctOutputs, nbMelFilters]; pos/lengths: per Mel filter; coefs: concatenated
    filter weights; window: fftLen.  Tables may be numpy arrays (host) or torch device
    tensors (their data_ptr is used)."""

    def __init__(self, fft_len, dct, pos, lengths, coefs, window):
        def keep(a, dt):
            if hasattr(a, "data_ptr"):
                return a, a.data_ptr()
            a = np.ascontiguousarray(a, dtype=dt)
            return a, a.ctypes.data
        self._t = [keep(dct, np.float32), keep(pos, np.uint32), keep(lengths, np.uint32), keep(coefs, np.float32),
                   keep(window, np.float32)]
        self.nb_mel = int(len(lengths))
        self.nb_dct = int(dct.shape[0])
        self.fft_len = int(fft_len)
        self.S = arm_mfcc_instance_f32()
        st = lib.arm_mfcc_init_f32(C.byref(self.S), self.fft_len, self.nb_mel, self.nb_dct,
                                   *[p for _, p in self._t])
        if st != ARM_MATH_SUCCESS:
            raise ValueError(f"arm_mfcc_init_f32({fft_len}) -> {st}")

    def __call__(self, x):
        """One frame (numpy) -> nbDctOutputs coefficients (the reference's call shape)."""
        src = np.ascontiguousarray(x, dtype=np.float32).copy()
        dst = np.zeros(self.nb_dct, dtype=np.float32)
        tmp = np.zeros(2 * self.fft_len, dtype=np.float32)
        lib.arm_mfcc_f32(C.byref(self.S), src.ctypes.data, dst.ctypes.data, tmp.ctypes.data)
        _check_void("arm_mfcc_f32")
        return dst

    def batch(self, frames, out=None, work=None, stream=None):
        """frames: torch device tensor [batch, fftLen] (overwritten) -> [batch, nbDct]."""
        import torch
        b = frames.shape[0]
        out = torch.empty((b, self.nb_dct), dtype=torch.float32, device=frames.device) if out is None else out
        work = torch.empty_like(frames) if work is None else work
        st = lib.arm_mfcc_f32_batch(C.byref(self.S), C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr()),
                                    C.c_void_p(work.data_ptr()), b, _stream_ptr(stream))
        if st != ARM_MATH_SUCCESS:
            raise RuntimeError(f"arm_mfcc_f32_batch -> {st}: {last_error()[1]}")
        return out


class _MfccFixed:
    """arm_mfcc_init_<t> + arm_mfcc_<t> (bit-exact) with the instance's tables kept alive.
    dct: [nbDctOutputs, nbMelFilters]; pos/lengths: per Mel filter; coefs: concatenated filter
    weights; window: fftLen.  Tables: numpy (host) or torch device tensors."""
    T = None            # "q31" | "q15"

    def __init__(self, fft_len, dct, pos, lengths, coefs, window):
        dt = np.int32 if self.T == "q31" else np.int16

        def keep(a, d):
            if hasattr(a, "data_ptr"):
                return a, a.data_ptr()
            a = np.ascontiguousarray(a, dtype=d)
            return a, a.ctypes.data
        self._dt = dt
        self._t = [keep(dct, dt), keep(pos, np.uint32), keep(lengths, np.uint32), keep(coefs, dt), keep(window, dt)]
        self.nb_mel = int(len(lengths))
        self.nb_dct = int(dct.shape[0])
        self.fft_len = int(fft_len)
        self.S = (arm_mfcc_instance_q31 if self.T == "q31" else arm_mfcc_instance_q15)()
        st = getattr(lib, f"arm_mfcc_init_{self.T}")(C.byref(self.S), self.fft_len, self.nb_mel, self.nb_dct,
                                                     *[p for _, p in self._t])
        if st != ARM_MATH_SUCCESS:
            raise ValueError(f"arm_mfcc_init_{self.T}({fft_len}) -> {st}")

    def __call__(self, x):
        """One frame (numpy) -> nbDctOutputs coefficients (the reference's call shape)."""
        src = np.ascontiguousarray(x, dtype=self._dt).copy()
        dst = np.zeros(self.nb_dct, dtype=self._dt)
        tmp = np.zeros(2 * self.fft_len, dtype=np.int32)
        st = getattr(lib, f"arm_mfcc_{self.T}")(C.byref(self.S), src.ctypes.data, dst.ctypes.data, tmp.ctypes.data)
        if st != ARM_MATH_SUCCESS:
            raise RuntimeError(f"arm_mfcc_{self.T} -> {st}: {last_error()[1]}")
        return dst

    def batch(self, frames, out=None, work=None, stream=None):
        """frames: torch device tensor [batch, fftLen] (int32 / int16, overwritten) -> [batch, nbDct]."""
        import torch
        b = frames.shape[0]
        out = torch.empty((b, self.nb_dct), dtype=frames.dtype, device=frames.device) if out is None else out
        work = torch.empty((b, 2 * self.fft_len), dtype=frames.dtype, device=frames.device) if work is None else work
        st = getattr(lib, f"arm_mfcc_{self.T}_batch")(C.byref(self.S), C.c_void_p(frames.data_ptr()),
                                                      C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), b,
                                                      _stream_ptr(stream))
        if st != ARM_MATH_SUCCESS:
            raise RuntimeError(f"arm_mfcc_{self.T}_batch -> {st}: {last_error()[1]}")
        return out


class MfccQ31(_MfccFixed):
    """arm_mfcc_q31: q31 frames -> q8.23 coefficients."""
    T = "q31"


class MfccQ15(_MfccFixed):
    """arm_mfcc_q15: q15 frames -> q8.7 coefficients."""
    T = "q15"


# ------------------------------------------------------------------ batched (torch, device)
def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


_CFFT_BATCH = {"f32": ("arm_cfft_f32_batch", 2), "q31": ("arm_cfft_q31_batch", 2),
               "q15": ("arm_cfft_q15_batch", 2)}


def cfft_batch(S, data, ifft, bitrev, stream=None, kind=None):
    """In-place CFFT of every row of `data` (torch device tensor [batch, 2*N])."""
    if kind is None:
        kind = {arm_cfft_instance_f32: "f32", arm_cfft_instance_q31: "q31",
                arm_cfft_instance_q15: "q15"}[type(S)]
    fn = getattr(lib, _CFFT_BATCH[kind][0])
    batch = data.numel() // (2 * S.fftLen)
    st = fn(C.byref(S), C.c_void_p(data.data_ptr()), batch, ifft, bitrev, _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def cfft_batch_multi(S, shards, ifft, bitrev, kind=None):
    """In-place CFFT of every row of every tensor in `shards` (torch tensors [batch_s, 2*N],
    each on its own device) through one arm_cfft_*_batch_multi call (synchronous)."""
    if kind is None:
        kind = {arm_cfft_instance_f32: "f32", arm_cfft_instance_q31: "q31",
                arm_cfft_instance_q15: "q15"}[type(S)]
    k = len(shards)
    # the C side runs each shard on the library's own stream of that device: order it after
    # whatever torch work is still producing the shards
    import torch
    for d in sorted({t.device.index for t in shards}):
        torch.cuda.synchronize(d)
    devs = (C.c_int * k)(*[t.device.index for t in shards])
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in shards])
    cnts = (C.c_uint32 * k)(*[t.numel() // (2 * S.fftLen) for t in shards])
    fn = getattr(lib, f"arm_cfft_{kind}_batch_multi")
    st = fn(C.byref(S), k, devs, ptrs, cnts, ifft, bitrev)
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def device_count():
    return lib.arm_mi355x_device_count()


def table_cache_bytes():
    """Device bytes held by the content-keyed cache of host tables / coefficients."""
    return lib.arm_mi355x_table_cache_bytes()


def set_table_cache_limit(nbytes):
    lib.arm_mi355x_set_table_cache_limit(C.c_size_t(nbytes))


def release_thread_resources():
    """Free the calling thread's drop-in streams, scratch and staging now (automatic at the exit
    of any thread but the main one)."""
    lib.arm_mi355x_release_thread_resources()


def thread_resource_owners():
    """Number of threads currently holding per-thread runtime resources."""
    return lib.arm_mi355x_thread_resource_owners()


RFFT_P_SCRATCH = 1     # ARM_MI355X_RFFT_P_SCRATCH


def rfft_fast_batch(S, p, out, ifft, stream=None, p_scratch=False):
    """Batched arm_rfft_fast_f32; p_scratch=True: arm_rfft_fast_f32_batch_ex with
    ARM_MI355X_RFFT_P_SCRATCH (p is scratch, the forward skips writing the inner CFFT back)."""
    batch = p.numel() // S.fftLenRFFT
    if p_scratch:
        st = lib.arm_rfft_fast_f32_batch_ex(C.byref(S), C.c_void_p(p.data_ptr()), C.c_void_p(out.data_ptr()),
                                            batch, ifft, RFFT_P_SCRATCH, _stream_ptr(stream))
    else:
        st = lib.arm_rfft_fast_f32_batch(C.byref(S), C.c_void_p(p.data_ptr()), C.c_void_p(out.data_ptr()), batch,
                                         ifft, _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"arm_rfft_fast_f32_batch -> {st}: {last_error()[1]}")


_FIR_BATCH = {"f32": "arm_fir_f32_batch", "f32_fma": "arm_fir_f32_batch_fma", "q15": "arm_fir_q15_batch",
              "q31": "arm_fir_q31_batch",
              "fast_q15": "arm_fir_fast_q15_batch", "fast_q31": "arm_fir_fast_q31_batch", "q7": "arm_fir_q7_batch"}


def fir_batch(S, src, dst, hist, stream=None, q15=False, kind=None):
    """src/dst: [batch, blockSize] device tensors; hist: [batch, numTaps-1] device state.
    kind: f32 | f32_fma (opt-in tolerance path) | q15 | q31 | fast_q15 | fast_q31 | q7 (default from
    the instance type / q15 flag)."""
    if kind is None:
        kind = "q15" if q15 else {arm_fir_instance_f32: "f32", arm_fir_instance_q15: "q15",
                                  arm_fir_instance_q31: "q31", arm_fir_instance_q7: "q7"}[type(S)]
    batch, block = src.shape
    fn = getattr(lib, _FIR_BATCH[kind])
    st = fn(C.byref(S), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), block, batch,
            C.c_void_p(hist.data_ptr() if hist is not None and hist.numel() else 0), _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def fir_batch_multi(S, shards, kind=None):
    """FIR over filter shards on several devices through one arm_fir_*_batch_multi call
    (synchronous): shards = [(src, dst, hist), ...], torch tensors [batch_s, blockSize] /
    [batch_s, numTaps-1] on each shard's device."""
    import torch
    if kind is None:
        kind = {arm_fir_instance_f32: "f32", arm_fir_instance_q15: "q15",
                arm_fir_instance_q31: "q31", arm_fir_instance_q7: "q7"}[type(S)]
    k = len(shards)
    for d in sorted({t[0].device.index for t in shards}):
        torch.cuda.synchronize(d)
    block = shards[0][0].shape[1] if k else 0
    devs = (C.c_int * k)(*[t[0].device.index for t in shards])
    src = (C.c_void_p * k)(*[t[0].data_ptr() for t in shards])
    dst = (C.c_void_p * k)(*[t[1].data_ptr() for t in shards])
    hist = (C.c_void_p * k)(*[t[2].data_ptr() if t[2] is not None and t[2].numel() else 0 for t in shards])
    cnts = (C.c_uint32 * k)(*[t[0].shape[0] for t in shards])
    fn = getattr(lib, f"arm_fir_{kind}_batch_multi")
    st = fn(C.byref(S), k, devs, src, dst, hist, block, cnts)
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def mat_mult_batch_multi(shards):
    """c[i] = a[i] @ b[i] per shard through one arm_mat_mult_*_batch_multi call (synchronous):
    shards = [(a, b, c), ...] with [batch_s, M, K] x [batch_s, K, N] -> [batch_s, M, N] tensors
    on each shard's device (f32 / int16 / int32)."""
    import torch
    a0, b0, _ = shards[0]
    m, k_, n = a0.shape[1], a0.shape[2], b0.shape[2]
    kind, inst = {torch.float32: ("f32", arm_matrix_instance_f32), torch.int16: ("q15", arm_matrix_instance_q15),
                  torch.int32: ("q31", arm_matrix_instance_q31), torch.int8: ("q7", arm_matrix_instance_q7)}[a0.dtype]
    for d in sorted({t[0].device.index for t in shards}):
        torch.cuda.synchronize(d)
    k = len(shards)
    A, B, Cm = inst(m, k_, None), inst(k_, n, None), inst(m, n, None)
    devs = (C.c_int * k)(*[t[0].device.index for t in shards])
    pa, pb, pc = ((C.c_void_p * k)(*[t[i].data_ptr() for t in shards]) for i in range(3))
    cnts = (C.c_uint32 * k)(*[t[0].shape[0] for t in shards])
    fn = getattr(lib, f"arm_mat_mult_{kind}_batch_multi")
    st = fn(C.byref(A), C.byref(B), C.byref(Cm), k, devs, pa, pb, pc, cnts)
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def mat_cmplx_mult_batch_multi(shards):
    """The complex product per shard through one arm_mat_cmplx_mult_*_batch_multi call (synchronous):
    shards = [(a, b, c), ...] with [batch_s, M, 2K] x [batch_s, K, 2N] -> [batch_s, M, 2N] tensors of
    interleaved (re, im) words on each shard's device (f32 / int16 / int32)."""
    import torch
    a0, b0, _ = shards[0]
    m, k_, n = a0.shape[1], b0.shape[1], b0.shape[2] // 2
    kind = {torch.float32: "f32", torch.int16: "q15", torch.int32: "q31"}[a0.dtype]
    inst = _abi.CMPLX_MAT_INST[kind]
    for d in sorted({t[0].device.index for t in shards}):
        torch.cuda.synchronize(d)
    k = len(shards)
    A, B, Cm = inst(m, a0.shape[2] // 2, None), inst(k_, n, None), inst(m, n, None)
    devs = (C.c_int * k)(*[t[0].device.index for t in shards])
    pa, pb, pc = ((C.c_void_p * k)(*[t[i].data_ptr() for t in shards]) for i in range(3))
    cnts = (C.c_uint32 * k)(*[t[0].shape[0] for t in shards])
    fn = getattr(lib, f"arm_mat_cmplx_mult_{kind}_batch_multi")
    st = fn(C.byref(A), C.byref(B), C.byref(Cm), k, devs, pa, pb, pc, cnts)
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def arm_conv(kind, a, b):
    """arm_conv_f32 / _q15 / _q31 / _q7 (drop-in, numpy): len(a) + len(b) - 1 samples."""
    dt = {"f32": np.float32, "q15": np.int16, "q31": np.int32, "q7": np.int8}[kind]
    a = np.ascontiguousarray(a, dtype=dt)
    b = np.ascontiguousarray(b, dtype=dt)
    y = np.zeros(len(a) + len(b) - 1, dtype=dt)
    getattr(lib, f"arm_conv_{kind}")(a.ctypes.data, len(a), b.ctypes.data, len(b), y.ctypes.data)
    _check_void(f"arm_conv_{kind}")
    return y


def conv_batch(a, b, out, stream=None):
    """out[i] = a[i] (*) b[i]; a [batch, La], b [batch, Lb] or [Lb] (shared), out [batch, La+Lb-1]."""
    import torch
    kind = {torch.float32: "f32", torch.int16: "q15", torch.int32: "q31", torch.int8: "q7"}[a.dtype]
    batch, la = a.shape
    lb = b.shape[-1]
    sb = 0 if b.dim() == 1 else b.stride(0)
    fn = getattr(lib, f"arm_conv_{kind}_batch")
    st = fn(C.c_void_p(a.data_ptr()), la, a.stride(0), C.c_void_p(b.data_ptr()), lb, sb,
            C.c_void_p(out.data_ptr()), batch, _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def arm_conv_family(fn, a, b, first=0, num=0, fill=0):
    """Drop-in (numpy) call of arm_<fn>, fn in _abi.CONV_FULL + _abi.CONV_PARTIAL (e.g.
    "correlate_q15", "conv_partial_f32", "conv_fast_q31"): returns (pDst, status); pDst is
    pre-filled with `fill`, since partial / correlate leave the words they do not compute."""
    dt = {"f32": np.float32, "q15": np.int16, "q31": np.int32, "q7": np.int8}[fn.split("_")[-1]]
    a = np.ascontiguousarray(a, dtype=dt)
    b = np.ascontiguousarray(b, dtype=dt)
    n = 2 * max(len(a), len(b)) - 1 if fn.startswith("correlate") else len(a) + len(b) - 1
    y = np.full(n, fill, dtype=dt)
    f = getattr(lib, f"arm_{fn}")
    if fn.startswith("conv_partial"):
        st = f(a.ctypes.data, len(a), b.ctypes.data, len(b), y.ctypes.data, first, num)
    else:
        f(a.ctypes.data, len(a), b.ctypes.data, len(b), y.ctypes.data)
        st = ARM_MATH_SUCCESS
    _check_void(f"arm_{fn}")
    return y, st


def conv_family_batch(fn, a, b, out, first=0, num=0, stream=None):
    """arm_<fn>_batch on torch device tensors: a [batch, La], b [batch, Lb] or [Lb] (shared),
    out [batch, La+Lb-1] (conv), [batch, 2*max-1] (correlate) or [batch, num] (partial)."""
    batch, la = a.shape
    lb = b.shape[-1]
    sb = 0 if b.dim() == 1 else b.stride(0)
    fn_ = getattr(lib, f"arm_{fn}_batch")
    args = [C.c_void_p(a.data_ptr()), la, a.stride(0), C.c_void_p(b.data_ptr()), lb, sb, C.c_void_p(out.data_ptr())]
    if fn.startswith("conv_partial"):
        args += [first, num]
    st = fn_(*args, batch, _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"arm_{fn}_batch -> {st}: {last_error()[1]}")


def arm_mat_mult_fixed(kind, a, b):
    """(status, C) = A @ B through arm_mat_mult_q7 / _q15 / _q31 / _fast_q15 / _fast_q31 (kind
    "q7", "q15", "q31", "opt_q31", "fast_q15", "fast_q31"; row-major)."""
    base = "q7" if kind == "q7" else kind[-3:]
    dt = {"q7": np.int8, "q15": np.int16, "q31": np.int32}[base]
    inst = {"q7": arm_matrix_instance_q7, "q15": arm_matrix_instance_q15, "q31": arm_matrix_instance_q31}[base]
    a = np.ascontiguousarray(a, dtype=dt)
    b = np.ascontiguousarray(b, dtype=dt)
    c = np.zeros((a.shape[0], b.shape[1]), dtype=dt)
    A, B, Cm = inst(), inst(), inst()
    init = getattr(lib, f"arm_mat_init_{base}")
    init(C.byref(A), a.shape[0], a.shape[1], a.ctypes.data)
    init(C.byref(B), b.shape[0], b.shape[1], b.ctypes.data)
    init(C.byref(Cm), c.shape[0], c.shape[1], c.ctypes.data)
    fn = getattr(lib, f"arm_mat_mult_{kind}")
    st = fn(C.byref(A), C.byref(B), C.byref(Cm), None) if base in ("q15", "q7") or kind == "opt_q31" else \
        fn(C.byref(A), C.byref(B), C.byref(Cm))
    _check_void(f"arm_mat_mult_{kind}")
    return st, c


def arm_mat_cmplx_mult(kind, a, b, scratch=None):
    """(status, C) through arm_mat_cmplx_mult_f32 / _q31 / _q15 (kind "f32", "q31", "q15"): a [M, 2K] and
    b [K, 2N] hold interleaved (re, im) words, C is [M, 2N].  scratch (q15 only): an int16 array of
    2 K N words that receives B transposed, as the reference's pScratch does; None passes NULL."""
    dt = {"f32": np.float32, "q15": np.int16, "q31": np.int32}[kind]
    inst = _abi.CMPLX_MAT_INST[kind]
    a = np.ascontiguousarray(a, dtype=dt)
    b = np.ascontiguousarray(b, dtype=dt)
    c = np.zeros((a.shape[0], b.shape[1]), dtype=dt)
    ptr = {"f32": _abi.c_f32p, "q15": _abi.c_i16p, "q31": _abi.c_i32p}[kind]
    A, B, Cm = (inst(x.shape[0], x.shape[1] // 2, C.cast(x.ctypes.data, ptr)) for x in (a, b, c))
    fn = getattr(lib, f"arm_mat_cmplx_mult_{kind}")
    args = [C.byref(A), C.byref(B), C.byref(Cm)]
    if kind == "q15":
        args.append(None if scratch is None else scratch.ctypes.data)
    st = fn(*args)
    _check_void(f"arm_mat_cmplx_mult_{kind}")
    return st, c


def mat_cmplx_mult_batch(a, b, c, stream=None):
    """The complex product c[i] = a[i] b[i] for device tensors [batch, M, 2K] x [batch, K, 2N] ->
    [batch, M, 2N] of interleaved (re, im) words; float32 -> arm_mat_cmplx_mult_f32_batch, int16 -> _q15,
    int32 -> _q31."""
    import torch
    batch, m, k2 = a.shape
    n2 = b.shape[2]
    kind, ptr = {torch.float32: ("f32", _abi.c_f32p), torch.int16: ("q15", _abi.c_i16p),
                 torch.int32: ("q31", _abi.c_i32p)}[a.dtype]
    inst = _abi.CMPLX_MAT_INST[kind]
    A, B, Cm = inst(m, k2 // 2, C.cast(a.data_ptr(), ptr)), inst(b.shape[1], n2 // 2, C.cast(b.data_ptr(), ptr)), \
        inst(c.shape[1], c.shape[2] // 2, C.cast(c.data_ptr(), ptr))
    fn = getattr(lib, f"arm_mat_cmplx_mult_{kind}_batch")
    st = fn(C.byref(A), C.byref(B), C.byref(Cm), batch, _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")


def _matf(x):
    """arm_matrix_instance_f32 over a 2-D numpy array (its own shape) or the items of a [batch, r, c] tensor."""
    if isinstance(x, np.ndarray):
        return _abi.arm_matrix_instance_f32(x.shape[0], x.shape[1], C.cast(x.ctypes.data, _abi.c_f32p))
    return _abi.arm_matrix_instance_f32(x.shape[-2], x.shape[-1], C.cast(x.data_ptr(), _abi.c_f32p))


def arm_mat_inverse(src):
    """(status, dst) through arm_mat_inverse_f32 (drop-in, numpy).  The call destroys its copy of src."""
    s = np.array(src, dtype=np.float32, order="C")
    d = np.zeros_like(s)
    st = lib.arm_mat_inverse_f32(C.byref(_matf(s)), C.byref(_matf(d)))
    _check_void("arm_mat_inverse_f32")
    return st, d


def arm_mat_cholesky(src):
    """(status, dst) through arm_mat_cholesky_f32: dst starts as zeros, so its strict upper triangle is zero."""
    s = np.ascontiguousarray(src, dtype=np.float32)
    d = np.zeros_like(s)
    st = lib.arm_mat_cholesky_f32(C.byref(_matf(s)), C.byref(_matf(d)))
    _check_void("arm_mat_cholesky_f32")
    return st, d


def arm_mat_ldlt(src):
    """(status, l, d, pp) through arm_mat_ldlt_f32: P A P^T = L D L^T, pp the uint16 pivot of each step."""
    s = np.ascontiguousarray(src, dtype=np.float32)
    l, d = np.zeros_like(s), np.zeros_like(s)
    pp = np.zeros(s.shape[0], dtype=np.uint16)
    st = lib.arm_mat_ldlt_f32(C.byref(_matf(s)), C.byref(_matf(l)), C.byref(_matf(d)), pp.ctypes.data)
    _check_void("arm_mat_ldlt_f32")
    return st, l, d, pp


def _arm_mat_solve(fn, t, a):
    t = np.ascontiguousarray(t, dtype=np.float32)
    a = np.ascontiguousarray(a, dtype=np.float32)
    x = np.zeros_like(a)
    st = getattr(lib, fn)(C.byref(_matf(t)), C.byref(_matf(a)), C.byref(_matf(x)))
    _check_void(fn)
    return st, x


def arm_mat_solve_lower_triangular(lt, a):
    """(status, x) with lt x = a through arm_mat_solve_lower_triangular_f32; a is [n, cols]."""
    return _arm_mat_solve("arm_mat_solve_lower_triangular_f32", lt, a)


def arm_mat_solve_upper_triangular(ut, a):
    """(status, x) with ut x = a through arm_mat_solve_upper_triangular_f32; a is [n, cols]."""
    return _arm_mat_solve("arm_mat_solve_upper_triangular_f32", ut, a)


def _solve_status(ref, status):
    import torch
    if status is None:
        status = torch.empty(ref.shape[0], dtype=torch.int32, device=ref.device)
    return status, C.c_void_p(status.data_ptr() if status is not False else None)


def _solve_call(name, *args):
    st = getattr(lib, name)(*args)
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{name} -> {st}: {last_error()[1]}")


def mat_inverse_batch(src, dst, status=None, stream=None):
    """dst[i] = inverse(src[i]) for contiguous float32 device tensors [batch, n, n] (arm_mat_inverse_f32_batch);
    src is destroyed as by the reference.  Returns the per-item int32 status tensor (status: a tensor to fill,
    None to allocate one, False to pass NULL and return None)."""
    status, ps = _solve_status(src, status)
    _solve_call("arm_mat_inverse_f32_batch", C.byref(_matf(src)), C.byref(_matf(dst)), src.shape[0], ps,
                _stream_ptr(stream))
    return None if status is False else status


def mat_cholesky_batch(src, dst, status=None, stream=None):
    """The lower triangle of dst[i] = cholesky(src[i]) (arm_mat_cholesky_f32_batch); dst may be src."""
    status, ps = _solve_status(src, status)
    _solve_call("arm_mat_cholesky_f32_batch", C.byref(_matf(src)), C.byref(_matf(dst)), src.shape[0], ps,
                _stream_ptr(stream))
    return None if status is False else status


def mat_ldlt_batch(src, l, d, pp, stream=None):
    """l[i], d[i], pp[i] = ldlt(src[i]) (arm_mat_ldlt_f32_batch); pp is an int16 / uint16 tensor [batch, n]
    holding the uint16 pivots.  Every item succeeds, as in the reference."""
    _solve_call("arm_mat_ldlt_f32_batch", C.byref(_matf(src)), C.byref(_matf(l)), C.byref(_matf(d)),
                C.c_void_p(pp.data_ptr()), src.shape[0], _stream_ptr(stream))


def mat_solve_triangular_batch(t, a, dst, lower, status=None, stream=None):
    """t[i] dst[i] = a[i] for device tensors t [batch, n, n], a and dst [batch, n, cols]
    (arm_mat_solve_{lower,upper}_triangular_f32_batch); dst may be a.  Returns the status tensor as
    mat_inverse_batch does."""
    status, ps = _solve_status(t, status)
    _solve_call(f"arm_mat_solve_{'lower' if lower else 'upper'}_triangular_f32_batch", C.byref(_matf(t)),
                C.byref(_matf(a)), C.byref(_matf(dst)), t.shape[0], ps, _stream_ptr(stream))
    return None if status is False else status


_MAT_DT = {"f32": np.float32, "q31": np.int32, "q15": np.int16, "q7": np.int8}


def _mat(kind, x, cmplx=False):
    """arm_matrix_instance_<kind> over a 2-D numpy array or over the items of a [batch, r, c] tensor; cmplx: the
    last axis holds interleaved (re, im) words and numCols counts pairs."""
    p = x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
    return _abi.MAT_INST[kind](x.shape[-2], x.shape[-1] // (2 if cmplx else 1), C.cast(p, _abi.MAT_PTR[kind]))


def _mat_kind(t):
    import torch
    return {torch.float32: "f32", torch.int32: "q31", torch.int16: "q15", torch.int8: "q7"}[t.dtype]


def _arm_mat_ew(op, kind, a, b):
    a = np.ascontiguousarray(a, dtype=_MAT_DT[kind])
    b = np.ascontiguousarray(b, dtype=_MAT_DT[kind])
    d = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
    st = getattr(lib, f"arm_mat_{op}_{kind}")(C.byref(_mat(kind, a)), C.byref(_mat(kind, b)), C.byref(_mat(kind, d)))
    _check_void(f"arm_mat_{op}_{kind}")
    return st, d


def arm_mat_add(kind, a, b):
    """(status, a + b) through arm_mat_add_f32 / _q31 / _q15 (kind "f32", "q31", "q15"; drop-in, numpy).  dst is
    [a rows, b cols], as the reference binding sizes it."""
    return _arm_mat_ew("add", kind, a, b)


def arm_mat_sub(kind, a, b):
    """(status, a - b) through arm_mat_sub_f32 / _q31 / _q15."""
    return _arm_mat_ew("sub", kind, a, b)


def arm_mat_scale(kind, a, scale, shift=0):
    """(status, dst) through arm_mat_scale_f32 (scale a float) or _q31 / _q15 (scale the scaleFract word, shift
    -1..30 / -16..15; outside it the status is ARM_MATH_ARGUMENT_ERROR and dst stays zero)."""
    a = np.ascontiguousarray(a, dtype=_MAT_DT[kind])
    d = np.zeros_like(a)
    args = [float(scale)] if kind == "f32" else [int(scale), int(shift)]
    st = getattr(lib, f"arm_mat_scale_{kind}")(C.byref(_mat(kind, a)), *args, C.byref(_mat(kind, d)))
    _check_void(f"arm_mat_scale_{kind}")
    return st, d


def arm_mat_trans(kind, a):
    """(status, a.T) through arm_mat_trans_f32 / _q31 / _q15 / _q7."""
    a = np.ascontiguousarray(a, dtype=_MAT_DT[kind])
    d = np.zeros(a.shape[::-1], dtype=a.dtype)
    st = getattr(lib, f"arm_mat_trans_{kind}")(C.byref(_mat(kind, a)), C.byref(_mat(kind, d)))
    _check_void(f"arm_mat_trans_{kind}")
    return st, d


def arm_mat_cmplx_trans(kind, a):
    """(status, dst) through arm_mat_cmplx_trans_f32 / _q31 / _q15: a [R, 2C] holds interleaved (re, im) words,
    dst is [C, 2R]; no conjugation."""
    a = np.ascontiguousarray(a, dtype=_MAT_DT[kind])
    d = np.zeros((a.shape[1] // 2, 2 * a.shape[0]), dtype=a.dtype)
    st = getattr(lib, f"arm_mat_cmplx_trans_{kind}")(C.byref(_mat(kind, a, True)), C.byref(_mat(kind, d, True)))
    _check_void(f"arm_mat_cmplx_trans_{kind}")
    return st, d


def arm_mat_vec_mult(kind, m, v):
    """m [R, C] times v [C] -> [R] through arm_mat_vec_mult_f32 / _q31 / _q15 / _q7."""
    m = np.ascontiguousarray(m, dtype=_MAT_DT[kind])
    v = np.ascontiguousarray(v, dtype=_MAT_DT[kind])
    if v.size < m.shape[1]:
        raise ValueError(f"arm_mat_vec_mult_{kind}: the vector has {v.size} words, the matrix {m.shape[1]} columns")
    d = np.zeros(m.shape[0], dtype=m.dtype)
    getattr(lib, f"arm_mat_vec_mult_{kind}")(C.byref(_mat(kind, m)), v.ctypes.data, d.ctypes.data)
    _check_void(f"arm_mat_vec_mult_{kind}")
    return d


def _mat_ew_batch(op, a, b, dst, stream):
    kind = _mat_kind(a)
    _solve_call(f"arm_mat_{op}_{kind}_batch", C.byref(_mat(kind, a)), C.byref(_mat(kind, b)), C.byref(_mat(kind, dst)),
                a.shape[0], _stream_ptr(stream))


def mat_add_batch(a, b, dst, stream=None):
    """dst[i] = a[i] + b[i] for contiguous device tensors [batch, R, C] of float32 / int32 (q31) / int16 (q15)
    (arm_mat_add_*_batch); dst may be a or b."""
    _mat_ew_batch("add", a, b, dst, stream)


def mat_sub_batch(a, b, dst, stream=None):
    """dst[i] = a[i] - b[i] (arm_mat_sub_*_batch); dst may be a or b."""
    _mat_ew_batch("sub", a, b, dst, stream)


def mat_scale_batch(src, scale, dst, shift=0, stream=None):
    """dst[i] = src[i] scaled by one scale (fixed point: scaleFract and shift) for the whole batch
    (arm_mat_scale_*_batch); dst may be src."""
    kind = _mat_kind(src)
    args = [float(scale)] if kind == "f32" else [int(scale), int(shift)]
    _solve_call(f"arm_mat_scale_{kind}_batch", C.byref(_mat(kind, src)), *args, C.byref(_mat(kind, dst)),
                src.shape[0], _stream_ptr(stream))


def mat_trans_batch(src, dst, stream=None):
    """dst[i] [C, R] = the transpose of src[i] [R, C] (arm_mat_trans_*_batch; float32, int32, int16, int8)."""
    kind = _mat_kind(src)
    _solve_call(f"arm_mat_trans_{kind}_batch", C.byref(_mat(kind, src)), C.byref(_mat(kind, dst)), src.shape[0],
                _stream_ptr(stream))


def mat_cmplx_trans_batch(src, dst, stream=None):
    """dst[i] [C, 2R] = the transpose of src[i] [R, 2C], interleaved (re, im) words
    (arm_mat_cmplx_trans_*_batch; float32, int32, int16)."""
    kind = _mat_kind(src)
    _solve_call(f"arm_mat_cmplx_trans_{kind}_batch", C.byref(_mat(kind, src, True)), C.byref(_mat(kind, dst, True)),
                src.shape[0], _stream_ptr(stream))


def mat_vec_mult_batch(mat, vec, dst, stream=None, mat_stride=None):
    """dst[i] [R] = mat_i [R, C] times vec[i] [C] for device tensors vec [batch, C], dst [batch, R]
    (arm_mat_vec_mult_*_batch).  mat [R, C]: one matrix for every item (matStride 0); mat [batch, R, C]: one per
    item.  mat_stride (elements) overrides the distance between the items' matrices (a padded layout)."""
    kind = _mat_kind(mat)
    if mat_stride is None:
        mat_stride = 0 if mat.dim() == 2 else mat.shape[-2] * mat.shape[-1]
    _solve_call(f"arm_mat_vec_mult_{kind}_batch", C.byref(_mat(kind, mat)), int(mat_stride),
                C.c_void_p(vec.data_ptr()), C.c_void_p(dst.data_ptr()), vec.shape[0], _stream_ptr(stream))


# ---- complex math, max / min ------------------------------------------------------------------------------
_DOT_DT = {"f32": np.float32, "q31": np.int64, "q15": np.int32}


def _cm_src(kind, x):
    return np.ascontiguousarray(x, dtype=_MAT_DT[kind]).reshape(-1)


def _arm_cmplx_1(op, kind, src, words):
    s = _cm_src(kind, src)
    n = s.size // 2
    d = np.zeros(n * words, dtype=s.dtype)
    getattr(lib, f"arm_cmplx_{op}_{kind}")(s.ctypes.data, d.ctypes.data, n)
    _check_void(f"arm_cmplx_{op}_{kind}")
    return d


def arm_cmplx_mag(kind, src):
    """|z| of every interleaved (re, im) pair of src through arm_cmplx_mag_f32 / _q31 / _q15 (drop-in, numpy)."""
    return _arm_cmplx_1("mag", kind, src, 1)


def arm_cmplx_mag_squared(kind, src):
    """re^2 + im^2 of every pair through arm_cmplx_mag_squared_f32 / _q31 / _q15."""
    return _arm_cmplx_1("mag_squared", kind, src, 1)


def arm_cmplx_conj(kind, src):
    """The conjugate of every pair through arm_cmplx_conj_f32 / _q31 / _q15."""
    return _arm_cmplx_1("conj", kind, src, 2)


def arm_cmplx_mult_cmplx(kind, a, b):
    """a[k] * b[k] for interleaved complex vectors through arm_cmplx_mult_cmplx_f32 / _q31 / _q15."""
    a, b = _cm_src(kind, a), _cm_src(kind, b)
    if b.size < a.size:
        raise ValueError(f"arm_cmplx_mult_cmplx_{kind}: pSrcB has {b.size} words, pSrcA {a.size}")
    d = np.zeros(a.size // 2 * 2, dtype=a.dtype)
    getattr(lib, f"arm_cmplx_mult_cmplx_{kind}")(a.ctypes.data, b.ctypes.data, d.ctypes.data, a.size // 2)
    _check_void(f"arm_cmplx_mult_cmplx_{kind}")
    return d


def arm_cmplx_mult_real(kind, cmplx, real):
    """cmplx[k] * real[k] (a complex by a real vector) through arm_cmplx_mult_real_f32 / _q31 / _q15."""
    a, r = _cm_src(kind, cmplx), _cm_src(kind, real)
    if r.size < a.size // 2:
        raise ValueError(f"arm_cmplx_mult_real_{kind}: pSrcReal has {r.size} words, pSrcCmplx {a.size // 2} samples")
    d = np.zeros(a.size // 2 * 2, dtype=a.dtype)
    getattr(lib, f"arm_cmplx_mult_real_{kind}")(a.ctypes.data, r.ctypes.data, d.ctypes.data, a.size // 2)
    _check_void(f"arm_cmplx_mult_real_{kind}")
    return d


def arm_cmplx_dot_prod(kind, a, b):
    """(real, imag) of sum a[k] * b[k] through arm_cmplx_dot_prod_f32 (float32) / _q31 (int64) / _q15 (int32)."""
    a, b = _cm_src(kind, a), _cm_src(kind, b)
    if b.size < a.size:
        raise ValueError(f"arm_cmplx_dot_prod_{kind}: pSrcB has {b.size} words, pSrcA {a.size}")
    out = np.zeros(2, dtype=_DOT_DT[kind])
    getattr(lib, f"arm_cmplx_dot_prod_{kind}")(a.ctypes.data, b.ctypes.data, a.size // 2, out[0:].ctypes.data,
                                               out[1:].ctypes.data)
    _check_void(f"arm_cmplx_dot_prod_{kind}")
    return out[0], out[1]


def _arm_search(op, kind, src):
    s = _cm_src(kind, src)
    if s.size == 0:
        raise ValueError(f"arm_{op}_{kind}: an empty vector has no {op}imum")
    val, idx = np.zeros(1, dtype=s.dtype), np.zeros(1, dtype=np.uint32)
    getattr(lib, f"arm_{op}_{kind}")(s.ctypes.data, s.size, val.ctypes.data, idx.ctypes.data)
    _check_void(f"arm_{op}_{kind}")
    return val[0], idx[0]


def arm_max(kind, src):
    """(value, index) of the maximum, the first index on a tie, through arm_max_f32 / _q31 / _q15 / _q7."""
    return _arm_search("max", kind, src)


def arm_min(kind, src):
    """(value, index) of the minimum, the first index on a tie, through arm_min_f32 / _q31 / _q15 / _q7."""
    return _arm_search("min", kind, src)


def _cm_ptr(t):
    return C.c_void_p(t.data_ptr())


def _cmplx_1_batch(op, src, dst, stream):
    kind = _mat_kind(src)
    _solve_call(f"arm_cmplx_{op}_{kind}_batch", _cm_ptr(src), _cm_ptr(dst), src.shape[-1] // 2, src.shape[0],
                _stream_ptr(stream))


def cmplx_mag_batch(src, dst, stream=None):
    """dst[i] [N] = |src[i]| for contiguous device tensors src [batch, 2N] of interleaved (re, im) float32 / int32
    (q31) / int16 (q15) words (arm_cmplx_mag_*_batch).  dst must not overlap src."""
    _cmplx_1_batch("mag", src, dst, stream)


def cmplx_mag_squared_batch(src, dst, stream=None):
    """dst[i] [N] = re^2 + im^2 of src[i] [2N] (arm_cmplx_mag_squared_*_batch)."""
    _cmplx_1_batch("mag_squared", src, dst, stream)


def cmplx_conj_batch(src, dst, stream=None):
    """dst[i] [2N] = the conjugate of src[i] [2N] (arm_cmplx_conj_*_batch); dst may be src."""
    _cmplx_1_batch("conj", src, dst, stream)


def cmplx_mult_cmplx_batch(a, b, dst, stream=None):
    """dst[i] [2N] = a[i] * b[i], element by element (arm_cmplx_mult_cmplx_*_batch); dst may be a or b."""
    kind = _mat_kind(a)
    _solve_call(f"arm_cmplx_mult_cmplx_{kind}_batch", _cm_ptr(a), _cm_ptr(b), _cm_ptr(dst), a.shape[-1] // 2,
                a.shape[0], _stream_ptr(stream))


def cmplx_mult_real_batch(cmplx, real, dst, stream=None):
    """dst[i] [2N] = cmplx[i] [2N] times the real vector real[i] [N] (arm_cmplx_mult_real_*_batch); dst may be
    cmplx."""
    kind = _mat_kind(cmplx)
    _solve_call(f"arm_cmplx_mult_real_{kind}_batch", _cm_ptr(cmplx), _cm_ptr(real), _cm_ptr(dst),
                cmplx.shape[-1] // 2, cmplx.shape[0], _stream_ptr(stream))


def cmplx_dot_prod_batch(a, b, re, im, stream=None, b_stride=None):
    """re[i], im[i] = sum_k a[i][k] * b_i[k] for a [batch, 2N] (arm_cmplx_dot_prod_*_batch).  b [2N]: one vector for
    every item (bStride 0); b [batch, 2N]: one per item.  re / im [batch]: float32, int64 (q31) or int32 (q15).
    b_stride (complex samples) overrides the distance between the items' b vectors."""
    kind = _mat_kind(a)
    n = a.shape[-1] // 2
    if b_stride is None:
        b_stride = 0 if b.dim() == 1 else b.shape[-1] // 2
    _solve_call(f"arm_cmplx_dot_prod_{kind}_batch", _cm_ptr(a), _cm_ptr(b), int(b_stride), n, _cm_ptr(re), _cm_ptr(im),
                a.shape[0], _stream_ptr(stream))


def _search_batch(op, src, result, index, stream):
    kind = _mat_kind(src)
    _solve_call(f"arm_{op}_{kind}_batch", _cm_ptr(src), src.shape[-1], _cm_ptr(result), _cm_ptr(index), src.shape[0],
                _stream_ptr(stream))


def max_batch(src, result, index, stream=None):
    """result[i], index[i] = the maximum of src[i] [N] and its first index (arm_max_*_batch; float32, int32, int16,
    int8).  index is a 32-bit tensor (the words are uint32)."""
    _search_batch("max", src, result, index, stream)


def min_batch(src, result, index, stream=None):
    """result[i], index[i] = the minimum of src[i] [N] and its first index (arm_min_*_batch)."""
    _search_batch("min", src, result, index, stream)


# ---- statistics: the sums and level measures, the abs / no-index searches, arm_sqrt_q15 -------------------------
_POWER_DT = {"f32": np.float32, "q31": np.int64, "q15": np.int64, "q7": np.int32}


def arm_stat(op, kind, src, src_b=None):
    """The one result word of arm_<op>_<kind> (drop-in, numpy): op is mean, power, rms, var, std, accumulate, mse
    (with src_b) or max_no_idx / min_no_idx / absmax_no_idx / absmin_no_idx.  power returns float32 / int64 / int64
    / int32, everything else the type of src."""
    name = f"arm_{op}_{kind}"
    s = _cm_src(kind, src)
    out = np.zeros(1, dtype=_POWER_DT[kind] if op == "power" else s.dtype)
    if op == "mse":
        b = _cm_src(kind, src_b)
        if b.size != s.size:
            raise ValueError(f"{name}: pSrcB has {b.size} words, pSrcA {s.size}")
        getattr(lib, name)(s.ctypes.data, b.ctypes.data, s.size, out.ctypes.data)
    else:
        getattr(lib, name)(s.ctypes.data, s.size, out.ctypes.data)
    _check_void(name)
    return out[0]


def arm_absmax(kind, src):
    """(value, index) of the maximum of |x| (saturating), the first index on a tie, through arm_absmax_*."""
    return _arm_search("absmax", kind, src)


def arm_absmin(kind, src):
    """(value, index) of the minimum of |x| (saturating), the first index on a tie, through arm_absmin_*."""
    return _arm_search("absmin", kind, src)


def arm_sqrt_q15(x):
    """(status, root) of one q15 word through arm_sqrt_q15: a negative x gives (ARM_MATH_ARGUMENT_ERROR, 0)."""
    out = np.zeros(1, dtype=np.int16)
    st = lib.arm_sqrt_q15(int(x), out.ctypes.data)
    return st, out[0]


def arm_cmplx_mag_fast_q15(src):
    """arm_sqrt_q15((re*re + im*im) >> 17) of every interleaved (re, im) pair through arm_cmplx_mag_fast_q15."""
    s = _cm_src("q15", src)
    n = s.size // 2
    d = np.zeros(n, dtype=np.int16)
    lib.arm_cmplx_mag_fast_q15(s.ctypes.data, d.ctypes.data, n)
    _check_void("arm_cmplx_mag_fast_q15")
    return d


def cmplx_mag_fast_batch(src, dst, stream=None):
    """dst[i] [N] = arm_cmplx_mag_fast_q15 of src[i] [2N] (int16 device tensors); dst must not overlap src."""
    _solve_call("arm_cmplx_mag_fast_q15_batch", _cm_ptr(src), _cm_ptr(dst), src.shape[-1] // 2, src.shape[0],
                _stream_ptr(stream))


def _stat_batch(op, src, result, stream):
    kind = _mat_kind(src)
    _solve_call(f"arm_{op}_{kind}_batch", _cm_ptr(src), src.shape[-1], _cm_ptr(result), src.shape[0],
                _stream_ptr(stream))


def mean_batch(src, result, stream=None):
    """result[i] = arm_mean_* of src[i] [N] for contiguous device tensors src [batch, N] (float32, int32, int16,
    int8) and result [batch] of the same type."""
    _stat_batch("mean", src, result, stream)


def power_batch(src, result, stream=None):
    """result[i] = arm_power_* of src[i] [N]; result is float32, int64 (q31, q15) or int32 (q7)."""
    _stat_batch("power", src, result, stream)


def rms_batch(src, result, stream=None):
    """result[i] = arm_rms_* of src[i] [N] (float32, int32, int16)."""
    _stat_batch("rms", src, result, stream)


def var_batch(src, result, stream=None):
    """result[i] = arm_var_* of src[i] [N] (float32, int32, int16): the unbiased variance."""
    _stat_batch("var", src, result, stream)


def std_batch(src, result, stream=None):
    """result[i] = arm_std_* of src[i] [N] (float32, int32, int16)."""
    _stat_batch("std", src, result, stream)


def accumulate_batch(src, result, stream=None):
    """result[i] = arm_accumulate_f32 of src[i] [N]: the ordered float32 sum."""
    _stat_batch("accumulate", src, result, stream)


def mse_batch(a, b, result, stream=None):
    """result[i] = arm_mse_* of a[i] and b[i] [N] (float32, int32, int16, int8)."""
    kind = _mat_kind(a)
    _solve_call(f"arm_mse_{kind}_batch", _cm_ptr(a), _cm_ptr(b), a.shape[-1], _cm_ptr(result), a.shape[0],
                _stream_ptr(stream))


def absmax_batch(src, result, index, stream=None):
    """result[i], index[i] = the maximum of |src[i]| and its first index (arm_absmax_*_batch)."""
    _search_batch("absmax", src, result, index, stream)


def absmin_batch(src, result, index, stream=None):
    """result[i], index[i] = the minimum of |src[i]| and its first index (arm_absmin_*_batch)."""
    _search_batch("absmin", src, result, index, stream)


def max_no_idx_batch(src, result, stream=None):
    """result[i] = arm_max_no_idx_* of src[i] [N]."""
    _stat_batch("max_no_idx", src, result, stream)


def min_no_idx_batch(src, result, stream=None):
    """result[i] = arm_min_no_idx_* of src[i] [N]."""
    _stat_batch("min_no_idx", src, result, stream)


def absmax_no_idx_batch(src, result, stream=None):
    """result[i] = arm_absmax_no_idx_* of src[i] [N]."""
    _stat_batch("absmax_no_idx", src, result, stream)


def absmin_no_idx_batch(src, result, stream=None):
    """result[i] = arm_absmin_no_idx_* of src[i] [N]."""
    _stat_batch("absmin_no_idx", src, result, stream)


# ---- basic math: add .. clip, the bitwise functions, dot_prod ---------------------------------------------------
_BASIC_DT = dict(_MAT_DT, u32=np.uint32, u16=np.uint16, u8=np.uint8)
_BASIC_TWO = ("add", "sub", "mult", "and", "or", "xor")
_DOT_PROD_DT = {"f32": np.float32, "q31": np.int64, "q15": np.int64, "q7": np.int32}


def _basic_scalars(op, kind, scalars):
    """The scalar arguments of arm_<op>_<kind> in the reference's order, as Python numbers."""
    want = {"offset": 1, "scale": 1 if kind == "f32" else 2, "shift": 1, "clip": 2}.get(op, 0)
    if len(scalars) != want:
        raise TypeError(f"arm_{op}_{kind} takes {want} scalar argument(s), got {len(scalars)}")
    num = float if kind == "f32" else int
    if op == "shift":
        return [int(scalars[0])]
    if op == "scale" and kind != "f32":
        return [int(scalars[0]), int(scalars[1])]
    return [num(v) for v in scalars]


def _basic_args(op, srcs, dst, scalars, n):
    """The C argument list: arm_clip_* has the scalars after pDst, the others after pSrc."""
    if op == "clip":
        return [*srcs, dst, *scalars, n]
    return [*srcs, *scalars, dst, n]


def arm_basic2(op, kind, a, b):
    """a op b, element by element, through arm_<op>_<kind> (drop-in, numpy): op add, sub, mult with kind f32, q31,
    q15, q7 (saturating in fixed point), or and, or, xor with kind u32, u16, u8."""
    dt = _BASIC_DT[kind]
    a, b = np.ascontiguousarray(a, dtype=dt).reshape(-1), np.ascontiguousarray(b, dtype=dt).reshape(-1)
    if b.size != a.size:
        raise ValueError(f"arm_{op}_{kind}: pSrcB has {b.size} words, pSrcA {a.size}")
    if op not in _BASIC_TWO:
        raise ValueError(f"arm_{op}_{kind} does not take two sources")
    d = np.zeros(a.size, dtype=dt)
    getattr(lib, f"arm_{op}_{kind}")(a.ctypes.data, b.ctypes.data, d.ctypes.data, a.size)
    _check_void(f"arm_{op}_{kind}")
    return d


def arm_basic1(op, kind, src, *scalars):
    """op(src) through arm_<op>_<kind> (drop-in, numpy) with the reference's scalar arguments: offset (offset),
    scale (scale; fixed point: scaleFract, shift), shift (shiftBits), clip (low, high), abs, negate, not."""
    dt = _BASIC_DT[kind]
    s = np.ascontiguousarray(src, dtype=dt).reshape(-1)
    d = np.zeros(s.size, dtype=dt)
    getattr(lib, f"arm_{op}_{kind}")(*_basic_args(op, [s.ctypes.data], d.ctypes.data,
                                                  _basic_scalars(op, kind, scalars), s.size))
    _check_void(f"arm_{op}_{kind}")
    return d


def arm_dot_prod(kind, a, b):
    """sum a[k] * b[k] through arm_dot_prod_f32 (float32, one ordered chain) / _q31 (int64, products >> 14) / _q15
    (int64) / _q7 (int32)."""
    a, b = _cm_src(kind, a), _cm_src(kind, b)
    if b.size != a.size:
        raise ValueError(f"arm_dot_prod_{kind}: pSrcB has {b.size} words, pSrcA {a.size}")
    out = np.zeros(1, dtype=_DOT_PROD_DT[kind])
    getattr(lib, f"arm_dot_prod_{kind}")(a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data)
    _check_void(f"arm_dot_prod_{kind}")
    return out[0]


def _basic_kind(op, t):
    if op in ("and", "or", "xor", "not"):
        return {4: "u32", 2: "u16", 1: "u8"}[t.element_size()]
    return _mat_kind(t)


def _basic_batch(op, srcs, dst, scalars, stream):
    kind = _basic_kind(op, srcs[0])
    n = srcs[0].shape[-1]
    batch = srcs[0].numel() // n if n else 0
    _solve_call(f"arm_{op}_{kind}_batch", *_basic_args(op, [_cm_ptr(x) for x in srcs], _cm_ptr(dst),
                                                       _basic_scalars(op, kind, scalars), n), batch,
                _stream_ptr(stream))


def add_batch(a, b, dst, stream=None):
    """dst = a + b for contiguous device tensors [batch, N] of float32 / int32 (q31) / int16 (q15) / int8 (q7)
    (arm_add_*_batch; saturating in fixed point).  dst may be a or b."""
    _basic_batch("add", [a, b], dst, (), stream)


def sub_batch(a, b, dst, stream=None):
    """dst = a - b (arm_sub_*_batch); dst may be a or b."""
    _basic_batch("sub", [a, b], dst, (), stream)


def mult_batch(a, b, dst, stream=None):
    """dst = a * b, element by element (arm_mult_*_batch: a window on a batch of frames); dst may be a or b."""
    _basic_batch("mult", [a, b], dst, (), stream)


def offset_batch(src, offset, dst, stream=None):
    """dst = src + offset (arm_offset_*_batch); dst may be src."""
    _basic_batch("offset", [src], dst, (offset,), stream)


def scale_batch(src, scale, dst, shift=0, stream=None):
    """dst = src * scale (arm_scale_*_batch); fixed point: (src * scale) << shift in the reference's formats."""
    _basic_batch("scale", [src], dst, (scale,) if _mat_kind(src) == "f32" else (scale, shift), stream)


def shift_batch(src, shift_bits, dst, stream=None):
    """dst = src << shift_bits, saturating (negative: an arithmetic right shift) (arm_shift_*_batch)."""
    _basic_batch("shift", [src], dst, (shift_bits,), stream)


def clip_batch(src, low, high, dst, stream=None):
    """dst = src clipped to [low, high] (arm_clip_*_batch)."""
    _basic_batch("clip", [src], dst, (low, high), stream)


def abs_batch(src, dst, stream=None):
    """dst = |src|, saturating in fixed point (arm_abs_*_batch)."""
    _basic_batch("abs", [src], dst, (), stream)


def negate_batch(src, dst, stream=None):
    """dst = -src, saturating in fixed point (arm_negate_*_batch)."""
    _basic_batch("negate", [src], dst, (), stream)


def and_batch(a, b, dst, stream=None):
    """dst = a & b for integer device tensors of 4-, 2- or 1-byte words (arm_and_u32 / _u16 / _u8_batch)."""
    _basic_batch("and", [a, b], dst, (), stream)


def or_batch(a, b, dst, stream=None):
    """dst = a | b (arm_or_*_batch)."""
    _basic_batch("or", [a, b], dst, (), stream)


def xor_batch(a, b, dst, stream=None):
    """dst = a ^ b (arm_xor_*_batch)."""
    _basic_batch("xor", [a, b], dst, (), stream)


def not_batch(src, dst, stream=None):
    """dst = ~src (arm_not_*_batch)."""
    _basic_batch("not", [src], dst, (), stream)


def dot_prod_batch(a, b, result, stream=None, b_stride=None):
    """result[i] = sum_k a[i][k] * b_i[k] for a [batch, N] (arm_dot_prod_*_batch).  b [N]: one vector for every item
    (bStride 0: a bank of signals against one template); b [batch, N]: one per item.  result [batch]: float32, int64
    (q31, q15) or int32 (q7).  b_stride (words) overrides the distance between the items' b vectors."""
    kind = _mat_kind(a)
    if b_stride is None:
        b_stride = 0 if b.dim() == 1 else b.shape[-1]
    _solve_call(f"arm_dot_prod_{kind}_batch", _cm_ptr(a), _cm_ptr(b), int(b_stride), a.shape[-1], _cm_ptr(result),
                a.shape[0], _stream_ptr(stream))


# ---- support functions: conversions, copy, fill, sort, weighted average, barycenter -----------------------------
ARM_SORT_BITONIC, ARM_SORT_BUBBLE, ARM_SORT_HEAP, ARM_SORT_INSERTION, ARM_SORT_QUICK, ARM_SORT_SELECTION = range(6)
ARM_SORT_DESCENDING, ARM_SORT_ASCENDING = 0, 1


def _support_name(src_kind, dst_kind):
    if src_kind == dst_kind:
        return f"arm_copy_{src_kind}"
    return f"arm_{_abi.SUPPORT_NAMES[src_kind]}_to_{_abi.SUPPORT_NAMES[dst_kind]}"


def arm_convert(src_kind, dst_kind, src):
    """arm_<src>_to_<dst> (kinds f32, q31, q15, q7; equal kinds: arm_copy_<kind>) of a numpy vector (drop-in)."""
    name = _support_name(src_kind, dst_kind)
    s = _cm_src(src_kind, src)
    d = np.zeros(s.size, dtype=_MAT_DT[dst_kind])
    getattr(lib, name)(s.ctypes.data, d.ctypes.data, s.size)
    _check_void(name)
    return d


def arm_fill(kind, value, block_size):
    """arm_fill_<kind>: block_size words of value (drop-in, numpy)."""
    d = np.zeros(int(block_size), dtype=_MAT_DT[kind])
    getattr(lib, f"arm_fill_{kind}")((float if kind == "f32" else int)(value), d.ctypes.data, d.size)
    _check_void(f"arm_fill_{kind}")
    return d


def arm_sort_init_f32(S, alg, dir):
    lib.arm_sort_init_f32(C.byref(S), int(alg), int(dir))


def arm_merge_sort_init_f32(S, dir, buffer=None):
    """buffer: a float32 numpy array the caller keeps alive, or None; the sort neither reads nor writes it."""
    lib.arm_merge_sort_init_f32(C.byref(S), int(dir), None if buffer is None else buffer.ctypes.data)


def _arm_sort(name, S, src):
    s = _cm_src("f32", src)
    d = np.zeros(s.size, dtype=np.float32)
    getattr(lib, name)(C.byref(S), s.ctypes.data, d.ctypes.data, s.size)
    _check_void(name)
    return d


def arm_sort_f32(S, src):
    """The float32 vector sorted in S.dir by the IEEE total order (arm_sort_f32; S.alg only selects among equal
    results)."""
    return _arm_sort("arm_sort_f32", S, src)


def arm_merge_sort_f32(S, src):
    """As arm_sort_f32 through arm_merge_sort_f32; S.buffer is not used."""
    return _arm_sort("arm_merge_sort_f32", S, src)


def arm_weighted_average_f32(src, weights):
    """sum(src * weights) / sum(weights) in float32, two ordered chains (arm_weighted_average_f32)."""
    a, w = _cm_src("f32", src), _cm_src("f32", weights)
    if w.size != a.size:
        raise ValueError(f"arm_weighted_average_f32: weights has {w.size} words, in {a.size}")
    r = lib.arm_weighted_average_f32(a.ctypes.data, w.ctypes.data, a.size)
    _check_void("arm_weighted_average_f32")
    return np.float32(r)


def arm_barycenter_f32(src, weights, nb_vectors, vec_dim):
    """The barycenter [vec_dim] of nb_vectors vectors (rows of src) under weights (arm_barycenter_f32)."""
    a, w = _cm_src("f32", src), _cm_src("f32", weights)
    if a.size != nb_vectors * vec_dim or w.size != nb_vectors:
        raise ValueError("arm_barycenter_f32: in holds nbVectors * vecDim words and weights nbVectors")
    d = np.zeros(vec_dim, dtype=np.float32)
    lib.arm_barycenter_f32(a.ctypes.data, w.ctypes.data, d.ctypes.data, nb_vectors, vec_dim)
    _check_void("arm_barycenter_f32")
    return d


def convert_batch(src, dst, stream=None):
    """dst = src converted between float32 / int32 (q31) / int16 (q15) / int8 (q7) for contiguous device tensors
    [batch, N] (arm_<a>_to_<b>_batch; equal types: arm_copy_*_batch).  dst may be src where the widths are equal."""
    n = src.shape[-1]
    _solve_call(_support_name(_mat_kind(src), _mat_kind(dst)) + "_batch", _cm_ptr(src), _cm_ptr(dst), n,
                src.numel() // n if n else 0, _stream_ptr(stream))


def copy_batch(src, dst, stream=None):
    """dst = src (arm_copy_*_batch)."""
    if src.dtype != dst.dtype:
        raise TypeError("copy_batch: src and dst differ in type")
    convert_batch(src, dst, stream)


def fill_batch(value, dst, stream=None):
    """Every word of dst [batch, N] = value (arm_fill_*_batch)."""
    kind = _mat_kind(dst)
    n = dst.shape[-1]
    _solve_call(f"arm_fill_{kind}_batch", (float if kind == "f32" else int)(value), _cm_ptr(dst), n,
                dst.numel() // n if n else 0, _stream_ptr(stream))


def sort_batch(src, dst, dir=ARM_SORT_ASCENDING, stream=None, merge=False):
    """dst[i] = src[i] sorted in dir by the IEEE total order, for contiguous float32 device tensors [batch, N]
    (arm_sort_f32_batch; merge=True: arm_merge_sort_f32_batch, the same kernels).  dst may be src."""
    n = src.shape[-1]
    _solve_call("arm_merge_sort_f32_batch" if merge else "arm_sort_f32_batch", _cm_ptr(src), _cm_ptr(dst), n,
                int(dir), src.numel() // n if n else 0, _stream_ptr(stream))


def weighted_average_batch(src, weights, result, stream=None, w_stride=None):
    """result[i] = arm_weighted_average_f32 of src[i] [N] under weights [N] (one for every item) or [batch, N].
    w_stride (words) overrides the distance between the items' weight vectors."""
    if w_stride is None:
        w_stride = 0 if weights.dim() == 1 else weights.shape[-1]
    _solve_call("arm_weighted_average_f32_batch", _cm_ptr(src), _cm_ptr(weights), int(w_stride), src.shape[-1],
                _cm_ptr(result), src.shape[0], _stream_ptr(stream))


def barycenter_batch(src, weights, out, stream=None, w_stride=None):
    """out[i] [vecDim] = the barycenter of src[i] [nbVectors, vecDim] under weights [nbVectors] (one for every item)
    or [batch, nbVectors] (arm_barycenter_f32_batch)."""
    if w_stride is None:
        w_stride = 0 if weights.dim() == 1 else weights.shape[-1]
    _solve_call("arm_barycenter_f32_batch", _cm_ptr(src), _cm_ptr(weights), int(w_stride), _cm_ptr(out),
                src.shape[1], src.shape[2], src.shape[0], _stream_ptr(stream))


# ---- distance functions: f32, boolean, dynamic time warping ------------------------------------------------------
ARM_DTW_SAKOE_CHIBA_WINDOW, ARM_DTW_SLANTED_BAND_WINDOW = 1, 3
DISTANCE_F32 = _abi.DISTANCE_F32
DISTANCE_BOOL = _abi.DISTANCE_BOOL


def arm_distance_f32(name, a, b):
    """arm_<name>_distance_f32 of two float32 vectors (drop-in, numpy; name in DISTANCE_F32).  correlation works on
    copies; arm_correlation_distance_f32 below returns the shifted vectors as well."""
    fn = f"arm_{name}_distance_f32"
    x, y = np.array(a, dtype=np.float32).reshape(-1), np.array(b, dtype=np.float32).reshape(-1)
    if x.size != y.size:
        raise ValueError(f"{fn}: {x.size} and {y.size} words")
    r = getattr(lib, fn)(x.ctypes.data, y.ctypes.data, x.size)
    _check_void(fn)
    return np.float32(r)


def arm_correlation_distance_f32(a, b):
    """(distance, a - mean(a), b - mean(b)): the reference overwrites its operands with the shifted words."""
    x, y = np.array(a, dtype=np.float32).reshape(-1), np.array(b, dtype=np.float32).reshape(-1)
    if x.size != y.size:
        raise ValueError(f"arm_correlation_distance_f32: {x.size} and {y.size} words")
    r = lib.arm_correlation_distance_f32(x.ctypes.data, y.ctypes.data, x.size)
    _check_void("arm_correlation_distance_f32")
    return np.float32(r), x, y


def arm_boolean_distance(name, a, b, number_of_bools):
    """arm_<name>_distance of two vectors of packed uint32 words (drop-in, numpy; name in DISTANCE_BOOL); of a last,
    partial word the top number_of_bools % 32 bits count."""
    fn = f"arm_{name}_distance"
    x, y = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1), np.ascontiguousarray(b, dtype=np.uint32).reshape(-1)
    words = (int(number_of_bools) + 31) // 32
    if x.size < words or y.size < words:
        raise ValueError(f"{fn}: {number_of_bools} booleans need {words} words")
    r = getattr(lib, fn)(x.ctypes.data, y.ctypes.data, int(number_of_bools))
    _check_void(fn)
    return np.float32(r)


def arm_dtw_init_window_q7(window_type, window_size, rows, cols):
    """(status, window [rows, cols] int8) through arm_dtw_init_window_q7."""
    w = np.zeros((rows, cols), dtype=np.int8)
    st = lib.arm_dtw_init_window_q7(int(window_type), int(window_size), C.byref(_mat("q7", w)))
    _check_void("arm_dtw_init_window_q7")
    return st, w


def arm_dtw_distance_f32(distance, window=None):
    """(status, distance value, dtw cost matrix) through arm_dtw_distance_f32; window: int8 [rows, cols] or None.
    The value is NaN where the status is ARM_MATH_ARGUMENT_ERROR (no path inside the window)."""
    d = np.ascontiguousarray(distance, dtype=np.float32)
    cost = np.zeros_like(d)
    value = np.full(1, np.nan, dtype=np.float32)
    w = None if window is None else np.ascontiguousarray(window, dtype=np.int8)
    st = lib.arm_dtw_distance_f32(C.byref(_matf(d)), None if w is None else C.byref(_mat("q7", w)),
                                  C.byref(_matf(cost)), value.ctypes.data)
    _check_void("arm_dtw_distance_f32")
    return st, value[0], cost


def arm_dtw_path_f32(dtw):
    """The warping path [length, 2] int16 of (query, template) index pairs through arm_dtw_path_f32."""
    c = np.ascontiguousarray(dtw, dtype=np.float32)
    path = np.zeros(2 * (c.shape[0] + c.shape[1]), dtype=np.int16)
    length = np.zeros(1, dtype=np.uint32)
    lib.arm_dtw_path_f32(C.byref(_matf(c)), path.ctypes.data, length.ctypes.data)
    _check_void("arm_dtw_path_f32")
    return path[:2 * int(length[0])].reshape(-1, 2)


def distance_batch(name, a, b, result, stream=None, b_stride=None):
    """result[i] = arm_<name>_distance_f32 of a[i] and b_i for float32 device tensors a [batch, N], b [N] (one vector
    for every item: one query against many stored vectors) or [batch, N], result [batch].  b_stride (words) overrides
    the distance between the items' b vectors.  The sources are only read."""
    if b_stride is None:
        b_stride = 0 if b.dim() == 1 else b.shape[-1]
    _solve_call(f"arm_{name}_distance_f32_batch", _cm_ptr(a), _cm_ptr(b), int(b_stride), a.shape[-1], _cm_ptr(result),
                a.shape[0], _stream_ptr(stream))


def boolean_distance_batch(name, a, b, number_of_bools, result, stream=None, b_stride=None):
    """result[i] = arm_<name>_distance of the number_of_bools booleans packed in a[i] and b_i: int32 device tensors a
    [batch, ceil(number_of_bools / 32)], b the same or one row for every item; result float32 [batch]."""
    if b_stride is None:
        b_stride = 0 if b.dim() == 1 else b.shape[-1]
    _solve_call(f"arm_{name}_distance_batch", _cm_ptr(a), _cm_ptr(b), int(b_stride), int(number_of_bools),
                _cm_ptr(result), a.shape[0], _stream_ptr(stream))


def dtw_init_window_batch(window_type, window_size, window, stream=None):
    """Fills every item of the int8 device tensor window [batch, rows, cols] (arm_dtw_init_window_q7_batch)."""
    _solve_call("arm_dtw_init_window_q7_batch", int(window_type), int(window_size), _cm_ptr(window), window.shape[-2],
                window.shape[-1], window.numel() // max(1, window.shape[-2] * window.shape[-1]), _stream_ptr(stream))


def dtw_distance_batch(distance, window, dtw, result, status=None, stream=None, w_stride=None):
    """dtw[i], result[i] = the cost matrix and the DTW distance of distance[i] for float32 device tensors [batch, rows,
    cols] (arm_dtw_distance_f32_batch); window: None, int8 [rows, cols] (one for every item) or [batch, rows, cols].
    Returns the per-item int32 status tensor as mat_inverse_batch does; result[i] is written where it is 0."""
    status, ps = _solve_status(distance, status)
    if w_stride is None:
        w_stride = 0 if window is None or window.dim() == 2 else window.shape[-2] * window.shape[-1]
    _solve_call("arm_dtw_distance_f32_batch", _cm_ptr(distance), C.c_void_p(None if window is None else window.data_ptr()),
                int(w_stride), _cm_ptr(dtw), distance.shape[-2], distance.shape[-1], _cm_ptr(result), ps,
                distance.shape[0], _stream_ptr(stream))
    return None if status is False else status


def dtw_path_batch(dtw, path, path_length, stream=None):
    """path[i] (int16 [batch, rows + cols, 2]) and path_length[i] (int32 [batch]) = the warping path of the cost
    matrix dtw[i] (arm_dtw_path_f32_batch); a length of 0 marks a matrix without a path."""
    _solve_call("arm_dtw_path_f32_batch", _cm_ptr(dtw), dtw.shape[-2], dtw.shape[-1], _cm_ptr(path),
                _cm_ptr(path_length), dtw.shape[0], _stream_ptr(stream))


# ---- vexp / vlog, log-domain statistics, SVM, naive Bayes -----------------------------------------------------------
arm_svm_linear_instance_f32 = _abi.arm_svm_linear_instance_f32
arm_svm_polynomial_instance_f32 = _abi.arm_svm_polynomial_instance_f32
arm_svm_rbf_instance_f32 = _abi.arm_svm_rbf_instance_f32
arm_gaussian_naive_bayes_instance_f32 = _abi.arm_gaussian_naive_bayes_instance_f32
SVM_KINDS = tuple(_abi.SVM_KINDS)
LOGDOM_FUNCS = ("entropy", "kullback_leibler", "logsumexp", "logsumexp_dot_prod")


def arm_fast_math_f32(name, src):
    """arm_vexp_f32 / arm_vlog_f32 (name "vexp" / "vlog") of a float32 vector (drop-in, numpy) -> a new array."""
    x = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    out = np.zeros_like(x)
    getattr(lib, f"arm_{name}_f32")(x.ctypes.data, out.ctypes.data, x.size)
    _check_void(f"arm_{name}_f32")
    return out


def arm_logdom_f32(name, a, b=None):
    """arm_<name>_f32 (name in LOGDOM_FUNCS; drop-in, numpy) -> np.float32.  b: the second vector of kullback_leibler
    and logsumexp_dot_prod, whose scratch buffer is allocated here."""
    fn = f"arm_{name}_f32"
    x = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if name in ("entropy", "logsumexp"):
        r = getattr(lib, fn)(x.ctypes.data, x.size)
    else:
        y = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if x.size != y.size:
            raise ValueError(f"{fn}: {x.size} and {y.size} words")
        if name == "kullback_leibler":
            r = lib.arm_kullback_leibler_f32(x.ctypes.data, y.ctypes.data, x.size)
        else:
            tmp = np.zeros(max(1, x.size), dtype=np.float32)
            r = lib.arm_logsumexp_dot_prod_f32(x.ctypes.data, y.ctypes.data, x.size, tmp.ctypes.data)
    _check_void(fn)
    return np.float32(r)


def svm_instance(kind, intercept, dual, vectors, classes, degree=0, coef0=0.0, gamma=0.0):
    """(instance, keep): an arm_svm_<kind>_instance_f32 filled by arm_svm_<kind>_init_f32 over dual [nSV], vectors
    [nSV, dim] and classes [2]: float32 / int32 numpy arrays (a drop-in model) or device tensors (a model for
    svm_predict_batch).  keep holds the arrays the instance points into."""
    inst, _ = _abi.SVM_KINDS[kind]
    S = inst()
    if hasattr(dual, "data_ptr"):
        keep = [dual.contiguous(), vectors.contiguous(), classes.contiguous()]
        ptrs = [k.data_ptr() for k in keep]
    else:
        keep = [np.ascontiguousarray(dual, dtype=np.float32), np.ascontiguousarray(vectors, dtype=np.float32),
                np.ascontiguousarray(classes, dtype=np.int32)]
        ptrs = [k.ctypes.data for k in keep]
    nsv = int(keep[0].shape[0])
    dim = int(keep[1].shape[-1]) if len(keep[1].shape) > 1 else 0
    extra = {"linear": [], "polynomial": [int(degree), float(coef0), float(gamma)], "rbf": [float(gamma)]}[kind]
    getattr(lib, f"arm_svm_{kind}_init_f32")(C.byref(S), nsv, dim, float(intercept), *ptrs, *extra)   # fills S only
    return S, keep


def arm_svm_predict_f32(kind, S, x):
    """arm_svm_<kind>_predict_f32 of one float32 vector against a host model (drop-in, numpy) -> the class (int)."""
    v = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if v.size != S.vectorDimension:
        raise ValueError(f"arm_svm_{kind}_predict_f32: {v.size} words for dimension {S.vectorDimension}")
    out = np.zeros(1, dtype=np.int32)
    getattr(lib, f"arm_svm_{kind}_predict_f32")(C.byref(S), v.ctypes.data, out.ctypes.data)
    _check_void(f"arm_svm_{kind}_predict_f32")
    return int(out[0])


def bayes_instance(theta, sigma, priors, epsilon):
    """(instance, keep): an arm_gaussian_naive_bayes_instance_f32 over theta, sigma [classes, dim] and priors
    [classes]: float32 numpy arrays or device tensors."""
    S = arm_gaussian_naive_bayes_instance_f32()
    if hasattr(theta, "data_ptr"):
        keep = [theta.contiguous(), sigma.contiguous(), priors.contiguous()]
        ptrs = [k.data_ptr() for k in keep]
    else:
        keep = [np.ascontiguousarray(a, dtype=np.float32) for a in (theta, sigma, priors)]
        ptrs = [k.ctypes.data for k in keep]
    S.numberOfClasses = int(keep[2].shape[0])
    S.vectorDimension = int(keep[0].shape[-1]) if len(keep[0].shape) > 1 else 0
    S.theta, S.sigma, S.classPriors = ptrs
    S.epsilon = float(epsilon)
    return S, keep


def arm_gaussian_naive_bayes_predict_f32(S, x):
    """(the classes' words [numberOfClasses], the class index) through arm_gaussian_naive_bayes_predict_f32."""
    v = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if v.size != S.vectorDimension:
        raise ValueError(f"arm_gaussian_naive_bayes_predict_f32: {v.size} words for dimension {S.vectorDimension}")
    prob = np.zeros(S.numberOfClasses, dtype=np.float32)
    idx = lib.arm_gaussian_naive_bayes_predict_f32(C.byref(S), v.ctypes.data, prob.ctypes.data, None)
    _check_void("arm_gaussian_naive_bayes_predict_f32")
    return prob, int(idx)


def fast_math_batch(name, src, dst, stream=None):
    """dst = expf(src) (name "vexp") or logf(src) ("vlog") for contiguous float32 device tensors of one shape
    (arm_vexp_f32_batch / arm_vlog_f32_batch).  dst may be src."""
    n = src.shape[-1] if src.dim() else 1
    _solve_call(f"arm_{name}_f32_batch", _cm_ptr(src), _cm_ptr(dst), n, src.numel() // n if n else 0,
                _stream_ptr(stream))


def logdom_batch(name, a, b, result, stream=None, b_stride=None):
    """result[i] = arm_<name>_f32 (name in LOGDOM_FUNCS) of a[i] (and b_i) for float32 device tensors a [batch, N],
    result [batch]; b: None for entropy and logsumexp, otherwise [N] (one vector for every item) or [batch, N].
    b_stride (words) overrides the distance between the items' b vectors."""
    if name in ("entropy", "logsumexp"):
        _solve_call(f"arm_{name}_f32_batch", _cm_ptr(a), a.shape[-1], _cm_ptr(result), a.shape[0], _stream_ptr(stream))
        return
    if b_stride is None:
        b_stride = 0 if b.dim() == 1 else b.shape[-1]
    _solve_call(f"arm_{name}_f32_batch", _cm_ptr(a), _cm_ptr(b), int(b_stride), a.shape[-1], _cm_ptr(result),
                a.shape[0], _stream_ptr(stream))


def svm_predict_batch(kind, S, x, result, decision=None, stream=None):
    """result[i] (int32 [items]) = the class of x[i] (float32 [items, dim]) under the device model S (svm_instance over
    device tensors); decision (float32 [items] or None) receives the sums the classes were taken from
    (arm_svm_<kind>_predict_f32_batch)."""
    _solve_call(f"arm_svm_{kind}_predict_f32_batch", C.byref(S), _cm_ptr(x), _cm_ptr(result),
                C.c_void_p(None if decision is None else decision.data_ptr()), x.shape[0], _stream_ptr(stream))


def bayes_predict_batch(S, x, probabilities, classes, stream=None):
    """probabilities[i] (float32 [items, numberOfClasses]) and classes[i] (int32 [items]) of x[i] (float32 [items,
    dim]) under the device model S (arm_gaussian_naive_bayes_predict_f32_batch)."""
    _solve_call("arm_gaussian_naive_bayes_predict_f32_batch", C.byref(S), _cm_ptr(x), _cm_ptr(probabilities),
                _cm_ptr(classes), x.shape[0], _stream_ptr(stream))


# ---- interpolation --------------------------------------------------------------------------------------------------
arm_linear_interp_instance_f32 = _abi.arm_linear_interp_instance_f32
arm_bilinear_interp_instance = _abi.arm_bilinear_interp_instance
arm_spline_instance_f32 = _abi.arm_spline_instance_f32
INTERP_KINDS = ("f32", "q31", "q15", "q7")
_INTERP_NP = {"f32": np.float32, "q31": np.int32, "q15": np.int16, "q7": np.int8}


def _table(t, kind):
    """(pointer, keep) of a table: a device tensor as it is, anything else as a contiguous numpy array."""
    if hasattr(t, "data_ptr"):
        return t.data_ptr(), t
    a = np.ascontiguousarray(t, dtype=_INTERP_NP[kind])
    return a.ctypes.data, a


def linear_interp_instance(x1, x_spacing, table):
    """(instance, keep): an arm_linear_interp_instance_f32 over a float32 table: a numpy array (the scalar drop-in) or a
    device tensor (linear_interp_batch)."""
    ptr, keep = _table(table, "f32")
    return arm_linear_interp_instance_f32(int(np.prod(keep.shape)), float(x1), float(x_spacing), ptr), keep


def bilinear_interp_instance(kind, table):
    """(instance, keep): an arm_bilinear_interp_instance_<kind> over a [numRows, numCols] table: a numpy array (the
    scalar drop-in) or a device tensor (bilinear_interp_batch)."""
    ptr, keep = _table(table, kind)
    return arm_bilinear_interp_instance(int(keep.shape[0]), int(keep.shape[1]), ptr), keep


def arm_linear_interp(kind, table_or_instance, x):
    """arm_linear_interp_<kind> of one sample (computed on the host): an instance for f32, a numpy table otherwise."""
    if kind == "f32":
        r = lib.arm_linear_interp_f32(C.byref(table_or_instance), float(x))
    else:
        t = np.ascontiguousarray(table_or_instance, dtype=_INTERP_NP[kind])
        r = getattr(lib, f"arm_linear_interp_{kind}")(t.ctypes.data, int(x), t.size)
    _check_void(f"arm_linear_interp_{kind}")
    return r


def arm_bilinear_interp(kind, S, X, Y):
    """arm_bilinear_interp_<kind> of one point (computed on the host)."""
    r = getattr(lib, f"arm_bilinear_interp_{kind}")(C.byref(S), *((float(X), float(Y)) if kind == "f32" else (int(X), int(Y))))
    _check_void(f"arm_bilinear_interp_{kind}")
    return r


def arm_spline_f32(spline_type, x, y, xq):
    """arm_spline_init_f32 and arm_spline_f32 on float32 numpy arrays (drop-ins) -> (the values at xq, coeffs
    [3 (n - 1)], tempBuffer [2 n - 1])."""
    x, y, xq = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (x, y, xq))
    n = x.size
    coeffs, temp = np.zeros(max(1, 3 * (n - 1)), np.float32), np.zeros(max(1, 2 * n - 1), np.float32)
    S = arm_spline_instance_f32()
    lib.arm_spline_init_f32(C.byref(S), int(spline_type), x.ctypes.data, y.ctypes.data, n, coeffs.ctypes.data,
                            temp.ctypes.data)
    _check_void("arm_spline_init_f32")
    out = np.zeros(xq.size, np.float32)
    lib.arm_spline_f32(C.byref(S), xq.ctypes.data, out.ctypes.data, xq.size)
    _check_void("arm_spline_f32")
    return out, coeffs[:3 * (n - 1)], temp[:2 * n - 1]


def linear_interp_batch(kind, table_or_instance, x, y, stream=None):
    """y[i] = arm_linear_interp_<kind>(x[i]) for device tensors x (float32, or int32 in 12.20) and y of one shape; an
    instance over a device table for f32, a device table otherwise (arm_linear_interp_<kind>_batch)."""
    if kind == "f32":
        _solve_call("arm_linear_interp_f32_batch", C.byref(table_or_instance), _cm_ptr(x), _cm_ptr(y), x.numel(),
                    _stream_ptr(stream))
    else:
        _solve_call(f"arm_linear_interp_{kind}_batch", _cm_ptr(table_or_instance), table_or_instance.numel(),
                    _cm_ptr(x), _cm_ptr(y), x.numel(), _stream_ptr(stream))


def bilinear_interp_batch(kind, S, X, Y, out, stream=None):
    """out[i] = arm_bilinear_interp_<kind>(S, X[i], Y[i]) for device tensors of one shape; S over a device table
    (arm_bilinear_interp_<kind>_batch)."""
    _solve_call(f"arm_bilinear_interp_{kind}_batch", C.byref(S), _cm_ptr(X), _cm_ptr(Y), _cm_ptr(out), X.numel(),
                _stream_ptr(stream))


def spline_init_batch(spline_type, x, y, coeffs, temp, stream=None):
    """The coefficients of `batch` splines: float32 device tensors x [n] (one knot vector for every item) or
    [batch, n], y [batch, n], coeffs [batch, 3 (n - 1)], temp [batch, 2 n - 1] (arm_spline_init_f32_batch)."""
    n = y.shape[-1]
    _solve_call("arm_spline_init_f32_batch", int(spline_type), _cm_ptr(x), 0 if x.dim() == 1 else x.stride(0),
                _cm_ptr(y), n, _cm_ptr(coeffs), _cm_ptr(temp), y.shape[0], _stream_ptr(stream))


def spline_batch(x, y, coeffs, xq, dst, stream=None):
    """dst[i] = the spline of item i at its queries: x [n] or [batch, n], y [batch, n], coeffs [batch, 3 (n - 1)], xq
    [blockSize] (one query vector for every item) or [batch, blockSize], dst [batch, blockSize]
    (arm_spline_f32_batch)."""
    _solve_call("arm_spline_f32_batch", _cm_ptr(x), 0 if x.dim() == 1 else x.stride(0), _cm_ptr(y), _cm_ptr(coeffs),
                y.shape[-1], _cm_ptr(xq), 0 if xq.dim() == 1 else xq.stride(0), _cm_ptr(dst), dst.shape[-1],
                y.shape[0], _stream_ptr(stream))


# ---- quaternions ----------------------------------------------------------------------------------------------------
QUATERNION_FUNCS = tuple(_abi.QUATERNION_FUNCS)


def arm_quaternion_f32(name, src):
    """arm_<name>_f32 (name in QUATERNION_FUNCS) of a flat float32 array of quaternions (4 words each; rotations of 9
    words for "rotation2quaternion") (drop-in, numpy) -> a new flat array."""
    wa, wd = _abi.QUATERNION_FUNCS[name]
    x = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    n = x.size // wa
    out = np.zeros(n * wd, dtype=np.float32)
    getattr(lib, f"arm_{name}_f32")(x.ctypes.data, out.ctypes.data, n)
    _check_void(f"arm_{name}_f32")
    return out


def arm_quaternion_product_f32(a, b, single=False):
    """arm_quaternion_product_f32 of two flat float32 arrays of quaternions (single=True:
    arm_quaternion_product_single_f32 of two quaternions) (drop-in, numpy) -> a new flat array."""
    x = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    y = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
    n = 1 if single else x.size // 4
    if x.size < 4 * n or y.size < 4 * n:
        raise ValueError(f"arm_quaternion_product_f32: {x.size} and {y.size} words for {n} quaternions")
    out = np.zeros(4 * n, dtype=np.float32)
    if single:
        lib.arm_quaternion_product_single_f32(x.ctypes.data, y.ctypes.data, out.ctypes.data)
    else:
        lib.arm_quaternion_product_f32(x.ctypes.data, y.ctypes.data, out.ctypes.data, n)
    _check_void("arm_quaternion_product_f32")
    return out


def quaternion_batch(name, src, dst, stream=None):
    """dst[i] = arm_<name>_f32 (name in QUATERNION_FUNCS) of src[i] for contiguous float32 device tensors src [n, 4]
    (or [n, 9] rotations) and dst [n], [n, 4] or [n, 9] (arm_<name>_f32_batch)."""
    _solve_call(f"arm_{name}_f32_batch", _cm_ptr(src), _cm_ptr(dst), src.shape[0], _stream_ptr(stream))


def quaternion_product_batch(a, b, dst, stream=None):
    """dst[i] = a[i] * b[i] for contiguous float32 device tensors a, dst [n, 4] and b [n, 4], or b [4]: one quaternion
    for every item (arm_quaternion_product_f32_batch)."""
    _solve_call("arm_quaternion_product_f32_batch", _cm_ptr(a), _cm_ptr(b), 0 if b.dim() == 1 else 4, _cm_ptr(dst),
                a.shape[0], _stream_ptr(stream))


def mat_mult_batch(a, b, c, stream=None, fast=False):
    """c[i] = a[i] @ b[i] for device tensors [batch, M, K] x [batch, K, N] -> [batch, M, N];
    float32 -> arm_mat_mult_f32_batch, int8 -> _q7, int16 -> _q15, int32 -> _q31 (fast=True:
    _fast_q15 / _fast_q31)."""
    import torch
    batch, m, k = a.shape
    n = b.shape[2]
    kind, inst, ptr = {torch.float32: ("f32", arm_matrix_instance_f32, _abi.c_f32p),
                       torch.int16: ("q15", arm_matrix_instance_q15, _abi.c_i16p),
                       torch.int32: ("q31", arm_matrix_instance_q31, _abi.c_i32p),
                       torch.int8: ("q7", arm_matrix_instance_q7, _abi.c_i8p)}[a.dtype]
    A, B, Cm = inst(m, k, C.cast(a.data_ptr(), ptr)), inst(k, n, C.cast(b.data_ptr(), ptr)), \
        inst(m, n, C.cast(c.data_ptr(), ptr))
    fn = getattr(lib, f"arm_mat_mult_{'fast_' if fast and kind != 'f32' else ''}{kind}_batch")
    st = fn(C.byref(A), C.byref(B), C.byref(Cm), batch, _stream_ptr(stream))
    if st != ARM_MATH_SUCCESS:
        raise RuntimeError(f"{fn.__name__} -> {st}: {last_error()[1]}")