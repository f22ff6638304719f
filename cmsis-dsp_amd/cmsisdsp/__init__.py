"""`cmsisdsp`-compatible Python module over the MI355X library.

Same function names, argument order and return conventions as the reference's CPython
extension (PythonWrapper/cmsisdsp_pkg/src/cmsisdsp_transform.c, _filtering.c, _matrix.c,
as exercised by PythonWrapper/examples/testdsp*.py, testrfft_all.py, testmfcc.py) for the
functions this backend provides: numpy (or list) in, a new numpy array out, instances as
opaque objects.  Every call runs on the GPU through libcmsisdsp_mi355x.so (the drop-in C
ABI, host buffers staged through device memory); there is no CPU implementation here.

    import sys; sys.path.insert(0, "cmsis-dsp_amd")
    import cmsisdsp as dsp
    S = dsp.arm_cfft_instance_f32(); dsp.arm_cfft_init_f32(S, 1024)
    y = dsp.arm_cfft_f32(S, x, 0, 1)
"""
import ctypes as _C

import numpy as _np

import cmsisdsp_amd as _amd
from cmsisdsp_amd import _abi
from . import datatype  # noqa: F401

_lib = _amd.lib
_ARCH_DEFAULT = 1                      # ARM_MATH_DEFAULT_TARGET_ARCH = ARM_MATH_SCALAR_ARCH (arm_math_types.h)


def has_neon():
    return False


# ------------------------------------------------------------------ instances
class _Instance:
    _struct = None

    def __init__(self):
        self._s = self._struct()
        self._keep = []

    def __getattr__(self, name):            # accessor methods: inst.fftLen(), inst.numTaps() ...
        s = object.__getattribute__(self, "_s")
        if any(f == name for f, _ in s._fields_):
            return lambda: getattr(s, name)
        raise AttributeError(name)


def _make(name, struct):
    return type(name, (_Instance,), {"_struct": struct})


arm_cfft_instance_f32 = _make("arm_cfft_instance_f32", _abi.arm_cfft_instance_f32)
arm_cfft_instance_q31 = _make("arm_cfft_instance_q31", _abi.arm_cfft_instance_q31)
arm_cfft_instance_q15 = _make("arm_cfft_instance_q15", _abi.arm_cfft_instance_q15)
arm_rfft_fast_instance_f32 = _make("arm_rfft_fast_instance_f32", _abi.arm_rfft_fast_instance_f32)
arm_fir_instance_f32 = _make("arm_fir_instance_f32", _abi.arm_fir_instance_f32)
arm_fir_instance_q31 = _make("arm_fir_instance_q31", _abi.arm_fir_instance_q31)
arm_fir_instance_q15 = _make("arm_fir_instance_q15", _abi.arm_fir_instance_q15)
arm_fir_instance_q7 = _make("arm_fir_instance_q7", _abi.arm_fir_instance_q7)
arm_mfcc_instance_f32 = _make("arm_mfcc_instance_f32", _abi.arm_mfcc_instance_f32)
arm_mfcc_instance_q31 = _make("arm_mfcc_instance_q31", _abi.arm_mfcc_instance_q31)
arm_mfcc_instance_q15 = _make("arm_mfcc_instance_q15", _abi.arm_mfcc_instance_q15)
for _t in ("f32", "q31", "q15"):
    globals()[f"arm_fir_decimate_instance_{_t}"] = _make(f"arm_fir_decimate_instance_{_t}",
                                                         _abi.arm_fir_decimate_instance)
    globals()[f"arm_fir_interpolate_instance_{_t}"] = _make(f"arm_fir_interpolate_instance_{_t}",
                                                            _abi.arm_fir_interpolate_instance)
for _t in ("f32", "q31", "q15"):
    globals()[f"arm_fir_lattice_instance_{_t}"] = _make(f"arm_fir_lattice_instance_{_t}", _abi.arm_fir_lattice_instance)
for _t in {v[0].__name__: v[0] for v in _abi.BIQUAD_FUNCS.values()}.values():
    globals()[_t.__name__] = _make(_t.__name__, _t)
for _t in (v[0] for v in _abi.ADAPTIVE_FUNCS.values()):
    globals()[_t.__name__] = _make(_t.__name__, _t)
for _t in ("f32", "q31", "q15", "q7"):
    globals()[f"arm_fir_sparse_instance_{_t}"] = _make(f"arm_fir_sparse_instance_{_t}", _abi.arm_fir_sparse_instance)
del _t
arm_rfft_instance_q31 = _make("arm_rfft_instance_q31", _abi.arm_rfft_instance_q31)
arm_rfft_instance_q15 = _make("arm_rfft_instance_q15", _abi.arm_rfft_instance_q15)

_DT = {"f32": _np.float32, "q31": _np.int32, "q15": _np.int16, "q7": _np.int8}


def _arr(x, dt):
    return _np.ascontiguousarray(_np.asarray(x).astype(dt, copy=False))


def _check(what):
    code, msg = _amd.last_error()
    if code:
        _lib.arm_mi355x_clear_error()
        raise RuntimeError(f"{what}: device error {code}: {msg}")


# ------------------------------------------------------------------ complex FFT
def _cfft_init(kind):
    def init(inst, fftLen):
        return getattr(_lib, f"arm_cfft_init_{kind}")(_C.byref(inst._s), int(fftLen))
    init.__name__ = f"arm_cfft_init_{kind}"
    return init


def _cfft(kind):
    def run(inst, p1, ifftFlag, bitReverseFlag=1, tmp=None):
        buf = _arr(p1, _DT[kind]).copy()
        getattr(_lib, f"arm_cfft_{kind}")(_C.byref(inst._s), buf.ctypes.data, int(ifftFlag), int(bitReverseFlag))
        _check(f"arm_cfft_{kind}")
        return buf
    run.__name__ = f"arm_cfft_{kind}"
    return run


arm_cfft_init_f32, arm_cfft_init_q31, arm_cfft_init_q15 = (_cfft_init(k) for k in ("f32", "q31", "q15"))
arm_cfft_f32, arm_cfft_q31, arm_cfft_q15 = (_cfft(k) for k in ("f32", "q31", "q15"))


def arm_cfft_tmp_buffer_size(dt, nbSamples, buf_id, arch=None):
    return 0                                  # no user temporary: work space lives on the device


def arm_cfft_output_buffer_size(dt, nbSamples, arch=None):
    return 2 * int(nbSamples)


def arm_cifft_output_buffer_size(dt, nbSamples, arch=None):
    """cmsisdsp_transform.c cmsis_arm_cifft_output_buffer_size ("II|$I", :3032-3050), answered
    by the library's arm_cifft_output_buffer_size (arm_transform_buffer_sizes.c)."""
    return int(_lib.arm_cifft_output_buffer_size(_ARCH_DEFAULT if arch is None else int(arch), int(dt),
                                                 int(nbSamples)))


# ------------------------------------------------------------------ real FFT (fast)
def arm_rfft_fast_init_f32(inst, fftLen):
    return _lib.arm_rfft_fast_init_f32(_C.byref(inst._s), int(fftLen))


def arm_rfft_fast_f32(inst, p, ifftFlag, tmp=None):
    src = _arr(p, _np.float32).copy()
    out = _np.zeros(inst._s.fftLenRFFT, dtype=_np.float32)
    _lib.arm_rfft_fast_f32(_C.byref(inst._s), src.ctypes.data, out.ctypes.data, int(ifftFlag))
    _check("arm_rfft_fast_f32")
    return out


# ------------------------------------------------------------------ real FFT, q31 / q15
# cmsisdsp_transform.c:2275-2313 (init: "Oi|ii"), :2180-2273 / :2317-2405 (rfft: "OO|i$O",
# the ifft / tmp arguments exist for the Neon API only): output fftLenReal words for an
# inverse instance, 2*fftLenReal otherwise; the input is converted (copied) first.
def _rfft_q_init(kind):
    def init(inst, fftLenReal, ifftFlagR=0, bitReverseFlag=0):
        return getattr(_lib, f"arm_rfft_init_{kind}")(_C.byref(inst._s), int(fftLenReal), int(ifftFlagR),
                                                      int(bitReverseFlag))
    init.__name__ = f"arm_rfft_init_{kind}"
    return init


def _rfft_q(kind):
    def rfft(inst, pSrc, ifft=0, tmp=None):
        s = inst._s
        n = int(s.fftLenReal)
        src = _np.zeros(2 * n, dtype=_DT[kind])           # room for the widest read (inverse: N+2)
        x = _arr(pSrc, _DT[kind]).ravel()
        src[:min(x.size, 2 * n)] = x[:2 * n]
        out = _np.zeros(2 * n, dtype=_DT[kind])
        getattr(_lib, f"arm_rfft_{kind}")(_C.byref(s), src.ctypes.data, out.ctypes.data)
        _check(f"arm_rfft_{kind}")
        return out[:n] if s.ifftFlagR else out
    rfft.__name__ = f"arm_rfft_{kind}"
    return rfft


arm_rfft_init_q31 = _rfft_q_init("q31")
arm_rfft_init_q15 = _rfft_q_init("q15")
arm_rfft_q31 = _rfft_q("q31")
arm_rfft_q15 = _rfft_q("q15")


def arm_rfft_tmp_buffer_size(dt, nbSamples, buf_id, arch=None):
    return 0


def arm_rfft_output_buffer_size(dt, nbSamples, arch=None):
    """arm_transform_buffer_sizes.c:204-230 (generic arch): float N, fixed point 2N."""
    from . import datatype as _dt
    return 2 * int(nbSamples) if dt in (_dt.Q31, _dt.Q15) else int(nbSamples)


def arm_rifft_input_buffer_size(dt, nbSamples, arch=None):
    """arm_transform_buffer_sizes.c:245-263: float N, fixed point N + 2."""
    from . import datatype as _dt
    return int(nbSamples) + 2 if dt in (_dt.Q31, _dt.Q15) else int(nbSamples)


# ------------------------------------------------------------------ FIR
def _fir_init(kind):
    def init(inst, numTaps, pCoeffs, pState):
        c = _arr(pCoeffs, _DT[kind])
        state = _arr(pState, _DT[kind]).copy()
        block = max(1, len(state) - int(numTaps) + 1)
        inst._keep = [c, state]
        inst._block = block
        getattr(_lib, f"arm_fir_init_{kind}")(_C.byref(inst._s), int(numTaps), c.ctypes.data, state.ctypes.data, block)
        _check(f"arm_fir_init_{kind}")
        return 0
    init.__name__ = f"arm_fir_init_{kind}"
    return init


def _fir(name, kind):
    def run(inst, pSrc):
        x = _arr(pSrc, _DT[kind])
        if len(x) > inst._block:
            raise ValueError(f"{name}: {len(x)} samples > the blockSize the state was sized for ({inst._block})")
        y = _np.zeros_like(x)
        getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, len(x))
        _check(name)
        return y
    run.__name__ = name
    return run


arm_fir_init_f32, arm_fir_init_q31, arm_fir_init_q15, arm_fir_init_q7 = (_fir_init(k) for k in ("f32", "q31", "q15", "q7"))
arm_fir_q7 = _fir("arm_fir_q7", "q7")
arm_fir_f32 = _fir("arm_fir_f32", "f32")
arm_fir_q31 = _fir("arm_fir_q31", "q31")
arm_fir_q15 = _fir("arm_fir_q15", "q15")
arm_fir_fast_q31 = _fir("arm_fir_fast_q31", "q31")
arm_fir_fast_q15 = _fir("arm_fir_fast_q15", "q15")


# ------------------------------------------------------------------ multirate FIR
# cmsisdsp_filtering.c cmsis_arm_fir_decimate_init_* ("OhiOO": blockSize = len(pState) -
# len(pCoeffs) + 1, :4742-4772) / cmsis_arm_fir_interpolate_init_* ("OihOO", same blockSize
# rule, :5164-5190) return the status; cmsis_arm_fir_decimate_* returns len(pSrc) / M words,
# cmsis_arm_fir_interpolate_* len(pSrc) * L words (:4706-4740, :5128-5160).
def _mr_init(family, kind):
    name = f"arm_fir_{family}_init_{kind}"

    def init(inst, a, b, pCoeffs, pState):
        c = _arr(pCoeffs, _DT[kind])
        state = _arr(pState, _DT[kind]).copy()
        block = len(state) - len(c) + 1
        inst._keep = [c, state]
        st = getattr(_lib, name)(_C.byref(inst._s), int(a), int(b), c.ctypes.data, state.ctypes.data, block)
        _check(name)
        return st
    init.__name__ = name
    return init


def _mr(family, fn, kind):
    name = f"arm_fir_{fn}"

    def run(inst, pSrc):
        x = _arr(pSrc, _DT[kind])
        n = len(x) // inst._s.M if family == "decimate" else len(x) * inst._s.L
        y = _np.zeros(n, dtype=_DT[kind])
        getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, len(x))
        _check(name)
        return y
    run.__name__ = name
    return run


for _k in ("f32", "q31", "q15"):
    globals()[f"arm_fir_decimate_init_{_k}"] = _mr_init("decimate", _k)
    globals()[f"arm_fir_interpolate_init_{_k}"] = _mr_init("interpolate", _k)
    globals()[f"arm_fir_decimate_{_k}"] = _mr("decimate", f"decimate_{_k}", _k)
    globals()[f"arm_fir_interpolate_{_k}"] = _mr("interpolate", f"interpolate_{_k}", _k)
arm_fir_decimate_fast_q15 = _mr("decimate", "decimate_fast_q15", "q15")
arm_fir_decimate_fast_q31 = _mr("decimate", "decimate_fast_q31", "q31")
del _k


# cmsisdsp_filtering.c cmsis_arm_fir_lattice_init_* ("OhOO": S, numStages, pCoeffs, pState) and
# cmsis_arm_fir_lattice_* ("OO": S, pSrc; returns len(pSrc) words).
def _lattice_init(kind):
    name = f"arm_fir_lattice_init_{kind}"

    def init(inst, numStages, pCoeffs, pState):
        c = _arr(pCoeffs, _DT[kind])
        state = _np.zeros(max(len(_np.asarray(pState)), int(numStages)), dtype=_DT[kind])
        inst._keep = [c, state]
        getattr(_lib, name)(_C.byref(inst._s), int(numStages), c.ctypes.data, state.ctypes.data)
        _check(name)
    init.__name__ = name
    return init


def _lattice(kind):
    name = f"arm_fir_lattice_{kind}"

    def run(inst, pSrc):
        x = _arr(pSrc, _DT[kind])
        y = _np.zeros(len(x), dtype=_DT[kind])
        getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, len(x))
        _check(name)
        return y
    run.__name__ = name
    return run


for _k in ("f32", "q31", "q15"):
    globals()[f"arm_fir_lattice_init_{_k}"] = _lattice_init(_k)
    globals()[f"arm_fir_lattice_{_k}"] = _lattice(_k)
del _k


# cmsisdsp_filtering.c cmsis_arm_biquad_cascade_*_init_* ("OiOO" / "OiOOi": S, numStages, pCoeffs, pState
# [, postShift], :3672-3880, :5232-5400) and the processing functions ("OO": S, pSrc; returns len(pSrc)
# words).  The module keeps its own zeroed state of the length the function needs.  Stereo: pSrc holds
# interleaved L,R words and blockSize is len(pSrc) / 2 (the extension passes len(pSrc) and overruns
# its own output buffer).
_BQ_STATE = {"arm_biquad_cascade_df1_init_f32": (4, _np.float32, _np.float32, 5),
             "arm_biquad_cascade_df1_init_q31": (4, _np.int32, _np.int32, 5),
             "arm_biquad_cascade_df1_init_q15": (4, _np.int16, _np.int16, 6),
             "arm_biquad_cas_df1_32x64_init_q31": (4, _np.int64, _np.int32, 5),
             "arm_biquad_cascade_df2T_init_f32": (2, _np.float32, _np.float32, 5),
             "arm_biquad_cascade_stereo_df2T_init_f32": (4, _np.float32, _np.float32, 5)}


def _biquad_init(name, with_shift):
    ks, sdt, cdt, nc = _BQ_STATE[name]

    def init(inst, numStages, pCoeffs, pState, *postShift):
        if len(postShift) != (1 if with_shift else 0):
            raise TypeError(f"{name}: takes {5 if with_shift else 4} arguments")
        c = _arr(pCoeffs, cdt)
        if len(c) < nc * int(numStages):
            raise ValueError(f"{name}: {nc} coefficients per stage")
        state = _np.zeros(max(len(_np.asarray(pState)), ks * int(numStages)), dtype=sdt)
        inst._keep = [c, state]
        getattr(_lib, name)(_C.byref(inst._s), int(numStages), c.ctypes.data, state.ctypes.data,
                            *[int(v) for v in postShift])
        _check(name)
    init.__name__ = name
    return init


def _biquad(name, dt, ch):
    def run(inst, pSrc):
        x = _arr(pSrc, dt)
        y = _np.zeros(len(x), dtype=dt)
        getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, len(x) // ch)
        _check(name)
        return y
    run.__name__ = name
    return run


for _f, (_i, _init, _ps) in _abi.BIQUAD_FUNCS.items():
    globals()[_init] = _biquad_init(_init, _ps is not None)
    globals()[_f] = _biquad(_f, _BQ_STATE[_init][2], 2 if "stereo" in _f else 1)
del _f, _i, _init, _ps


# cmsisdsp_filtering.c cmsis_arm_iir_lattice_init_* ("OhOOO": S, numStages, pkCoeffs, pvCoeffs, pState; the
# extension passes blockSize = len(pkCoeffs), :5652-5812) and cmsis_arm_iir_lattice_* ("OO": S, pSrc; returns
# len(pSrc) words, :5618-5780).  The module keeps its own zeroed state, at least the numStages +
# len(pkCoeffs) words that init clears.
def _iir_lattice_init(name, dt):
    def init(inst, numStages, pkCoeffs, pvCoeffs, pState):
        k, v = _arr(pkCoeffs, dt), _arr(pvCoeffs, dt)
        if len(k) < int(numStages) or len(v) < int(numStages) + 1:
            raise ValueError(f"{name}: numStages reflection and numStages + 1 ladder coefficients")
        state = _np.zeros(max(len(_np.asarray(pState)), int(numStages) + len(k)), dtype=dt)
        inst._keep = [k, v, state]
        getattr(_lib, name)(_C.byref(inst._s), int(numStages), k.ctypes.data, v.ctypes.data, state.ctypes.data, len(k))
        _check(name)
    init.__name__ = name
    return init


def _iir_lattice(name, dt):
    def run(inst, pSrc):
        x = _arr(pSrc, dt)
        y = _np.zeros(len(x), dtype=dt)
        getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, len(x))
        _check(name)
        return y
    run.__name__ = name
    return run


# cmsis_arm_lms*_init_* ("OhOOf" / "OhOOhi" / "OhOOii": S, numTaps, pCoeffs, pState, mu[, postShift];
# blockSize = len(pState) - len(pCoeffs) + 1, :5856-6240) and cmsis_arm_lms* ("OOOO": S, pSrc, pRef, pErr;
# returns pOut, len(pSrc) words, :5814-6210).  The extension works on converted copies, so the error
# signal and the adapted coefficients never reach its caller; here a numpy pErr of the function's dtype
# and len(pSrc) words receives the error, and inst.coeffs() returns the instance's current coefficients.
def _lms_init(name, dt, with_shift):
    def init(inst, numTaps, pCoeffs, pState, mu, *postShift):
        if len(postShift) != (1 if with_shift else 0):
            raise TypeError(f"{name}: takes {7 if with_shift else 6} arguments")
        c = _arr(pCoeffs, dt).copy()
        if len(c) < int(numTaps) or int(numTaps) < 1:
            raise ValueError(f"{name}: numTaps coefficients")
        state = _np.zeros(max(len(_np.asarray(pState)), int(numTaps) - 1), dtype=dt)
        inst._keep = [c, state]
        inst.coeffs = lambda: c[:int(numTaps)].copy()
        getattr(_lib, name)(_C.byref(inst._s), int(numTaps), c.ctypes.data, state.ctypes.data,
                            float(mu) if dt == _np.float32 else int(mu), len(state) - len(c) + 1 if len(state) >= len(c) else 0,
                            *[int(v) for v in postShift])
        _check(name)
    init.__name__ = name
    return init


def _lms(name, dt):
    def run(inst, pSrc, pRef, pErr):
        x, d = _arr(pSrc, dt), _arr(pRef, dt)
        if len(d) < len(x):
            raise ValueError(f"{name}: pRef shorter than pSrc")
        y, e = _np.zeros(len(x), dtype=dt), _np.zeros(len(x), dtype=dt)
        getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, d.ctypes.data, y.ctypes.data, e.ctypes.data, len(x))
        _check(name)
        if isinstance(pErr, _np.ndarray) and pErr.dtype == dt and pErr.shape == e.shape:
            pErr[...] = e
        return y
    run.__name__ = name
    return run


for _f, (_i, _init, _extra) in _abi.ADAPTIVE_FUNCS.items():
    _d = _DT[_f.rsplit("_", 1)[1]]
    if "lattice" in _f:
        globals()[_init], globals()[_f] = _iir_lattice_init(_init, _d), _iir_lattice(_f, _d)
    else:
        globals()[_init], globals()[_f] = _lms_init(_init, _d, len(_extra) == 2), _lms(_f, _d)
del _f, _i, _init, _extra, _d


# cmsisdsp_filtering.c cmsis_arm_fir_sparse_init_* ("OhOOOh": S, numTaps, pCoeffs, pState,
# pTapDelay, maxDelay; blockSize = len(pState) - len(pCoeffs) + 1, :6666-6690) and
# cmsis_arm_fir_sparse_f32 ("OOO": S, pSrc, pScratchIn; returns len(pSrc) words, :6628-6662).
# The module keeps its own state copy of at least maxDelay + blockSize words and refuses a
# block that would not fit it (the C call would run past the caller's state).
def _sparse_init(kind):
    name = f"arm_fir_sparse_init_{kind}"

    def init(inst, numTaps, pCoeffs, pState, pTapDelay, maxDelay):
        c = _arr(pCoeffs, _DT[kind])
        d = _arr(pTapDelay, _np.int32)
        block = max(len(_np.asarray(pState)) - len(c) + 1, 0)
        state = _np.zeros(max(len(_np.asarray(pState)), int(maxDelay) + block), dtype=_DT[kind])
        inst._keep = [c, d, state]
        getattr(_lib, name)(_C.byref(inst._s), int(numTaps), c.ctypes.data, state.ctypes.data, d.ctypes.data,
                            int(maxDelay), block)
        _check(name)
    init.__name__ = name
    return init


def _sparse(kind):
    name = f"arm_fir_sparse_{kind}"

    def run(inst, pSrc, pScratchIn=None, pScratchOut=None):
        x = _arr(pSrc, _DT[kind])
        if inst._s.maxDelay + len(x) > len(inst._keep[2]):
            raise ValueError(f"{name}: maxDelay + len(pSrc) exceeds the state given to the init call")
        y = _np.zeros(len(x), dtype=_DT[kind])
        if kind in ("q15", "q7"):
            getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, None, None, len(x))
        else:
            getattr(_lib, name)(_C.byref(inst._s), x.ctypes.data, y.ctypes.data, None, len(x))
        _check(name)
        return y
    run.__name__ = name
    return run


for _k in ("f32", "q31", "q15", "q7"):
    globals()[f"arm_fir_sparse_init_{_k}"] = _sparse_init(_k)
    globals()[f"arm_fir_sparse_{_k}"] = _sparse(_k)
del _k


# ------------------------------------------------------------------ matrix multiply
def arm_mat_mult_f32(pSrcA, pSrcB):
    """(status, A @ B) as in the reference binding."""
    return _amd.arm_mat_mult_f32(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32))


def arm_mat_mult_q31(pSrcA, pSrcB):
    return _amd.arm_mat_mult_fixed("q31", _arr(pSrcA, _np.int32), _arr(pSrcB, _np.int32))


def arm_mat_mult_opt_q31(pSrcA, pSrcB, pState=None):
    """cmsisdsp_matrix.c cmsis_arm_mat_mult_opt_q31 ("OOO" -> (status, C), :1302-1330)."""
    return _amd.arm_mat_mult_fixed("opt_q31", _arr(pSrcA, _np.int32), _arr(pSrcB, _np.int32))


def arm_mat_mult_q7(pSrcA, pSrcB, pState=None):
    """cmsisdsp_matrix.c cmsis_arm_mat_mult_q7 ("OOO" -> (status, C), :1110-1140)."""
    return _amd.arm_mat_mult_fixed("q7", _arr(pSrcA, _np.int8), _arr(pSrcB, _np.int8))


def arm_mat_mult_q15(pSrcA, pSrcB, pState=None):
    return _amd.arm_mat_mult_fixed("q15", _arr(pSrcA, _np.int16), _arr(pSrcB, _np.int16))


def arm_mat_cmplx_mult_f32(pSrcA, pSrcB):
    """cmsisdsp_matrix.c cmsis_arm_mat_cmplx_mult_f32 (:661-690): real arrays [M, 2K], [K, 2N] of
    interleaved (re, im) words -> (status, C [M, 2N])."""
    return _amd.arm_mat_cmplx_mult("f32", _arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32))


def arm_mat_cmplx_mult_q31(pSrcA, pSrcB):
    """cmsisdsp_matrix.c cmsis_arm_mat_cmplx_mult_q31 (:729-760)."""
    return _amd.arm_mat_cmplx_mult("q31", _arr(pSrcA, _np.int32), _arr(pSrcB, _np.int32))


def arm_mat_cmplx_mult_q15(pSrcA, pSrcB, pScratch):
    """cmsisdsp_matrix.c cmsis_arm_mat_cmplx_mult_q15 ("OOO" -> (status, C), :692-727).  The wrapper
    converts pScratch to a private q15 buffer and frees it, so the caller's array is left as it is;
    here the library writes B transposed into a buffer of the size it needs."""
    b = _arr(pSrcB, _np.int16)
    return _amd.arm_mat_cmplx_mult("q15", _arr(pSrcA, _np.int16), b, _np.zeros(max(b.size, 1), dtype=_np.int16))


def arm_mat_inverse_f32(src):
    """cmsisdsp_matrix.c cmsis_arm_mat_inverse_f32 (:1832-1860): (status, dst).  The wrapper inverts a private
    copy, so the caller's array is left as it is."""
    return _amd.arm_mat_inverse(_arr(src, _np.float32))


def arm_mat_cholesky_f32(src):
    """cmsis_arm_mat_cholesky_f32 (:1896-1933): (status, dst), dst zero-filled before the call as there, so its
    strict upper triangle is zero."""
    return _amd.arm_mat_cholesky(_arr(src, _np.float32))


def arm_mat_ldlt_f32(src):
    """cmsis_arm_mat_ldlt_f32 (:1977-2015): (status, l, d, perm), perm an int16 array as there."""
    st, l, d, pp = _amd.arm_mat_ldlt(_arr(src, _np.float32))
    return st, l, d, pp.view(_np.int16)


def arm_mat_solve_lower_triangular_f32(pSrcA, pSrcB):
    """cmsis_arm_mat_solve_lower_triangular_f32 (:2063-2098): (status, x) with pSrcA x = pSrcB [n, cols]."""
    return _amd.arm_mat_solve_lower_triangular(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32))


def arm_mat_solve_upper_triangular_f32(pSrcA, pSrcB):
    """cmsis_arm_mat_solve_upper_triangular_f32 (:2137-2171)."""
    return _amd.arm_mat_solve_upper_triangular(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32))


def _mat_basic(name, kind, doc):
    """One of the 20 element-wise, transpose and matrix-vector bindings (cmsisdsp_matrix.c)."""
    op = name[len("arm_mat_"):-len(kind) - 1]
    dt = _DT[kind]
    if op in ("add", "sub"):
        def run(pSrcA, pSrcB):
            return getattr(_amd, f"arm_mat_{op}")(kind, _arr(pSrcA, dt), _arr(pSrcB, dt))
    elif op == "scale" and kind == "f32":
        def run(pSrc, scale):
            return _amd.arm_mat_scale(kind, _arr(pSrc, dt), scale)
    elif op == "scale":
        def run(pSrc, scaleFract, shift):
            return _amd.arm_mat_scale(kind, _arr(pSrc, dt), scaleFract, shift)
    elif op == "vec_mult":
        def run(pSrcA, pSrcB):
            return _amd.arm_mat_vec_mult(kind, _arr(pSrcA, dt), _arr(pSrcB, dt))
    else:
        def run(pSrc):
            return getattr(_amd, f"arm_mat_{op}")(kind, _arr(pSrc, dt))
    run.__name__ = name
    run.__doc__ = doc
    return run


arm_mat_add_f32 = _mat_basic("arm_mat_add_f32", "f32", """cmsisdsp_matrix.c cmsis_arm_mat_add_f32 ("OO", :421-454):
    (status, dst); dst is created [pSrcA rows, pSrcB cols] as there.""")
arm_mat_add_q15 = _mat_basic("arm_mat_add_q15", "q15", """cmsis_arm_mat_add_q15 ("OO", :458-494): (status, dst), int16
    words, saturating.""")
arm_mat_add_q31 = _mat_basic("arm_mat_add_q31", "q31", """cmsis_arm_mat_add_q31 ("OO", :497-532): (status, dst), int32
    words, saturating.""")
arm_mat_sub_f32 = _mat_basic("arm_mat_sub_f32", "f32", """cmsis_arm_mat_sub_f32 ("OO", :1380-1413): (status, dst); dst is
    created [pSrcA rows, pSrcB cols].""")
arm_mat_sub_q15 = _mat_basic("arm_mat_sub_q15", "q15", """cmsis_arm_mat_sub_q15 ("OO", :1453-1487): (status, dst),
    saturating.""")
arm_mat_sub_q31 = _mat_basic("arm_mat_sub_q31", "q31", """cmsis_arm_mat_sub_q31 ("OO", :1490-1524): (status, dst),
    saturating.""")
arm_mat_scale_f32 = _mat_basic("arm_mat_scale_f32", "f32", """cmsis_arm_mat_scale_f32 ("Of", :1527-1556): (status, dst)
    with dst = pSrc * scale, the shape of pSrc.""")
arm_mat_scale_q15 = _mat_basic("arm_mat_scale_q15", "q15", """cmsis_arm_mat_scale_q15 ("Ohi", :1560-1590): (status, dst)
    from scaleFract (a q15 word) and shift; a shift outside -16..15 gives ARM_MATH_ARGUMENT_ERROR and a zero
    dst here (undefined in the reference).""")
arm_mat_scale_q31 = _mat_basic("arm_mat_scale_q31", "q31", """cmsis_arm_mat_scale_q31 ("Oii", :1594-1624): (status, dst)
    from scaleFract (a q31 word) and shift; a shift outside -1..30 gives ARM_MATH_ARGUMENT_ERROR and a zero dst
    here (undefined in the reference).""")
arm_mat_trans_f32 = _mat_basic("arm_mat_trans_f32", "f32", """cmsis_arm_mat_trans_f32 ("O", :782-810): (status, dst),
    dst created [pSrc cols, pSrc rows].""")
arm_mat_trans_q7 = _mat_basic("arm_mat_trans_q7", "q7", """cmsis_arm_mat_trans_q7 ("O", :844-872): (status, dst), int8
    words.""")
arm_mat_trans_q15 = _mat_basic("arm_mat_trans_q15", "q15", """cmsis_arm_mat_trans_q15 ("O", :875-904): (status, dst),
    int16 words.""")
arm_mat_trans_q31 = _mat_basic("arm_mat_trans_q31", "q31", """cmsis_arm_mat_trans_q31 ("O", :907-935): (status, dst),
    int32 words.""")
arm_mat_cmplx_trans_f32 = _mat_basic("arm_mat_cmplx_trans_f32", "f32", """cmsis_arm_mat_cmplx_trans_f32 ("O", :535-574):
    a real array [R, 2C] of interleaved (re, im) words -> (status, dst [C, 2R]); the wrapper halves numCols
    before the call, as here.""")
arm_mat_cmplx_trans_q31 = _mat_basic("arm_mat_cmplx_trans_q31", "q31", """cmsis_arm_mat_cmplx_trans_q31 ("O", :577-616):
    [R, 2C] int32 -> (status, dst [C, 2R]).""")
arm_mat_cmplx_trans_q15 = _mat_basic("arm_mat_cmplx_trans_q15", "q15", """cmsis_arm_mat_cmplx_trans_q15 ("O", :619-658):
    [R, 2C] int16 -> (status, dst [C, 2R]).""")
arm_mat_vec_mult_f32 = _mat_basic("arm_mat_vec_mult_f32", "f32", """cmsis_arm_mat_vec_mult_f32 ("OO", :938-968): the
    matrix and a vector of numCols words -> dst, a 1-D array of numRows words; no status (the C function
    returns void).""")
arm_mat_vec_mult_q15 = _mat_basic("arm_mat_vec_mult_q15", "q15", """cmsis_arm_mat_vec_mult_q15 ("OO", :1044-1074): -> dst,
    numRows int16 words; keeps the reference's 16-bit row offset (INTEGRATION.md).""")
arm_mat_vec_mult_q7 = _mat_basic("arm_mat_vec_mult_q7", "q7", """cmsis_arm_mat_vec_mult_q7 ("OO", :1077-1107): -> dst,
    numRows int8 words.""")
arm_mat_vec_mult_q31 = _mat_basic("arm_mat_vec_mult_q31", "q31", """cmsis_arm_mat_vec_mult_q31 ("OO", :1233-1263): -> dst,
    numRows int32 words; keeps the reference's 16-bit row offset (INTEGRATION.md).""")


def _cmplx_math(name, doc):
    """One of the 26 complex-math and max / min bindings (cmsisdsp_complexf.c, cmsisdsp_statistics.c)."""
    op, kind = name[len("arm_"):].rsplit("_", 1)
    dt = _DT[kind]
    if op in ("max", "min"):
        def run(pSrc):
            v, i = getattr(_amd, f"arm_{op}")(kind, _arr(pSrc, dt))
            return (float(v) if kind == "f32" else int(v)), int(i)
    elif op == "cmplx_dot_prod":
        def run(pSrcA, pSrcB):
            re, im = _amd.arm_cmplx_dot_prod(kind, _arr(pSrcA, dt), _arr(pSrcB, dt))
            return (float(re), float(im)) if kind == "f32" else (int(re), int(im))
    elif op in ("cmplx_mult_cmplx", "cmplx_mult_real"):
        def run(pSrcA, pSrcB):
            return getattr(_amd, f"arm_{op}")(kind, _arr(pSrcA, dt), _arr(pSrcB, dt))
    else:
        def run(pSrc):
            return getattr(_amd, f"arm_{op}")(kind, _arr(pSrc, dt))
    run.__name__ = name
    run.__doc__ = doc
    return run


for _t in ("f32", "q31", "q15"):
    for _op, _doc in (
            ("mag", "(pSrc) -> pDst: numSamples = len(pSrc) / 2 magnitudes, one word per complex sample."),
            ("mag_squared", "(pSrc) -> pDst: len(pSrc) / 2 squared magnitudes."),
            ("conj", "(pSrc) -> pDst: the conjugates, interleaved, as long as pSrc."),
            ("mult_cmplx", "(pSrcA, pSrcB) -> pDst: the products, interleaved; numSamples = len(pSrcA) / 2."),
            ("mult_real", "(pSrcCmplx, pSrcReal) -> pCmplxDst: interleaved; numSamples = len(pSrcCmplx) / 2."),
            ("dot_prod", "(pSrcA, pSrcB) -> (realResult, imagResult), two Python numbers (f32: float; q31: the two "
                         "64-bit sums; q15: q31 words).")):
        _n = f"arm_cmplx_{_op}_{_t}"
        globals()[_n] = _cmplx_math(_n, f"cmsisdsp_complexf.c cmsis_{_n} {_doc}")
for _t in ("f32", "q31", "q15", "q7"):
    for _op in ("max", "min"):
        _n = f"arm_{_op}_{_t}"
        globals()[_n] = _cmplx_math(_n, f"cmsisdsp_statistics.c cmsis_{_n} (pSrc) -> (pResult, pIndex): the {_op}imum "
                                        "and the first index that holds it; blockSize = len(pSrc).")


def _statistics(name, doc):
    """One of the statistics bindings (cmsisdsp_statistics.c): a Python number, or (value, index)."""
    op, kind = name[len("arm_"):].rsplit("_", 1)
    dt = _DT[kind]
    num = float if kind == "f32" else int
    if op in ("absmax", "absmin"):
        def run(pSrc):
            v, i = getattr(_amd, f"arm_{op}")(kind, _arr(pSrc, dt))
            return num(v), int(i)
    elif op == "mse":
        def run(pSrcA, pSrcB):
            return num(_amd.arm_stat(op, kind, _arr(pSrcA, dt), _arr(pSrcB, dt)))
    else:
        def run(pSrc):
            return num(_amd.arm_stat(op, kind, _arr(pSrc, dt)))
    run.__name__ = name
    run.__doc__ = doc
    return run


for _t in ("f32", "q31", "q15", "q7"):
    _ops = [("mean", "(pSrc) -> pResult: the mean, truncated toward zero in fixed point."),
            ("power", "(pSrc) -> pResult: the sum of squares (f32: float; q31, q15: a 64-bit int; q7: q31)."),
            ("mse", "(pSrcA, pSrcB) -> pResult: the mean squared error."),
            ("max_no_idx", "(pSrc) -> pResult: the maximum."), ("min_no_idx", "(pSrc) -> pResult: the minimum."),
            ("absmax_no_idx", "(pSrc) -> pResult: the maximum of |x|."),
            ("absmin_no_idx", "(pSrc) -> pResult: the minimum of |x|."),
            ("absmax", "(pSrc) -> (pResult, pIndex): the maximum of |x| and the first index that holds it."),
            ("absmin", "(pSrc) -> (pResult, pIndex): the minimum of |x| and the first index that holds it.")]
    if _t != "q7":
        _ops += [("rms", "(pSrc) -> pResult: the root mean square."),
                 ("var", "(pSrc) -> pResult: the unbiased variance."),
                 ("std", "(pSrc) -> pResult: the standard deviation.")]
    if _t == "f32":
        _ops += [("accumulate", "(pSrc) -> pResult: the ordered sum.")]
    for _op, _doc in _ops:
        _n = f"arm_{_op}_{_t}"
        globals()[_n] = _statistics(_n, f"cmsisdsp_statistics.c cmsis_{_n} {_doc}  blockSize = len(pSrc).")


def _basic_math(name, doc):
    """One of the basic math bindings (cmsisdsp_basic.c): an array as long as pSrc, or dot_prod's Python number."""
    op, kind = name[len("arm_"):].rsplit("_", 1)
    dt = _amd._BASIC_DT[kind]
    if op == "dot_prod":
        def run(pSrcA, pSrcB):
            return (float if kind == "f32" else int)(_amd.arm_dot_prod(kind, _arr(pSrcA, dt), _arr(pSrcB, dt)))
    elif op in _amd._BASIC_TWO:
        def run(pSrcA, pSrcB):
            return _amd.arm_basic2(op, kind, _arr(pSrcA, dt), _arr(pSrcB, dt))
    else:
        def run(pSrc, *scalars):
            return _amd.arm_basic1(op, kind, _arr(pSrc, dt), *scalars)
    run.__name__ = name
    run.__doc__ = doc
    return run


for _t in ("f32", "q31", "q15", "q7"):
    _ops = [("add", "(pSrcA, pSrcB) -> pDst"), ("sub", "(pSrcA, pSrcB) -> pDst"), ("mult", "(pSrcA, pSrcB) -> pDst"),
            ("offset", "(pSrc, offset) -> pDst"), ("clip", "(pSrc, low, high) -> pDst"), ("abs", "(pSrc) -> pDst"),
            ("negate", "(pSrc) -> pDst"),
            ("scale", "(pSrc, scale) -> pDst" if _t == "f32" else "(pSrc, scaleFract, shift) -> pDst"),
            ("dot_prod", "(pSrcA, pSrcB) -> result, a Python number (f32: float; q31, q15: a 64-bit int; q7: q31)")]
    if _t != "f32":
        _ops += [("shift", "(pSrc, shiftBits) -> pDst")]
    for _op, _doc in _ops:
        _n = f"arm_{_op}_{_t}"
        globals()[_n] = _basic_math(_n, f"cmsisdsp_basic.c cmsis_{_n} {_doc}; blockSize = len(pSrc).")
for _t in ("u32", "u16", "u8"):
    for _op, _doc in (("and", "(pSrcA, pSrcB)"), ("or", "(pSrcA, pSrcB)"), ("xor", "(pSrcA, pSrcB)"), ("not", "(pSrc)")):
        _n = f"arm_{_op}_{_t}"
        globals()[_n] = _basic_math(_n, f"cmsisdsp_basic.c cmsis_{_n} {_doc} -> pDst; blockSize = len(pSrc).")


# ------------------------------------------------------------------ support functions (cmsisdsp_support.c)
class arm_sort_instance_f32(_Instance):
    """cmsisdsp_support.c arm_sort_instance_f32(alg=0, dir=0) with the accessors alg() and dir()."""
    _struct = _abi.arm_sort_instance_f32

    def __init__(self, alg=0, dir=0):
        super().__init__()
        self._s.alg, self._s.dir = int(alg), int(dir)


def arm_sort_init_f32(S, alg, dir):
    """cmsisdsp_support.c cmsis_arm_sort_init_f32 (S, alg, dir)."""
    _amd.arm_sort_init_f32(S._s, alg, dir)


def arm_sort_f32(S, pSrc):
    """cmsisdsp_support.c cmsis_arm_sort_f32 (S, pSrc) -> pDst; blockSize = len(pSrc)."""
    return _amd.arm_sort_f32(S._s, _arr(pSrc, _np.float32))


def _support_convert(name, src, dst):
    def run(pSrc):
        return _amd.arm_convert(src, dst, _arr(pSrc, _DT[src]))
    run.__name__ = name
    run.__doc__ = f"cmsisdsp_support.c cmsis_{name} (pSrc) -> pDst; blockSize = len(pSrc)."
    return run


def _support_fill(kind):
    def run(value, blockSize):
        return _amd.arm_fill(kind, value, blockSize)
    run.__name__ = f"arm_fill_{kind}"
    run.__doc__ = f"cmsisdsp_support.c cmsis_arm_fill_{kind} (value, blockSize) -> pDst."
    return run


for _s in ("f32", "q31", "q15", "q7"):
    for _d in ("f32", "q31", "q15", "q7"):
        _n = _amd._support_name(_s, _d)
        globals()[_n] = _support_convert(_n, _s, _d)
    globals()[f"arm_fill_{_s}"] = _support_fill(_s)


def arm_weighted_average_f32(pSrcA, pSrcB):
    """cmsisdsp_support.c cmsis_arm_weighted_average_f32 (in, weights) -> a Python float; blockSize = len(in)."""
    return float(_amd.arm_weighted_average_f32(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32)))


def arm_barycenter_f32(pSrcA, pSrcB, nbVectors, vecDim):
    """cmsisdsp_support.c cmsis_arm_barycenter_f32 (in, weights, nbVectors, vecDim) -> out [vecDim]."""
    return _amd.arm_barycenter_f32(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32), int(nbVectors), int(vecDim))


# ------------------------------------------------------------------ distance functions
ARM_DTW_SAKOE_CHIBA_WINDOW = _amd.ARM_DTW_SAKOE_CHIBA_WINDOW
ARM_DTW_SLANTED_BAND_WINDOW = _amd.ARM_DTW_SLANTED_BAND_WINDOW


def _distance_f32(name):
    def run(pSrcA, pSrcB):
        return float(_amd.arm_distance_f32(name, _arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32)))
    run.__name__ = f"arm_{name}_distance_f32"
    run.__doc__ = f"cmsisdsp_distance.c cmsis_arm_{name}_distance_f32 (pSrcA, pSrcB) -> a Python float; blockSize = " \
                  "len(pSrcA).  The operands are copied (the reference's binding copies them too)."
    return run


def _distance_bool(name):
    def run(pSrcA, pSrcB, numberOfBools):
        return float(_amd.arm_boolean_distance(name, _arr(pSrcA, _np.uint32), _arr(pSrcB, _np.uint32),
                                               int(numberOfBools)))
    run.__name__ = f"arm_{name}_distance"
    run.__doc__ = f"cmsisdsp_distance.c cmsis_arm_{name}_distance (pSrcA, pSrcB, numberOfBools) -> a Python float."
    return run


for _n in _amd.DISTANCE_F32:
    globals()[f"arm_{_n}_distance_f32"] = _distance_f32(_n)
for _n in _amd.DISTANCE_BOOL:
    globals()[f"arm_{_n}_distance"] = _distance_bool(_n)


def arm_dtw_init_window_q7(windowType, windowSize, pWindow):
    """cmsisdsp_distance.c cmsis_arm_dtw_init_window_q7 (type, size, window matrix) -> (status, window): the shape is
    taken from pWindow; an unknown type returns the status and a copy of pWindow."""
    w = _arr(pWindow, _np.int8)
    st, out = _amd.arm_dtw_init_window_q7(windowType, windowSize, w.shape[0], w.shape[1])
    return int(st), (out if st == 0 else w.copy())


def arm_dtw_distance_f32(pDistance, pWindow):
    """cmsisdsp_distance.c cmsis_arm_dtw_distance_f32 (distance matrix, window matrix or None) -> (status, distance,
    dtw cost matrix)."""
    st, value, cost = _amd.arm_dtw_distance_f32(_arr(pDistance, _np.float32),
                                                None if pWindow is None else _arr(pWindow, _np.int8))
    return int(st), float(value), cost


def arm_dtw_path_f32(pDTW):
    """cmsisdsp_distance.c cmsis_arm_dtw_path_f32 (cost matrix) -> the path as 2 * pathLength int16 words."""
    return _amd.arm_dtw_path_f32(_arr(pDTW, _np.float32)).reshape(-1)


# ------------------------------------------------------------------ vexp / vlog, log-domain statistics, SVM, Bayes
def arm_vexp_f32(pSrc):
    """cmsisdsp_fastmath.c cmsis_arm_vexp_f32 (pSrc) -> pDst; blockSize = len(pSrc)."""
    return _amd.arm_fast_math_f32("vexp", _arr(pSrc, _np.float32))


def arm_vlog_f32(pSrc):
    """cmsisdsp_fastmath.c cmsis_arm_vlog_f32 (pSrc) -> pDst; blockSize = len(pSrc)."""
    return _amd.arm_fast_math_f32("vlog", _arr(pSrc, _np.float32))


def arm_entropy_f32(pSrc):
    """cmsisdsp_statistics.c cmsis_arm_entropy_f32 (pSrc) -> a Python float; blockSize = len(pSrc)."""
    return float(_amd.arm_logdom_f32("entropy", _arr(pSrc, _np.float32)))


def arm_logsumexp_f32(pSrc):
    """cmsisdsp_statistics.c cmsis_arm_logsumexp_f32 (pSrc) -> a Python float; blockSize = len(pSrc)."""
    return float(_amd.arm_logdom_f32("logsumexp", _arr(pSrc, _np.float32)))


def arm_kullback_leibler_f32(pSrcA, pSrcB):
    """cmsisdsp_statistics.c cmsis_arm_kullback_leibler_f32 (pSrcA, pSrcB) -> a Python float; blockSize = len(pSrcA)."""
    return float(_amd.arm_logdom_f32("kullback_leibler", _arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32)))


def arm_logsumexp_dot_prod_f32(pSrcA, pSrcB):
    """cmsisdsp_statistics.c cmsis_arm_logsumexp_dot_prod_f32 (pSrcA, pSrcB) -> a Python float; the binding
    allocates the scratch buffer."""
    return float(_amd.arm_logdom_f32("logsumexp_dot_prod", _arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32)))


class _SvmInstance(_Instance):
    """cmsisdsp_svm.c: every constructor argument is optional and may be given by keyword; the arrays are copied."""
    _kind = None
    _extra = ()

    def __init__(self, nbOfSupportVectors=0, vectorDimension=0, intercept=0.0, dualCoefficients=None,
                 supportVectors=None, classes=None, **extra):
        super().__init__()
        unknown = set(extra) - set(self._extra)
        if unknown:
            raise TypeError(f"unexpected keyword argument {sorted(unknown)[0]!r}")
        if dualCoefficients is not None and supportVectors is not None and classes is not None:
            _svm_fill(self, nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes,
                      [extra.get(k, 0) for k in self._extra])


def _svm_fill(S, nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes, extra):
    nsv, dim = int(nbOfSupportVectors), int(vectorDimension)
    dual = _arr(dualCoefficients, _np.float32).reshape(-1)[:nsv]
    vectors = _arr(supportVectors, _np.float32).reshape(-1)[:nsv * dim].reshape(nsv, dim)
    names = dict(zip(S._extra, extra))
    S._s, S._keep = _amd.svm_instance(S._kind, intercept, dual, vectors, _arr(classes, _np.int32).reshape(-1)[:2],
                                      **names)


def _svm(kind, extra):
    inst = type(f"arm_svm_{kind}_instance_f32", (_SvmInstance,),
                {"_struct": _abi.SVM_KINDS[kind][0], "_kind": kind, "_extra": extra})

    def init(S, nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes, *rest):
        if len(rest) != len(extra):
            raise TypeError(f"arm_svm_{kind}_init_f32 takes {7 + len(extra)} arguments")
        _svm_fill(S, nbOfSupportVectors, vectorDimension, intercept, dualCoefficients, supportVectors, classes, rest)
    init.__name__ = f"arm_svm_{kind}_init_f32"
    init.__doc__ = f"cmsisdsp_svm.c cmsis_arm_svm_{kind}_init_f32 (S, nbOfSupportVectors, vectorDimension, intercept, " \
                   f"dualCoefficients, supportVectors, classes{''.join(', ' + e for e in extra)})."

    def predict(S, pSrc):
        return _amd.arm_svm_predict_f32(kind, S._s, _arr(pSrc, _np.float32))
    predict.__name__ = f"arm_svm_{kind}_predict_f32"
    predict.__doc__ = f"cmsisdsp_svm.c cmsis_arm_svm_{kind}_predict_f32 (S, pSrc) -> the class, a Python int."
    return inst, init, predict


for _k, _e in (("linear", ()), ("polynomial", ("degree", "coef0", "gamma")), ("rbf", ("gamma",))):
    (globals()[f"arm_svm_{_k}_instance_f32"], globals()[f"arm_svm_{_k}_init_f32"],
     globals()[f"arm_svm_{_k}_predict_f32"]) = _svm(_k, _e)
del _k, _e


class arm_gaussian_naive_bayes_instance_f32(_Instance):
    """cmsisdsp_bayes.c: (vectorDimension, numberOfClasses, theta, sigma, classPriors, epsilon), all optional and
    accepted by keyword; the arrays are copied."""
    _struct = _abi.arm_gaussian_naive_bayes_instance_f32

    def __init__(self, vectorDimension=0, numberOfClasses=0, theta=None, sigma=None, classPriors=None, epsilon=0.0):
        super().__init__()
        if theta is not None and sigma is not None and classPriors is not None:
            c, d = int(numberOfClasses), int(vectorDimension)
            self._s, self._keep = _amd.bayes_instance(_arr(theta, _np.float32).reshape(-1)[:c * d].reshape(c, d),
                                                      _arr(sigma, _np.float32).reshape(-1)[:c * d].reshape(c, d),
                                                      _arr(classPriors, _np.float32).reshape(-1)[:c], epsilon)


def arm_gaussian_naive_bayes_predict_f32(S, pSrc):
    """cmsisdsp_bayes.c cmsis_arm_gaussian_naive_bayes_predict_f32 (S, pSrc) -> (pOutputProbabilities, index)."""
    return _amd.arm_gaussian_naive_bayes_predict_f32(S._s, _arr(pSrc, _np.float32))


def arm_sqrt_q15(x):
    """cmsisdsp_fastmath.c cmsis_arm_sqrt_q15 (in) -> (status, pOut)."""
    st, v = _amd.arm_sqrt_q15(x)
    return int(st), int(v)


def arm_cmplx_mag_fast_q15(pSrc):
    """cmsisdsp_complexf.c cmsis_arm_cmplx_mag_fast_q15 (pSrc) -> pDst: numSamples = len(pSrc) / 2 magnitudes."""
    return _amd.arm_cmplx_mag_fast_q15(_arr(pSrc, _np.int16))


def arm_mat_mult_fast_q31(pSrcA, pSrcB):
    """cmsisdsp_matrix.c cmsis_arm_mat_mult_fast_q31: (status, C)."""
    return _amd.arm_mat_mult_fixed("fast_q31", _arr(pSrcA, _np.int32), _arr(pSrcB, _np.int32))


def arm_mat_mult_fast_q15(pSrcA, pSrcB, pState=None):
    return _amd.arm_mat_mult_fixed("fast_q15", _arr(pSrcA, _np.int16), _arr(pSrcB, _np.int16))


# ------------------------------------------------------------------ interpolation (cmsisdsp_interpolation.c)
class arm_linear_interp_instance_f32(_Instance):
    """cmsisdsp_interpolation.c: (nValues, x1, xSpacing, pYData), each optional and by keyword; the table is copied."""
    _struct = _abi.arm_linear_interp_instance_f32

    def __init__(self, nValues=0, x1=0.0, xSpacing=0.0, pYData=None):
        super().__init__()
        if pYData is not None:
            self._s, keep = _amd.linear_interp_instance(x1, xSpacing, _arr(pYData, _np.float32).reshape(-1)[:int(nValues)])
            self._keep = [keep]


def _bilinear_instance(kind, dt):
    class _Bilinear(_Instance):
        _struct = _abi.arm_bilinear_interp_instance

        def __init__(self, numRows=0, numCols=0, pData=None):
            super().__init__()
            if pData is not None:
                table = _arr(pData, dt).reshape(-1)[:int(numRows) * int(numCols)].reshape(int(numRows), int(numCols))
                self._s, keep = _amd.bilinear_interp_instance(kind, table)
                self._keep = [keep]
    _Bilinear.__name__ = f"arm_bilinear_interp_instance_{kind}"
    _Bilinear.__doc__ = "cmsisdsp_interpolation.c: (numRows, numCols, pData), each optional and by keyword."
    return _Bilinear


for _k, _dt in (("f32", _np.float32), ("q31", _np.int32), ("q15", _np.int16), ("q7", _np.int8)):
    globals()[f"arm_bilinear_interp_instance_{_k}"] = _bilinear_instance(_k, _dt)


class arm_spline_instance_f32(_Instance):
    """cmsisdsp_interpolation.c: filled by arm_spline_init_f32."""
    _struct = _abi.arm_spline_instance_f32

    def __init__(self, type=0, x=None, y=None, n_x=0):
        super().__init__()
        self._s.type = int(type)


def arm_linear_interp_f32(S, x):
    """cmsisdsp_interpolation.c cmsis_arm_linear_interp_f32 (S, x) -> a Python float (computed on the host)."""
    return float(_amd.arm_linear_interp("f32", S._s, x))


def arm_bilinear_interp_f32(S, X, Y):
    """cmsisdsp_interpolation.c cmsis_arm_bilinear_interp_f32 (S, X, Y) -> a Python float (computed on the host)."""
    return float(_amd.arm_bilinear_interp("f32", S._s, X, Y))


def _interp_fixed(kind, dt):
    def linear(pYData, x, nValues):
        return int(_amd.arm_linear_interp(kind, _arr(pYData, dt).reshape(-1)[:int(nValues)], x))

    def bilinear(S, X, Y):
        return int(_amd.arm_bilinear_interp(kind, S._s, X, Y))
    linear.__name__, bilinear.__name__ = f"arm_linear_interp_{kind}", f"arm_bilinear_interp_{kind}"
    linear.__doc__ = (f"cmsisdsp_interpolation.c cmsis_arm_linear_interp_{kind} (pYData, x, nValues) -> an int; x is "
                      "12.20 (computed on the host).")
    bilinear.__doc__ = (f"cmsisdsp_interpolation.c cmsis_arm_bilinear_interp_{kind} (S, X, Y) -> an int; X and Y are "
                        "12.20 (computed on the host).")
    return linear, bilinear


for _k, _dt in (("q31", _np.int32), ("q15", _np.int16), ("q7", _np.int8)):
    globals()[f"arm_linear_interp_{_k}"], globals()[f"arm_bilinear_interp_{_k}"] = _interp_fixed(_k, _dt)


def arm_spline_init_f32(S, type, pX, pY):
    """cmsisdsp_interpolation.c cmsis_arm_spline_init_f32 (S, type, x, y) -> 0; n = len(x); the binding allocates the
    coefficients and the scratch buffer."""
    x, y = _arr(pX, _np.float32).reshape(-1), _arr(pY, _np.float32).reshape(-1)
    n = x.size
    coeffs, temp = _np.zeros(max(1, 3 * (n - 1)), _np.float32), _np.zeros(max(1, 2 * n - 1), _np.float32)
    S._s.type = int(type)
    _lib.arm_spline_init_f32(_C.byref(S._s), int(type), x.ctypes.data, y.ctypes.data, n, coeffs.ctypes.data,
                             temp.ctypes.data)
    _check("arm_spline_init_f32")
    S._keep = [x, y, coeffs]
    return 0


def arm_spline_f32(S, pSrc):
    """cmsisdsp_interpolation.c cmsis_arm_spline_f32 (S, xq) -> the values; blockSize = len(xq)."""
    xq = _arr(pSrc, _np.float32).reshape(-1)
    out = _np.zeros(xq.size, _np.float32)
    _lib.arm_spline_f32(_C.byref(S._s), xq.ctypes.data, out.ctypes.data, xq.size)
    _check("arm_spline_f32")
    return out


# ------------------------------------------------------------------ quaternions (cmsisdsp_quaternion.c)
def _quaternion(name):
    def run(pSrc):
        return _amd.arm_quaternion_f32(name, _arr(pSrc, _np.float32))
    wa, wd = _abi.QUATERNION_FUNCS[name]
    run.__name__ = f"arm_{name}_f32"
    run.__doc__ = (f"cmsisdsp_quaternion.c cmsis_arm_{name}_f32 (pSrc) -> {wd} words per item; nbQuaternions = "
                   f"len(pSrc) // {wa}.")
    return run


for _f in _abi.QUATERNION_FUNCS:
    globals()[f"arm_{_f}_f32"] = _quaternion(_f)


def arm_quaternion_product_f32(pSrcA, pSrcB):
    """cmsisdsp_quaternion.c cmsis_arm_quaternion_product_f32 (pSrcA, pSrcB) -> 4 words per item; nbQuaternions =
    len(pSrcA) // 4."""
    return _amd.arm_quaternion_product_f32(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32))


def arm_quaternion_product_single_f32(pSrcA, pSrcB):
    """cmsisdsp_quaternion.c cmsis_arm_quaternion_product_single_f32 (pSrcA, pSrcB) -> the 4 words of one product."""
    return _amd.arm_quaternion_product_f32(_arr(pSrcA, _np.float32), _arr(pSrcB, _np.float32), single=True)


# ------------------------------------------------------------------ convolution
def _conv(kind, dt):
    def run(pSrcA, srcALen, pSrcB, srcBLen):
        """Full linear convolution, srcALen + srcBLen - 1 samples (reference binding
        PythonWrapper/cmsisdsp_pkg/src/cmsisdsp_filtering.c cmsis_arm_conv_*)."""
        a = _arr(pSrcA, dt)[:int(srcALen)]
        b = _arr(pSrcB, dt)[:int(srcBLen)]
        return _amd.arm_conv(kind, a, b)
    run.__name__ = f"arm_conv_{kind}"
    return run


arm_conv_f32 = _conv("f32", _np.float32)
arm_conv_q15 = _conv("q15", _np.int16)
arm_conv_q31 = _conv("q31", _np.int32)
arm_conv_q7 = _conv("q7", _np.int8)


# cmsisdsp_filtering.c cmsis_arm_conv_fast_* ("OiOi", srcALen + srcBLen - 1 words),
# cmsis_arm_correlate_* ("OiOi", 2 * max(srcALen, srcBLen) - 1 words, :6244-6276) and
# cmsis_arm_conv_partial_* ("OiOiii" -> (status, srcALen + srcBLen - 1 words), :4313-4350).
# The binding's output buffer is uninitialised where the C function does not write; here
# those words are zero.
def _conv_family(fn):
    dt = _DT[fn.split("_")[-1]]

    def run(pSrcA, srcALen, pSrcB, srcBLen, *partial):
        a = _arr(pSrcA, dt)[:int(srcALen)]
        b = _arr(pSrcB, dt)[:int(srcBLen)]
        y, st = _amd.arm_conv_family(fn, a, b, *[int(v) for v in partial])
        return (st, y) if partial else y
    run.__name__ = f"arm_{fn}"
    return run


for _fn in ("conv_fast_q15", "conv_fast_q31", "correlate_f32", "correlate_q15", "correlate_q31", "correlate_fast_q15",
            "correlate_fast_q31", "conv_partial_f32", "conv_partial_q15", "conv_partial_q31", "conv_partial_fast_q15",
            "conv_partial_fast_q31", "correlate_q7", "conv_partial_q7"):
    globals()[f"arm_{_fn}"] = _conv_family(_fn)
del _fn


# The scratch-buffer ("_opt") forms, cmsisdsp_filtering.c cmsis_arm_conv_opt_q15 / _q7 /
# _fast_opt_q15 ("OiOiOO", :3993, :4231, :4112), cmsis_arm_correlate_opt_q15 / _fast_opt_q15
# ("OiOiO", :6316, :6431), cmsis_arm_correlate_opt_q7 ("OiOiOO", :6546) -> the output words;
# cmsis_arm_conv_partial_opt_q15 / _q7 / _fast_opt_q15 ("OiOiiiOO", :4354, :4616, :4485) ->
# (status, srcALen + srcBLen - 1 words).  The caller's scratch arrays are accepted and not
# touched: the C call gets scratch of its own, sized as the reference requires
# (pScratch1 srcALen + 2 srcBLen - 2 q15 words, pScratch2 min(srcALen, srcBLen)).
def _conv_opt(fn):
    dt = _DT[fn.split("_")[-1]]
    n_scratch = _abi.CONV_OPT_FULL.get(fn, 2)

    def run(pSrcA, srcALen, pSrcB, srcBLen, *rest):
        a = _arr(pSrcA, dt)[:int(srcALen)]
        b = _arr(pSrcB, dt)[:int(srcBLen)]
        s1 = _np.zeros(len(a) + 2 * len(b) + 16, _np.int16)
        s2 = _np.zeros(len(a) + 2 * len(b) + 16, _np.int16)
        f = getattr(_lib, f"arm_{fn}")
        if fn in _abi.CONV_OPT_PARTIAL:
            first, num = int(rest[0]), int(rest[1])
            y = _np.zeros(len(a) + len(b) - 1, dt)
            st = f(a.ctypes.data, len(a), b.ctypes.data, len(b), y.ctypes.data, first, num, s1.ctypes.data,
                   s2.ctypes.data)
            _check(f"arm_{fn}")
            return st, y
        n = 2 * max(len(a), len(b)) - 1 if fn.startswith("correlate") else len(a) + len(b) - 1
        y = _np.zeros(n, dt)
        args = [a.ctypes.data, len(a), b.ctypes.data, len(b), y.ctypes.data, s1.ctypes.data]
        if n_scratch == 2:
            args.append(s2.ctypes.data)
        f(*args)
        _check(f"arm_{fn}")
        return y
    run.__name__ = f"arm_{fn}"
    return run


for _fn in (*_abi.CONV_OPT_FULL, *_abi.CONV_OPT_PARTIAL):
    globals()[f"arm_{_fn}"] = _conv_opt(_fn)
del _fn


# ------------------------------------------------------------------ MFCC
def arm_mfcc_init_f32(inst, fftLen, nbMelFilters, nbDctOutputs, dctCoefs, filterPos, filterLengths,
                      filterCoefs, windowCoefs):
    keep = [_arr(dctCoefs, _np.float32).reshape(-1), _arr(filterPos, _np.uint32), _arr(filterLengths, _np.uint32),
            _arr(filterCoefs, _np.float32), _arr(windowCoefs, _np.float32)]
    inst._keep = keep
    return _lib.arm_mfcc_init_f32(_C.byref(inst._s), int(fftLen), int(nbMelFilters), int(nbDctOutputs),
                                  *[k.ctypes.data for k in keep])


def arm_mfcc_f32(inst, pSrc, pTmp, tmp2=None):
    src = _arr(pSrc, _np.float32).copy()
    out = _np.zeros(inst._s.nbDctOutputs, dtype=_np.float32)
    tmp = _np.zeros(2 * inst._s.fftLen, dtype=_np.float32)
    _lib.arm_mfcc_f32(_C.byref(inst._s), src.ctypes.data, out.ctypes.data, tmp.ctypes.data)
    _check("arm_mfcc_f32")
    return out


def _mfcc_fixed_init(t, dt):
    def init(inst, fftLen, nbMelFilters, nbDctOutputs, dctCoefs, filterPos, filterLengths, filterCoefs, windowCoefs):
        keep = [_arr(dctCoefs, dt).reshape(-1), _arr(filterPos, _np.uint32), _arr(filterLengths, _np.uint32),
                _arr(filterCoefs, dt), _arr(windowCoefs, dt)]
        inst._keep = keep
        return getattr(_lib, f"arm_mfcc_init_{t}")(_C.byref(inst._s), int(fftLen), int(nbMelFilters),
                                                   int(nbDctOutputs), *[k.ctypes.data for k in keep])
    init.__name__ = f"arm_mfcc_init_{t}"
    return init


def _mfcc_fixed(t, dt):
    # cmsisdsp_transform.c:2821-2870 (q15), the q31 analogue: returns (status, pDst)
    def mfcc(inst, pSrc, pTmp, tmp2=None):
        src = _arr(pSrc, dt).copy()
        out = _np.zeros(inst._s.nbDctOutputs, dtype=dt)
        tmp = _np.zeros(2 * inst._s.fftLen, dtype=_np.int32)
        st = getattr(_lib, f"arm_mfcc_{t}")(_C.byref(inst._s), src.ctypes.data, out.ctypes.data, tmp.ctypes.data)
        return st, out
    mfcc.__name__ = f"arm_mfcc_{t}"
    return mfcc


arm_mfcc_init_q31 = _mfcc_fixed_init("q31", _np.int32)
arm_mfcc_init_q15 = _mfcc_fixed_init("q15", _np.int16)
arm_mfcc_q31 = _mfcc_fixed("q31", _np.int32)
arm_mfcc_q15 = _mfcc_fixed("q15", _np.int16)


def arm_mfcc_tmp_buffer_size(dt, fftLen, buf_id, arch=None, use_cfft=0):
    return 2 * int(fftLen) if buf_id == 1 else 0
