"""ctypes mirror of include/arm_math.h (struct layouts + prototypes).

The same declarations bind three libraries with the identical C ABI:
  * libcmsisdsp_mi355x.so  — this backend (the product);
  * oracle/_ref/libcmsisdsp_ref.so — the reference scalar C path (test infrastructure);
  * oracle/_build/liboracle.so — the CPU restatement (test infrastructure, `oracle_` prefix).
"""
import ctypes as C

c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int32)
c_i16p = C.POINTER(C.c_int16)
c_i8p = C.POINTER(C.c_int8)
c_u16p = C.POINTER(C.c_uint16)

ARM_MATH_SUCCESS = 0
ARM_MATH_ARGUMENT_ERROR = -1
ARM_MATH_LENGTH_ERROR = -2
ARM_MATH_SIZE_MISMATCH = -3


def _cfft_struct(name, twp):
    # Include/dsp/transform_functions.h:410-424 (scalar layout)
    return type(name, (C.Structure,), {"_fields_": [
        ("fftLen", C.c_uint16), ("pTwiddle", twp), ("pBitRevTable", c_u16p), ("bitRevLength", C.c_uint16)]})


arm_cfft_instance_f32 = _cfft_struct("arm_cfft_instance_f32", c_f32p)
arm_cfft_instance_q31 = _cfft_struct("arm_cfft_instance_q31", c_i32p)
arm_cfft_instance_q15 = _cfft_struct("arm_cfft_instance_q15", c_i16p)


class arm_rfft_fast_instance_f32(C.Structure):
    # Include/dsp/transform_functions.h:813-818
    _fields_ = [("Sint", arm_cfft_instance_f32), ("fftLenRFFT", C.c_uint16), ("pTwiddleRFFT", c_f32p)]


def _rfft_fixed_struct(name, twp, cfft):
    # Include/dsp/transform_functions.h:636-649 (q31), :508-521 (q15): non-Neon, non-MVE layout
    return type(name, (C.Structure,), {"_fields_": [
        ("fftLenReal", C.c_uint32), ("ifftFlagR", C.c_uint8), ("bitReverseFlagR", C.c_uint8),
        ("twidCoefRModifier", C.c_uint32), ("pTwiddleAReal", twp), ("pTwiddleBReal", twp),
        ("pCfft", C.POINTER(cfft))]})


arm_rfft_instance_q31 = _rfft_fixed_struct("arm_rfft_instance_q31", c_i32p, arm_cfft_instance_q31)
arm_rfft_instance_q15 = _rfft_fixed_struct("arm_rfft_instance_q15", c_i16p, arm_cfft_instance_q15)


class arm_fir_instance_f32(C.Structure):
    # Include/dsp/filtering_functions.h:86-91
    _fields_ = [("numTaps", C.c_uint16), ("pState", c_f32p), ("pCoeffs", c_f32p)]


class arm_fir_instance_q7(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p)]


# arm_fir_decimate_instance_{f32,q15,q31} / arm_fir_interpolate_instance_{f32,q15,q31}: one
# layout per family (the element type only changes the pointees)
class arm_fir_decimate_instance(C.Structure):
    _fields_ = [("M", C.c_uint8), ("numTaps", C.c_uint16), ("pCoeffs", C.c_void_p), ("pState", C.c_void_p)]


class arm_fir_interpolate_instance(C.Structure):
    _fields_ = [("L", C.c_uint8), ("phaseLength", C.c_uint16), ("pCoeffs", C.c_void_p), ("pState", C.c_void_p)]


# arm_fir_lattice_instance_{f32,q31,q15} (filtering_functions.h:1312-1340), one layout
class arm_fir_lattice_instance(C.Structure):
    _fields_ = [("numStages", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p)]


# Biquad cascade instances (filtering_functions.h:285-312, :1148-1203)
class arm_biquad_casd_df1_inst_q15(C.Structure):
    _fields_ = [("numStages", C.c_int8), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("postShift", C.c_int8)]


class arm_biquad_casd_df1_inst_q31(C.Structure):
    _fields_ = [("numStages", C.c_uint32), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("postShift", C.c_uint8)]


class arm_biquad_casd_df1_inst_f32(C.Structure):
    _fields_ = [("numStages", C.c_uint32), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p)]


class arm_biquad_cas_df1_32x64_ins_q31(C.Structure):
    _fields_ = [("numStages", C.c_uint8), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("postShift", C.c_uint8)]


class arm_biquad_cascade_df2T_instance_f32(C.Structure):
    _fields_ = [("numStages", C.c_uint8), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p)]


class arm_biquad_cascade_stereo_df2T_instance_f32(C.Structure):
    _fields_ = [("numStages", C.c_uint8), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p)]


# IIR lattice instances (filtering_functions.h:1428-1458): one layout, a class per type
class arm_iir_lattice_instance_f32(C.Structure):
    _fields_ = [("numStages", C.c_uint16), ("pState", C.c_void_p), ("pkCoeffs", C.c_void_p), ("pvCoeffs", C.c_void_p)]


class arm_iir_lattice_instance_q31(C.Structure):
    _fields_ = arm_iir_lattice_instance_f32._fields_


class arm_iir_lattice_instance_q15(C.Structure):
    _fields_ = arm_iir_lattice_instance_f32._fields_


# LMS / normalised LMS instances (filtering_functions.h:1560-1566, :1608-1615, :1659-1666, :1710-1718, :1813-1824)
class arm_lms_instance_f32(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("mu", C.c_float)]


class arm_lms_instance_q31(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("mu", C.c_int32),
                ("postShift", C.c_uint32)]


class arm_lms_instance_q15(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("mu", C.c_int16),
                ("postShift", C.c_uint32)]


class arm_lms_norm_instance_f32(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("mu", C.c_float),
                ("energy", C.c_float), ("x0", C.c_float)]


class arm_lms_norm_instance_q15(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p), ("mu", C.c_int16),
                ("postShift", C.c_uint8), ("recipTable", C.c_void_p), ("energy", C.c_int16), ("x0", C.c_int16)]


# arm_fir_sparse_instance_{f32,q31,q15,q7} (filtering_functions.h:2033-2091), one layout
class arm_fir_sparse_instance(C.Structure):
    _fields_ = [("numTaps", C.c_uint16), ("stateIndex", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p),
                ("maxDelay", C.c_uint16), ("pTapDelay", C.c_void_p)]


class arm_fir_instance_q15(C.Structure):
    # Include/dsp/filtering_functions.h:66-71
    _fields_ = [("numTaps", C.c_uint16), ("pState", c_i16p), ("pCoeffs", c_i16p)]


class arm_fir_instance_q31(C.Structure):
    # Include/dsp/filtering_functions.h:76-81
    _fields_ = [("numTaps", C.c_uint16), ("pState", c_i32p), ("pCoeffs", c_i32p)]


class arm_matrix_instance_f32(C.Structure):
    # Include/dsp/matrix_functions.h:118-123
    _fields_ = [("numRows", C.c_uint16), ("numCols", C.c_uint16), ("pData", c_f32p)]


class arm_mfcc_instance_f32(C.Structure):
    # Include/dsp/transform_functions.h:856-873 (RFFT-based default build)
    _fields_ = [("dctCoefs", c_f32p), ("filterCoefs", c_f32p), ("windowCoefs", c_f32p),
                ("filterPos", C.POINTER(C.c_uint32)), ("filterLengths", C.POINTER(C.c_uint32)),
                ("fftLen", C.c_uint32), ("nbMelFilters", C.c_uint32), ("nbDctOutputs", C.c_uint32),
                ("rfft", arm_rfft_fast_instance_f32)]


class arm_mfcc_instance_q31(C.Structure):
    # Include/dsp/transform_functions.h:1000-1020 (RFFT-based default build)
    _fields_ = [("dctCoefs", c_i32p), ("filterCoefs", c_i32p), ("windowCoefs", c_i32p),
                ("filterPos", C.POINTER(C.c_uint32)), ("filterLengths", C.POINTER(C.c_uint32)),
                ("fftLen", C.c_uint32), ("nbMelFilters", C.c_uint32), ("nbDctOutputs", C.c_uint32),
                ("rfft", arm_rfft_instance_q31)]


class arm_mfcc_instance_q15(C.Structure):
    # Include/dsp/transform_functions.h:1150-1168 (RFFT-based default build)
    _fields_ = [("dctCoefs", c_i16p), ("filterCoefs", c_i16p), ("windowCoefs", c_i16p),
                ("filterPos", C.POINTER(C.c_uint32)), ("filterLengths", C.POINTER(C.c_uint32)),
                ("fftLen", C.c_uint32), ("nbMelFilters", C.c_uint32), ("nbDctOutputs", C.c_uint32),
                ("rfft", arm_rfft_instance_q15)]


class arm_matrix_instance_q7(C.Structure):
    # Include/dsp/matrix_functions.h:139-143
    _fields_ = [("numRows", C.c_uint16), ("numCols", C.c_uint16), ("pData", c_i8p)]


class arm_matrix_instance_q15(C.Structure):
    # Include/dsp/matrix_functions.h:139-144
    _fields_ = [("numRows", C.c_uint16), ("numCols", C.c_uint16), ("pData", c_i16p)]


class arm_matrix_instance_q31(C.Structure):
    # Include/dsp/matrix_functions.h:149-154
    _fields_ = [("numRows", C.c_uint16), ("numCols", C.c_uint16), ("pData", c_i32p)]


P = C.POINTER
SIZES = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
RFFT_SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
# convolution / correlation family (drop-in names without the arm_ prefix)
CONV_FULL = ("conv_f32", "conv_q15", "conv_q31", "conv_fast_q15", "conv_fast_q31", "correlate_f32", "correlate_q15",
             "correlate_q31", "correlate_fast_q15", "correlate_fast_q31", "conv_q7", "correlate_q7")
CONV_PARTIAL = ("conv_partial_f32", "conv_partial_q15", "conv_partial_q31", "conv_partial_q7")
# product only (the oracle restates them as arm_conv_fast_* over the range; the reference's
# own bodies are memory-unsafe for most ranges)
CONV_PARTIAL_FAST = ("conv_partial_fast_q15", "conv_partial_fast_q31")
# scratch-buffer forms: name -> number of trailing scratch pointers
CONV_OPT_FULL = {"conv_opt_q15": 2, "conv_fast_opt_q15": 2, "conv_opt_q7": 2, "correlate_opt_q15": 1,
                 "correlate_fast_opt_q15": 1, "correlate_opt_q7": 2}
CONV_OPT_PARTIAL = ("conv_partial_opt_q15", "conv_partial_fast_opt_q15", "conv_partial_opt_q7")

# name -> (restype, argtypes): the drop-in surface of include/arm_math.h
DROPIN = {
    "arm_cfft_init_f32": (C.c_int, [P(arm_cfft_instance_f32), C.c_uint16]),
    "arm_cfft_init_q31": (C.c_int, [P(arm_cfft_instance_q31), C.c_uint16]),
    "arm_cfft_init_q15": (C.c_int, [P(arm_cfft_instance_q15), C.c_uint16]),
    "arm_cfft_f32": (None, [P(arm_cfft_instance_f32), C.c_void_p, C.c_uint8, C.c_uint8]),
    "arm_cfft_q31": (None, [P(arm_cfft_instance_q31), C.c_void_p, C.c_uint8, C.c_uint8]),
    "arm_cfft_q15": (None, [P(arm_cfft_instance_q15), C.c_void_p, C.c_uint8, C.c_uint8]),
    "arm_rfft_fast_init_f32": (C.c_int, [P(arm_rfft_fast_instance_f32), C.c_uint16]),
    "arm_rfft_fast_f32": (None, [P(arm_rfft_fast_instance_f32), C.c_void_p, C.c_void_p, C.c_uint8]),
    "arm_rfft_init_q31": (C.c_int, [P(arm_rfft_instance_q31), C.c_uint32, C.c_uint32, C.c_uint32]),
    "arm_rfft_init_q15": (C.c_int, [P(arm_rfft_instance_q15), C.c_uint32, C.c_uint32, C.c_uint32]),
    "arm_rfft_q31": (None, [P(arm_rfft_instance_q31), C.c_void_p, C.c_void_p]),
    "arm_rfft_q15": (None, [P(arm_rfft_instance_q15), C.c_void_p, C.c_void_p]),
    "arm_fir_init_f32": (None, [P(arm_fir_instance_f32), C.c_uint16, C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_f32": (None, [P(arm_fir_instance_f32), C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_init_q15": (C.c_int, [P(arm_fir_instance_q15), C.c_uint16, C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_q15": (None, [P(arm_fir_instance_q15), C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_fast_q15": (None, [P(arm_fir_instance_q15), C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_init_q31": (None, [P(arm_fir_instance_q31), C.c_uint16, C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_q31": (None, [P(arm_fir_instance_q31), C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_fast_q31": (None, [P(arm_fir_instance_q31), C.c_void_p, C.c_void_p, C.c_uint32]),
    "arm_fir_init_q7": (None, [P(arm_fir_instance_q7), C.c_uint16, C.c_void_p, C.c_void_p, C.c_uint32]),
    **{f"arm_fir_decimate_init_{t}": (C.c_int, [P(arm_fir_decimate_instance), C.c_uint16, C.c_uint8, C.c_void_p,
                                                C.c_void_p, C.c_uint32]) for t in ("f32", "q15", "q31")},
    **{f"arm_fir_interpolate_init_{t}": (C.c_int, [P(arm_fir_interpolate_instance), C.c_uint8, C.c_uint16,
                                                   C.c_void_p, C.c_void_p, C.c_uint32]) for t in ("f32", "q15", "q31")},
    **{f"arm_fir_{k}": (None, [P(arm_fir_decimate_instance), C.c_void_p, C.c_void_p, C.c_uint32])
       for k in ("decimate_f32", "decimate_q15", "decimate_fast_q15", "decimate_q31", "decimate_fast_q31")},
    **{f"arm_fir_{k}": (None, [P(arm_fir_interpolate_instance), C.c_void_p, C.c_void_p, C.c_uint32])
       for k in ("interpolate_f32", "interpolate_q15", "interpolate_q31")},
    "arm_fir_q7": (None, [P(arm_fir_instance_q7), C.c_void_p, C.c_void_p, C.c_uint32]),
    **{f"arm_{k}": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_void_p] * n)
       for k, n in CONV_OPT_FULL.items()},
    **{f"arm_{k}": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                              C.c_void_p, C.c_void_p]) for k in CONV_OPT_PARTIAL},
    **{f"arm_fir_lattice_init_{t}": (None, [P(arm_fir_lattice_instance), C.c_uint16, C.c_void_p, C.c_void_p])
       for t in ("f32", "q31", "q15")},
    **{f"arm_fir_lattice_{t}": (None, [P(arm_fir_lattice_instance), C.c_void_p, C.c_void_p, C.c_uint32])
       for t in ("f32", "q31", "q15")},
    **{f"arm_fir_sparse_init_{t}": (None, [P(arm_fir_sparse_instance), C.c_uint16, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint16, C.c_uint32]) for t in ("f32", "q31", "q15", "q7")},
    **{f"arm_fir_sparse_{t}": (None, [P(arm_fir_sparse_instance), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32])
       for t in ("f32", "q31")},
    **{f"arm_fir_sparse_{t}": (None, [P(arm_fir_sparse_instance), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32]) for t in ("q15", "q7")},
    "arm_mat_init_f32": (None, [P(arm_matrix_instance_f32), C.c_uint16, C.c_uint16, C.c_void_p]),
    "arm_mat_init_q7": (None, [P(arm_matrix_instance_q7), C.c_uint16, C.c_uint16, C.c_void_p]),
    "arm_mat_init_q15": (None, [P(arm_matrix_instance_q15), C.c_uint16, C.c_uint16, C.c_void_p]),
    "arm_mat_mult_q7": (C.c_int, [P(arm_matrix_instance_q7), P(arm_matrix_instance_q7),
                                  P(arm_matrix_instance_q7), C.c_void_p]),
    "arm_mat_init_q31": (None, [P(arm_matrix_instance_q31), C.c_uint16, C.c_uint16, C.c_void_p]),
    "arm_mat_mult_q15": (C.c_int, [P(arm_matrix_instance_q15), P(arm_matrix_instance_q15),
                                   P(arm_matrix_instance_q15), C.c_void_p]),
    "arm_mat_mult_q31": (C.c_int, [P(arm_matrix_instance_q31), P(arm_matrix_instance_q31),
                                   P(arm_matrix_instance_q31)]),
    "arm_mat_mult_opt_q31": (C.c_int, [P(arm_matrix_instance_q31), P(arm_matrix_instance_q31),
                                       P(arm_matrix_instance_q31), C.c_void_p]),
    "arm_mat_mult_fast_q15": (C.c_int, [P(arm_matrix_instance_q15), P(arm_matrix_instance_q15),
                                        P(arm_matrix_instance_q15), C.c_void_p]),
    "arm_mat_mult_fast_q31": (C.c_int, [P(arm_matrix_instance_q31), P(arm_matrix_instance_q31),
                                        P(arm_matrix_instance_q31)]),
    "arm_conv_f32": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "arm_conv_q15": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "arm_conv_q31": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    **{f"arm_{f}": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])
       for f in CONV_FULL if f not in ("conv_f32", "conv_q15", "conv_q31")},
    **{f"arm_{f}": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32])
       for f in CONV_PARTIAL},
    "arm_mfcc_init_f32": (C.c_int, [P(arm_mfcc_instance_f32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "arm_mfcc_f32": (None, [P(arm_mfcc_instance_f32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "arm_mfcc_init_q31": (C.c_int, [P(arm_mfcc_instance_q31), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "arm_mfcc_q31": (C.c_int, [P(arm_mfcc_instance_q31), C.c_void_p, C.c_void_p, C.c_void_p]),
    "arm_mfcc_init_q15": (C.c_int, [P(arm_mfcc_instance_q15), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "arm_mfcc_q15": (C.c_int, [P(arm_mfcc_instance_q15), C.c_void_p, C.c_void_p, C.c_void_p]),
    "arm_mat_mult_f32": (C.c_int, [P(arm_matrix_instance_f32), P(arm_matrix_instance_f32),
                                   P(arm_matrix_instance_f32)]),
}
for _t in ("f32", "q31", "q15"):
    _inst = {"f32": arm_cfft_instance_f32, "q31": arm_cfft_instance_q31, "q15": arm_cfft_instance_q15}[_t]
    for _n in SIZES:
        DROPIN[f"arm_cfft_init_{_n}_{_t}"] = (C.c_int, [P(_inst)])
for _n in RFFT_SIZES:
    DROPIN[f"arm_rfft_fast_init_{_n}_f32"] = (C.c_int, [P(arm_rfft_fast_instance_f32)])

# Biquad cascades: processing function -> (instance, init function, init takes postShift).  The product
# only: neither CPU checker builds them (tests/golden/biquad.npz holds the reference's outputs).
BIQUAD_FUNCS = {
    "arm_biquad_cascade_df1_f32": (arm_biquad_casd_df1_inst_f32, "arm_biquad_cascade_df1_init_f32", None),
    "arm_biquad_cascade_df1_q31": (arm_biquad_casd_df1_inst_q31, "arm_biquad_cascade_df1_init_q31", C.c_int8),
    "arm_biquad_cascade_df1_fast_q31": (arm_biquad_casd_df1_inst_q31, "arm_biquad_cascade_df1_init_q31", C.c_int8),
    "arm_biquad_cascade_df1_q15": (arm_biquad_casd_df1_inst_q15, "arm_biquad_cascade_df1_init_q15", C.c_int8),
    "arm_biquad_cascade_df1_fast_q15": (arm_biquad_casd_df1_inst_q15, "arm_biquad_cascade_df1_init_q15", C.c_int8),
    "arm_biquad_cas_df1_32x64_q31": (arm_biquad_cas_df1_32x64_ins_q31, "arm_biquad_cas_df1_32x64_init_q31", C.c_uint8),
    "arm_biquad_cascade_df2T_f32": (arm_biquad_cascade_df2T_instance_f32, "arm_biquad_cascade_df2T_init_f32", None),
    "arm_biquad_cascade_stereo_df2T_f32": (arm_biquad_cascade_stereo_df2T_instance_f32,
                                           "arm_biquad_cascade_stereo_df2T_init_f32", None),
}
BIQUAD = {}
for _f, (_inst, _init, _ps) in BIQUAD_FUNCS.items():
    BIQUAD[_f] = (None, [P(_inst), C.c_void_p, C.c_void_p, C.c_uint32])
    BIQUAD[_init] = (None, [P(_inst), C.c_uint8, C.c_void_p, C.c_void_p] + ([_ps] if _ps else []))

# IIR lattice and LMS / normalised LMS: processing function -> (instance, init function, the init's
# arguments after (S, n, coefficient pointers, pState): mu and postShift).  The product only, as BIQUAD
# (tests/golden/adaptive.npz holds the reference's outputs).
ADAPTIVE_FUNCS = {
    "arm_iir_lattice_f32": (arm_iir_lattice_instance_f32, "arm_iir_lattice_init_f32", []),
    "arm_iir_lattice_q31": (arm_iir_lattice_instance_q31, "arm_iir_lattice_init_q31", []),
    "arm_iir_lattice_q15": (arm_iir_lattice_instance_q15, "arm_iir_lattice_init_q15", []),
    "arm_lms_f32": (arm_lms_instance_f32, "arm_lms_init_f32", [C.c_float]),
    "arm_lms_q31": (arm_lms_instance_q31, "arm_lms_init_q31", [C.c_int32, C.c_uint32]),
    "arm_lms_q15": (arm_lms_instance_q15, "arm_lms_init_q15", [C.c_int16, C.c_uint32]),
    "arm_lms_norm_f32": (arm_lms_norm_instance_f32, "arm_lms_norm_init_f32", [C.c_float]),
    "arm_lms_norm_q15": (arm_lms_norm_instance_q15, "arm_lms_norm_init_q15", [C.c_int16, C.c_uint8]),
}
ADAPTIVE = {}
for _f, (_inst, _init, _extra) in ADAPTIVE_FUNCS.items():
    if "lattice" in _f:   # (S, pSrc, pDst, blockSize); init (S, numStages, pkCoeffs, pvCoeffs, pState, blockSize)
        ADAPTIVE[_f] = (None, [P(_inst), C.c_void_p, C.c_void_p, C.c_uint32])
        ADAPTIVE[_init] = (None, [P(_inst), C.c_uint16, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32])
    else:                 # (S, pSrc, pRef, pOut, pErr, blockSize); init (S, numTaps, pCoeffs, pState, mu, blockSize[, postShift])
        ADAPTIVE[_f] = (None, [P(_inst), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32])
        ADAPTIVE[_init] = (None, [P(_inst), C.c_uint16, C.c_void_p, C.c_void_p, _extra[0], C.c_uint32] + _extra[1:])

# Complex matrix multiply: the drop-ins (q15 takes pScratch), the batched and the multi-shard forms.  The
# product only, as BIQUAD (tests/golden/cmplx_mat.npz holds the reference's outputs).
CMPLX_MAT_INST = {"f32": arm_matrix_instance_f32, "q31": arm_matrix_instance_q31, "q15": arm_matrix_instance_q15}
CMPLX_MAT = {}
for _t, _inst in CMPLX_MAT_INST.items():
    CMPLX_MAT[f"arm_mat_cmplx_mult_{_t}"] = (C.c_int, [P(_inst)] * 3 + ([C.c_void_p] if _t == "q15" else []))
    CMPLX_MAT[f"arm_mat_cmplx_mult_{_t}_batch"] = (C.c_int, [P(_inst)] * 3 + [C.c_uint32, C.c_void_p])
    CMPLX_MAT[f"arm_mat_cmplx_mult_{_t}_batch_multi"] = (C.c_int, [P(_inst)] * 3 + [C.c_uint32] + [C.c_void_p] * 5)

# Inverse, Cholesky, LDLT and triangular solves: the drop-ins and the batched forms (d_status / d_pp are device
# pointers).  The product only, as CMPLX_MAT (tests/golden/mat_solve.npz holds the reference's outputs).
_MF = P(arm_matrix_instance_f32)
MAT_SOLVE = {
    "arm_mat_inverse_f32": (C.c_int, [_MF, _MF]),
    "arm_mat_cholesky_f32": (C.c_int, [_MF, _MF]),
    "arm_mat_ldlt_f32": (C.c_int, [_MF, _MF, _MF, C.c_void_p]),
    "arm_mat_solve_lower_triangular_f32": (C.c_int, [_MF, _MF, _MF]),
    "arm_mat_solve_upper_triangular_f32": (C.c_int, [_MF, _MF, _MF]),
    "arm_mat_inverse_f32_batch": (C.c_int, [_MF, _MF, C.c_uint32, C.c_void_p, C.c_void_p]),
    "arm_mat_cholesky_f32_batch": (C.c_int, [_MF, _MF, C.c_uint32, C.c_void_p, C.c_void_p]),
    "arm_mat_ldlt_f32_batch": (C.c_int, [_MF, _MF, _MF, C.c_void_p, C.c_uint32, C.c_void_p]),
    "arm_mat_solve_lower_triangular_f32_batch": (C.c_int, [_MF, _MF, _MF, C.c_uint32, C.c_void_p, C.c_void_p]),
    "arm_mat_solve_upper_triangular_f32_batch": (C.c_int, [_MF, _MF, _MF, C.c_uint32, C.c_void_p, C.c_void_p]),
}

# Element-wise add / sub / scale, the transposes and matrix x vector: 20 drop-ins and their _batch forms.  The
# product only (tests/golden/mat_basic.npz holds the reference's outputs).
MAT_INST = {"f32": arm_matrix_instance_f32, "q31": arm_matrix_instance_q31, "q15": arm_matrix_instance_q15,
            "q7": arm_matrix_instance_q7}
MAT_PTR = {"f32": c_f32p, "q31": c_i32p, "q15": c_i16p, "q7": c_i8p}
MAT_SCALAR = {"f32": C.c_float, "q31": C.c_int32, "q15": C.c_int16}
MAT_BASIC = {}
for _t, _inst in MAT_INST.items():
    _pm, _tail = P(_inst), [C.c_uint32, C.c_void_p]
    if _t != "q7":
        _sc = [_pm, MAT_SCALAR[_t]] + ([C.c_int32] if _t != "f32" else []) + [_pm]
        for _n, _a in (("add", [_pm] * 3), ("sub", [_pm] * 3), ("scale", _sc), ("cmplx_trans", [_pm] * 2)):
            MAT_BASIC[f"arm_mat_{_n}_{_t}"] = (C.c_int, _a)
            MAT_BASIC[f"arm_mat_{_n}_{_t}_batch"] = (C.c_int, _a + _tail)
    MAT_BASIC[f"arm_mat_trans_{_t}"] = (C.c_int, [_pm] * 2)
    MAT_BASIC[f"arm_mat_trans_{_t}_batch"] = (C.c_int, [_pm] * 2 + _tail)
    MAT_BASIC[f"arm_mat_vec_mult_{_t}"] = (None, [_pm, C.c_void_p, C.c_void_p])
    MAT_BASIC[f"arm_mat_vec_mult_{_t}_batch"] = (C.c_int, [_pm, C.c_uint32, C.c_void_p, C.c_void_p] + _tail)

# Complex math and max / min: 26 drop-ins (the reference's signatures, all void) and their _batch forms.  The
# product only (tests/golden/cmplx_math.npz holds the reference's outputs).  Every pointer is a void*.
CMPLX_MATH = {}
_vp, _u32 = C.c_void_p, C.c_uint32
for _t in ("f32", "q31", "q15"):
    for _n, _a, _b in (("mag", [_vp, _vp, _u32], None), ("mag_squared", [_vp, _vp, _u32], None),
                       ("conj", [_vp, _vp, _u32], None), ("mult_cmplx", [_vp, _vp, _vp, _u32], None),
                       ("mult_real", [_vp, _vp, _vp, _u32], None),
                       ("dot_prod", [_vp, _vp, _u32, _vp, _vp], [_vp, _vp, _u32, _u32, _vp, _vp])):
        CMPLX_MATH[f"arm_cmplx_{_n}_{_t}"] = (None, _a)
        CMPLX_MATH[f"arm_cmplx_{_n}_{_t}_batch"] = (C.c_int, (_b or _a) + [_u32, _vp])
for _t in ("f32", "q31", "q15", "q7"):
    for _n in ("max", "min"):
        CMPLX_MATH[f"arm_{_n}_{_t}"] = (None, [_vp, _u32, _vp, _vp])
        CMPLX_MATH[f"arm_{_n}_{_t}_batch"] = (C.c_int, [_vp, _u32, _vp, _vp, _u32, _vp])

# Statistics: 46 drop-ins (the reference's signatures, all void), arm_cmplx_mag_fast_q15 and their _batch forms, and
# the scalar arm_sqrt_q15.  The product only (tests/golden/statistics.npz holds the reference's outputs).
STATISTICS = {}
STAT_TYPES = ("f32", "q31", "q15", "q7")
for _t in STAT_TYPES:
    _one = [("mean", 0), ("power", 0), ("max_no_idx", 0), ("min_no_idx", 0), ("absmax_no_idx", 0),
            ("absmin_no_idx", 0), ("absmax", 1), ("absmin", 1), ("mse", 2)]
    if _t != "q7":
        _one += [("rms", 0), ("var", 0), ("std", 0)]
    if _t == "f32":
        _one += [("accumulate", 0)]
    for _n, _k in _one:
        _a = ([_vp, _u32, _vp], [_vp, _u32, _vp, _vp], [_vp, _vp, _u32, _vp])[_k]
        STATISTICS[f"arm_{_n}_{_t}"] = (None, _a)
        STATISTICS[f"arm_{_n}_{_t}_batch"] = (C.c_int, _a + [_u32, _vp])
STATISTICS["arm_cmplx_mag_fast_q15"] = (None, [_vp, _vp, _u32])
STATISTICS["arm_cmplx_mag_fast_q15_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp])
STATISTICS["arm_sqrt_q15"] = (C.c_int, [C.c_int16, _vp])

# Basic math: 51 drop-ins (the reference's signatures, all void) and their _batch forms.  The product only
# (tests/golden/basic_math.npz holds the reference's outputs).  Scalars have the element's C type; shifts are int8_t.
BASIC_MATH = {}
BASIC_TYPES = ("f32", "q31", "q15", "q7")
BITWISE_TYPES = ("u32", "u16", "u8")
BASIC_SCALAR = {"f32": C.c_float, "q31": C.c_int32, "q15": C.c_int16, "q7": C.c_int8}
for _t in BASIC_TYPES:
    _s = BASIC_SCALAR[_t]
    _ops = [("add", [_vp, _vp, _vp, _u32]), ("sub", [_vp, _vp, _vp, _u32]), ("mult", [_vp, _vp, _vp, _u32]),
            ("offset", [_vp, _s, _vp, _u32]), ("clip", [_vp, _vp, _s, _s, _u32]), ("abs", [_vp, _vp, _u32]),
            ("negate", [_vp, _vp, _u32]),
            ("scale", [_vp, _s, _vp, _u32] if _t == "f32" else [_vp, _s, C.c_int8, _vp, _u32])]
    if _t != "f32":
        _ops += [("shift", [_vp, C.c_int8, _vp, _u32])]
    for _n, _a in _ops:
        BASIC_MATH[f"arm_{_n}_{_t}"] = (None, _a)
        BASIC_MATH[f"arm_{_n}_{_t}_batch"] = (C.c_int, _a + [_u32, _vp])
    BASIC_MATH[f"arm_dot_prod_{_t}"] = (None, [_vp, _vp, _u32, _vp])
    BASIC_MATH[f"arm_dot_prod_{_t}_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp])
for _t in BITWISE_TYPES:
    for _n, _a in (("and", [_vp, _vp, _vp, _u32]), ("or", [_vp, _vp, _vp, _u32]), ("xor", [_vp, _vp, _vp, _u32]),
                   ("not", [_vp, _vp, _u32])):
        BASIC_MATH[f"arm_{_n}_{_t}"] = (None, _a)
        BASIC_MATH[f"arm_{_n}_{_t}_batch"] = (C.c_int, _a + [_u32, _vp])

# Support functions: 24 drop-ins with their _batch forms and the two sort inits.  The product only
# (tests/golden/support.npz holds the reference's outputs).  arm_sort_alg / arm_sort_dir are C enums (int).
class arm_sort_instance_f32(C.Structure):
    _fields_ = [("alg", C.c_int), ("dir", C.c_int)]


class arm_merge_sort_instance_f32(C.Structure):
    _fields_ = [("dir", C.c_int), ("buffer", C.c_void_p)]


SUPPORT = {}
SUPPORT_NAMES = {"f32": "float", "q31": "q31", "q15": "q15", "q7": "q7"}      # the type's name in arm_<a>_to_<b>
for _s in BASIC_TYPES:
    for _d in BASIC_TYPES:
        if _s != _d:
            _n = f"arm_{SUPPORT_NAMES[_s]}_to_{SUPPORT_NAMES[_d]}"
            SUPPORT[_n] = (None, [_vp, _vp, _u32])
            SUPPORT[_n + "_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp])
    SUPPORT[f"arm_copy_{_s}"] = (None, [_vp, _vp, _u32])
    SUPPORT[f"arm_copy_{_s}_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp])
    SUPPORT[f"arm_fill_{_s}"] = (None, [BASIC_SCALAR[_s], _vp, _u32])
    SUPPORT[f"arm_fill_{_s}_batch"] = (C.c_int, [BASIC_SCALAR[_s], _vp, _u32, _u32, _vp])
SUPPORT["arm_sort_init_f32"] = (None, [P(arm_sort_instance_f32), C.c_int, C.c_int])
SUPPORT["arm_sort_f32"] = (None, [P(arm_sort_instance_f32), _vp, _vp, _u32])
SUPPORT["arm_merge_sort_init_f32"] = (None, [P(arm_merge_sort_instance_f32), C.c_int, _vp])
SUPPORT["arm_merge_sort_f32"] = (None, [P(arm_merge_sort_instance_f32), _vp, _vp, _u32])
SUPPORT["arm_sort_f32_batch"] = (C.c_int, [_vp, _vp, _u32, C.c_int, _u32, _vp])
SUPPORT["arm_merge_sort_f32_batch"] = (C.c_int, [_vp, _vp, _u32, C.c_int, _u32, _vp])
SUPPORT["arm_weighted_average_f32"] = (C.c_float, [_vp, _vp, _u32])
SUPPORT["arm_weighted_average_f32_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp])
SUPPORT["arm_barycenter_f32"] = (None, [_vp, _vp, _vp, _u32, _u32])
SUPPORT["arm_barycenter_f32_batch"] = (C.c_int, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp])

# Distance functions: 20 drop-ins (the reference's signatures) with their _batch forms.  The product only
# (tests/golden/distance.npz holds the reference's outputs).  arm_dtw_window is a C enum (int).
DISTANCE = {}
DISTANCE_F32 = ("braycurtis", "canberra", "chebyshev", "cityblock", "correlation", "cosine", "euclidean",
                "jensenshannon")
DISTANCE_BOOL = ("dice", "hamming", "jaccard", "kulsinski", "rogerstanimoto", "russellrao", "sokalmichener",
                 "sokalsneath", "yule")
for _n in DISTANCE_F32:
    DISTANCE[f"arm_{_n}_distance_f32"] = (C.c_float, [_vp, _vp, _u32])
    DISTANCE[f"arm_{_n}_distance_f32_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp])
for _n in DISTANCE_BOOL:
    DISTANCE[f"arm_{_n}_distance"] = (C.c_float, [_vp, _vp, _u32])
    DISTANCE[f"arm_{_n}_distance_batch"] = (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp])
DISTANCE["arm_dtw_init_window_q7"] = (C.c_int, [C.c_int, C.c_int32, P(arm_matrix_instance_q7)])
DISTANCE["arm_dtw_init_window_q7_batch"] = (C.c_int, [C.c_int, C.c_int32, _vp, _u32, _u32, _u32, _vp])
DISTANCE["arm_dtw_distance_f32"] = (C.c_int, [P(arm_matrix_instance_f32), P(arm_matrix_instance_q7),
                                              P(arm_matrix_instance_f32), _vp])
DISTANCE["arm_dtw_distance_f32_batch"] = (C.c_int, [_vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _u32, _vp])
DISTANCE["arm_dtw_path_f32"] = (None, [P(arm_matrix_instance_f32), _vp, _vp])
DISTANCE["arm_dtw_path_f32_batch"] = (C.c_int, [_vp, _u32, _u32, _vp, _vp, _u32, _vp])

# vexp / vlog, the log-domain statistics, the SVMs and naive Bayes: 10 drop-ins with their _batch forms and the three
# SVM inits.  The product only (tests/golden/ml.npz holds the reference's outputs).
class arm_svm_linear_instance_f32(C.Structure):
    # Include/dsp/svm_functions.h:80-88
    _fields_ = [("nbOfSupportVectors", C.c_uint32), ("vectorDimension", C.c_uint32), ("intercept", C.c_float),
                ("dualCoefficients", C.c_void_p), ("supportVectors", C.c_void_p), ("classes", C.c_void_p)]


class arm_svm_polynomial_instance_f32(C.Structure):
    # Include/dsp/svm_functions.h:94-105
    _fields_ = arm_svm_linear_instance_f32._fields_ + [("degree", C.c_int32), ("coef0", C.c_float),
                                                       ("gamma", C.c_float)]


class arm_svm_rbf_instance_f32(C.Structure):
    # Include/dsp/svm_functions.h:111-120
    _fields_ = arm_svm_linear_instance_f32._fields_ + [("gamma", C.c_float)]


class arm_svm_sigmoid_instance_f32(C.Structure):
    # Include/dsp/svm_functions.h:126-136 (the type only: arm_svm_sigmoid_* are left out)
    _fields_ = arm_svm_linear_instance_f32._fields_ + [("coef0", C.c_float), ("gamma", C.c_float)]


class arm_gaussian_naive_bayes_instance_f32(C.Structure):
    # Include/dsp/bayes_functions.h:57-65
    _fields_ = [("vectorDimension", C.c_uint32), ("numberOfClasses", C.c_uint32), ("theta", C.c_void_p),
                ("sigma", C.c_void_p), ("classPriors", C.c_void_p), ("epsilon", C.c_float)]


SVM_KINDS = {"linear": (arm_svm_linear_instance_f32, []),
             "polynomial": (arm_svm_polynomial_instance_f32, [C.c_int32, C.c_float, C.c_float]),
             "rbf": (arm_svm_rbf_instance_f32, [C.c_float])}
ML = {
    "arm_vexp_f32": (None, [_vp, _vp, _u32]),
    "arm_vlog_f32": (None, [_vp, _vp, _u32]),
    "arm_vexp_f32_batch": (C.c_int, [_vp, _vp, _u32, _u32, _vp]),
    "arm_vlog_f32_batch": (C.c_int, [_vp, _vp, _u32, _u32, _vp]),
    "arm_entropy_f32": (C.c_float, [_vp, _u32]),
    "arm_logsumexp_f32": (C.c_float, [_vp, _u32]),
    "arm_kullback_leibler_f32": (C.c_float, [_vp, _vp, _u32]),
    "arm_logsumexp_dot_prod_f32": (C.c_float, [_vp, _vp, _u32, _vp]),
    "arm_entropy_f32_batch": (C.c_int, [_vp, _u32, _vp, _u32, _vp]),
    "arm_logsumexp_f32_batch": (C.c_int, [_vp, _u32, _vp, _u32, _vp]),
    "arm_kullback_leibler_f32_batch": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp]),
    "arm_logsumexp_dot_prod_f32_batch": (C.c_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp]),
    "arm_gaussian_naive_bayes_predict_f32": (C.c_uint32, [P(arm_gaussian_naive_bayes_instance_f32), _vp, _vp, _vp]),
    "arm_gaussian_naive_bayes_predict_f32_batch": (C.c_int, [P(arm_gaussian_naive_bayes_instance_f32), _vp, _vp, _vp,
                                                             _u32, _vp]),
}
for _k, (_inst, _extra) in SVM_KINDS.items():
    ML[f"arm_svm_{_k}_init_f32"] = (None, [P(_inst), _u32, _u32, C.c_float, _vp, _vp, _vp] + _extra)
    ML[f"arm_svm_{_k}_predict_f32"] = (None, [P(_inst), _vp, _vp])
    ML[f"arm_svm_{_k}_predict_f32_batch"] = (C.c_int, [P(_inst), _vp, _vp, _vp, _u32, _vp])

# The quaternion functions: 8 drop-ins and 7 _batch forms (product_single has none).  QUATERNION_FUNCS: name -> (words
# per source item, words per result item).  The product only (tests/golden/quaternion.npz holds the reference's outputs).
QUATERNION_FUNCS = {"quaternion_norm": (4, 1), "quaternion_inverse": (4, 4), "quaternion_conjugate": (4, 4),
                    "quaternion_normalize": (4, 4), "quaternion2rotation": (4, 9), "rotation2quaternion": (9, 4)}
QUATERNION = {
    **{f"arm_{f}_f32": (None, [_vp, _vp, _u32]) for f in QUATERNION_FUNCS},
    **{f"arm_{f}_f32_batch": (C.c_int, [_vp, _vp, _u32, _vp]) for f in QUATERNION_FUNCS},
    "arm_quaternion_product_f32": (None, [_vp, _vp, _vp, _u32]),
    "arm_quaternion_product_single_f32": (None, [_vp, _vp, _vp]),
    "arm_quaternion_product_f32_batch": (C.c_int, [_vp, _vp, _u32, _vp, _u32, _vp]),
}

# Interpolation: the 8 scalar drop-ins (computed on the host), the 2 spline drop-ins and the 10 _batch forms.
class arm_linear_interp_instance_f32(C.Structure):
    # Include/dsp/interpolation_functions.h:53-59
    _fields_ = [("nValues", C.c_uint32), ("x1", C.c_float), ("xSpacing", C.c_float), ("pYData", C.c_void_p)]


class arm_bilinear_interp_instance(C.Structure):
    # Include/dsp/interpolation_functions.h:64-99 (one layout for f32, q31, q15, q7)
    _fields_ = [("numRows", C.c_uint16), ("numCols", C.c_uint16), ("pData", C.c_void_p)]


arm_bilinear_interp_instance_f32 = arm_bilinear_interp_instance_q31 = arm_bilinear_interp_instance
arm_bilinear_interp_instance_q15 = arm_bilinear_interp_instance_q7 = arm_bilinear_interp_instance


class arm_spline_instance_f32(C.Structure):
    # Include/dsp/interpolation_functions.h:114-121
    _fields_ = [("type", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("n_x", C.c_uint32), ("coeffs", C.c_void_p)]


INTERP_FIXED = {"q31": C.c_int32, "q15": C.c_int16, "q7": C.c_int8}
INTERP = {
    "arm_linear_interp_f32": (C.c_float, [P(arm_linear_interp_instance_f32), C.c_float]),
    "arm_linear_interp_f32_batch": (C.c_int, [P(arm_linear_interp_instance_f32), _vp, _vp, _u32, _vp]),
    "arm_bilinear_interp_f32": (C.c_float, [P(arm_bilinear_interp_instance), C.c_float, C.c_float]),
    "arm_bilinear_interp_f32_batch": (C.c_int, [P(arm_bilinear_interp_instance), _vp, _vp, _vp, _u32, _vp]),
    **{f"arm_linear_interp_{t}": (ct, [_vp, C.c_int32, _u32]) for t, ct in INTERP_FIXED.items()},
    **{f"arm_linear_interp_{t}_batch": (C.c_int, [_vp, _u32, _vp, _vp, _u32, _vp]) for t in INTERP_FIXED},
    **{f"arm_bilinear_interp_{t}": (ct, [P(arm_bilinear_interp_instance), C.c_int32, C.c_int32])
       for t, ct in INTERP_FIXED.items()},
    **{f"arm_bilinear_interp_{t}_batch": (C.c_int, [P(arm_bilinear_interp_instance), _vp, _vp, _vp, _u32, _vp])
       for t in INTERP_FIXED},
    "arm_spline_init_f32": (None, [P(arm_spline_instance_f32), C.c_int, _vp, _vp, _u32, _vp, _vp]),
    "arm_spline_f32": (None, [P(arm_spline_instance_f32), _vp, _vp, _u32]),
    "arm_spline_init_f32_batch": (C.c_int, [C.c_int, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp]),
    "arm_spline_f32_batch": (C.c_int, [_vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp]),
}

# per-length MFCC init functions (the product and the reference build; the oracle has the
# generic init only)
MFCC_LEN = {f"arm_mfcc_init_{n}_f32": (C.c_int, [P(arm_mfcc_instance_f32), C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
            for n in RFFT_SIZES}
MFCC_LEN.update({f"arm_mfcc_init_{n}_q31": (C.c_int, [P(arm_mfcc_instance_q31), C.c_uint32, C.c_uint32, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
                 for n in RFFT_SIZES})
MFCC_LEN.update({f"arm_mfcc_init_{n}_q15": (C.c_int, [P(arm_mfcc_instance_q15), C.c_uint32, C.c_uint32, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
                 for n in RFFT_SIZES})

# per-length q31 / q15 RFFT init functions (product and reference build; the oracle has
# the generic init only)
RFFTQ_SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)
RFFTQ_LEN = {f"arm_rfft_init_{n}_{t}": (C.c_int, [P(arm_rfft_instance_q31 if t == "q31" else arm_rfft_instance_q15),
                                                 C.c_uint32, C.c_uint32])
             for n in RFFTQ_SIZES for t in ("q31", "q15")}

PARTIAL_FAST = {f"arm_{f}": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                       C.c_uint32]) for f in CONV_PARTIAL_FAST}

# the additive batched device API of include/arm_math_mi355x.h
BATCHED = {
    "arm_cfft_f32_batch": (C.c_int, [P(arm_cfft_instance_f32), C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint8,
                                     C.c_void_p]),
    "arm_cfft_q31_batch": (C.c_int, [P(arm_cfft_instance_q31), C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint8,
                                     C.c_void_p]),
    "arm_cfft_q15_batch": (C.c_int, [P(arm_cfft_instance_q15), C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint8,
                                     C.c_void_p]),
    "arm_rfft_fast_f32_batch": (C.c_int, [P(arm_rfft_fast_instance_f32), C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_uint8, C.c_void_p]),
    "arm_rfft_fast_f32_batch_ex": (C.c_int, [P(arm_rfft_fast_instance_f32), C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_uint8, C.c_uint32, C.c_void_p]),
    "arm_rfft_q31_batch": (C.c_int, [P(arm_rfft_instance_q31), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "arm_rfft_q15_batch": (C.c_int, [P(arm_rfft_instance_q15), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "arm_fir_f32_batch": (C.c_int, [P(arm_fir_instance_f32), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p]),
    "arm_fir_f32_batch_fma": (C.c_int, [P(arm_fir_instance_f32), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "arm_fir_q15_batch": (C.c_int, [P(arm_fir_instance_q15), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p]),
    "arm_fir_fast_q15_batch": (C.c_int, [P(arm_fir_instance_q15), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p]),
    "arm_fir_q31_batch": (C.c_int, [P(arm_fir_instance_q31), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p]),
    "arm_fir_fast_q31_batch": (C.c_int, [P(arm_fir_instance_q31), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p]),
    "arm_fir_q7_batch": (C.c_int, [P(arm_fir_instance_q7), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p]),
    **{f"arm_fir_{k}_batch": (C.c_int, [P(arm_fir_decimate_instance), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p])
       for k in ("decimate_f32", "decimate_q15", "decimate_fast_q15", "decimate_q31", "decimate_fast_q31")},
    **{f"arm_fir_{k}_batch": (C.c_int, [P(arm_fir_interpolate_instance), C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_void_p])
       for k in ("interpolate_f32", "interpolate_q15", "interpolate_q31")},
    **{f"arm_fir_lattice_{t}_batch": (C.c_int, [P(arm_fir_lattice_instance), C.c_void_p, C.c_void_p, C.c_uint32,
                                                C.c_uint32, C.c_void_p, C.c_void_p]) for t in ("f32", "q31", "q15")},
    **{f"{f}_batch": (C.c_int, [P(inst), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
       for f, (inst, _, _) in BIQUAD_FUNCS.items()},
    # (S, d_src, d_dst, blockSize, batch, d_state, stream)
    **{f"{f}_batch": (C.c_int, [P(inst), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
       for f, (inst, _, _) in ADAPTIVE_FUNCS.items() if "lattice" in f},
    # (S, d_src, d_ref, d_out, d_err, blockSize, batch, d_coeffs, d_state[, d_energy_x0], stream)
    **{f"{f}_batch": (C.c_int, [P(inst)] + [C.c_void_p] * 4 + [C.c_uint32] * 2 + [C.c_void_p] * (4 if "norm" in f else 3))
       for f, (inst, _, _) in ADAPTIVE_FUNCS.items() if "lms" in f},
    **{f"arm_fir_sparse_{t}_batch": (C.c_int, [P(arm_fir_sparse_instance), C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.c_uint32, C.c_void_p, C.c_void_p]) for t in ("f32", "q31", "q15", "q7")},
    "arm_mat_mult_f32_batch": (C.c_int, [P(arm_matrix_instance_f32), P(arm_matrix_instance_f32),
                                         P(arm_matrix_instance_f32), C.c_uint32, C.c_void_p]),
    "arm_mat_mult_q7_batch": (C.c_int, [P(arm_matrix_instance_q7), P(arm_matrix_instance_q7),
                                        P(arm_matrix_instance_q7), C.c_uint32, C.c_void_p]),
    "arm_mat_mult_q15_batch": (C.c_int, [P(arm_matrix_instance_q15), P(arm_matrix_instance_q15),
                                         P(arm_matrix_instance_q15), C.c_uint32, C.c_void_p]),
    "arm_mat_mult_q31_batch": (C.c_int, [P(arm_matrix_instance_q31), P(arm_matrix_instance_q31),
                                         P(arm_matrix_instance_q31), C.c_uint32, C.c_void_p]),
    "arm_mat_mult_fast_q15_batch": (C.c_int, [P(arm_matrix_instance_q15), P(arm_matrix_instance_q15),
                                              P(arm_matrix_instance_q15), C.c_uint32, C.c_void_p]),
    "arm_mat_mult_fast_q31_batch": (C.c_int, [P(arm_matrix_instance_q31), P(arm_matrix_instance_q31),
                                              P(arm_matrix_instance_q31), C.c_uint32, C.c_void_p]),
    **{f"arm_{f}_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_uint32, C.c_void_p]) for f in CONV_FULL},
    **{f"arm_{f}_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p])
       for f in CONV_PARTIAL + CONV_PARTIAL_FAST},
    "arm_mfcc_f32_batch": (C.c_int, [P(arm_mfcc_instance_f32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_void_p]),
    "arm_mfcc_q31_batch": (C.c_int, [P(arm_mfcc_instance_q31), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_void_p]),
    "arm_mfcc_q15_batch": (C.c_int, [P(arm_mfcc_instance_q15), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_void_p]),
    **{f"arm_cfft_{t}_batch_multi": (C.c_int, [P(inst), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_uint8, C.c_uint8])
       for t, inst in (("f32", arm_cfft_instance_f32), ("q31", arm_cfft_instance_q31),
                       ("q15", arm_cfft_instance_q15))},
    **{f"arm_fir_{t}_batch_multi": (C.c_int, [P(inst), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p])
       for t, inst in (("f32", arm_fir_instance_f32), ("q15", arm_fir_instance_q15), ("fast_q15", arm_fir_instance_q15),
                       ("q31", arm_fir_instance_q31), ("fast_q31", arm_fir_instance_q31), ("q7", arm_fir_instance_q7))},
    **{f"arm_mat_mult_{t}_batch_multi": (C.c_int, [P(inst), P(inst), P(inst), C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p])
       for t, inst in (("f32", arm_matrix_instance_f32), ("q15", arm_matrix_instance_q15),
                       ("q31", arm_matrix_instance_q31), ("q7", arm_matrix_instance_q7))},
    "arm_mi355x_device_count": (C.c_int, []),
    "arm_mi355x_last_error": (C.c_int, []),
    "arm_mi355x_last_error_string": (C.c_char_p, []),
    "arm_mi355x_clear_error": (None, []),
    "arm_mi355x_version": (C.c_char_p, []),
    "arm_mi355x_table_cache_bytes": (C.c_size_t, []),
    "arm_mi355x_set_table_cache_limit": (None, [C.c_size_t]),
    "arm_mi355x_release_thread_resources": (None, []),
    "arm_mi355x_thread_resource_owners": (C.c_int, []),
}

# exported data symbols (arm_const_structs.h / arm_common_tables.h)
DATA = ([f"arm_cfft_sR_{t}_len{n}" for t in ("f32", "q31", "q15") for n in SIZES]
        + [f"arm_rfft_fast_sR_f32_len{n}" for n in RFFT_SIZES]
        + [f"twiddleCoef_{n}" for n in SIZES] + [f"twiddleCoef_{n}_q31" for n in SIZES]
        + [f"twiddleCoef_{n}_q15" for n in SIZES] + [f"twiddleCoef_rfft_{n}" for n in RFFT_SIZES]
        + [f"armBitRevIndexTable{n}" for n in SIZES] + [f"armBitRevIndexTable_fixed_{n}" for n in SIZES])


def bind(lib, table, prefix=""):
    """Attach restype/argtypes for every function of `table` (optionally name-prefixed)."""
    for name, (res, args) in table.items():
        fn = getattr(lib, prefix + name)
        fn.restype = res
        fn.argtypes = args
    return lib
