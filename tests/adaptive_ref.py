"""Numpy restatement of the reference's IIR lattice and LMS / normalised LMS filters (scalar build:
ARM_MATH_LOOPUNROLL on, ARM_MATH_DSP and Neon off, -ffp-contract=off), vectorised over streams.

    arm_iir_lattice_{f32,q31,q15}, arm_lms_{f32,q31,q15}, arm_lms_norm_{f32,q15}, arm_recip_q15

f32 works on float32 arrays, every product rounded before it is added; fixed point works on int64 with
explicit wraps and saturations.  tests/test_adaptive.py holds this file to tests/golden/adaptive.npz (the
reference's own outputs) bit for bit, then uses it as the checker of the batched device API.
"""
import numpy as np

F32, Q31, Q15 = np.float32, np.int32, np.int16
# function -> (word type, family)
FUNCS = {
    "arm_iir_lattice_f32": (F32, "iir"), "arm_iir_lattice_q31": (Q31, "iir"), "arm_iir_lattice_q15": (Q15, "iir"),
    "arm_lms_f32": (F32, "lms"), "arm_lms_q31": (Q31, "lms"), "arm_lms_q15": (Q15, "lms"),
    "arm_lms_norm_f32": (F32, "nlms"), "arm_lms_norm_q15": (Q15, "nlms"),
}
MAX_POST_SHIFT = {Q31: 30, Q15: 14}          # beyond: a shift count outside 0...31 in the reference
DELTA_Q15 = 5
EPS_F32 = np.float32(0.000000119209289)


def wrap(v, bits):
    half = 1 << (bits - 1)
    return ((v + half) & ((1 << bits) - 1)) - half


def sat(v, bits):
    half = 1 << (bits - 1)
    return np.clip(v, -half, half - 1)


def recip_table():
    """armRecipTableQ15: the mean of the reciprocals of the ends of [1 + i/64, 1 + (i+1)/64], q15 with one
    integer bit, rounded down."""
    i = np.arange(64, dtype=np.int64)
    return ((1 << 20) * (129 + 2 * i) // ((64 + i) * (65 + i))).astype(np.int16)


def recip_q15(arg, table):
    """arm_recip_q15 (Include/dsp/utils.h) on int64 arrays holding q15 words: (out, signBits + 1)."""
    arg = np.asarray(arg, dtype=np.int64)
    mag = np.where(arg > 0, arg, -arg)
    if (mag == 0).any() or (mag == 32768).any():
        raise ValueError("arm_recip_q15: argument 0 or -32768 (undefined shift count in the reference)")
    sign_bits = (32 - np.frexp(mag.astype(np.float64))[1]) - 17          # __CLZ(mag) - 17
    x = wrap(arg << sign_bits, 16)
    out = table.astype(np.int64)[(x >> 8) & 63]
    for _ in range(2):
        t = 0x7FFF - ((x * out) >> 15)
        out = wrap((out * t) >> 14, 16)
    return out, sign_bits + 1


# ------------------------------------------------------------------ IIR lattice
def iir_lattice(func, k, v, x, state):
    """k [N], v [N + 1] shared; x [S][B]; state [S][N], the live words.  Returns (y, new state)."""
    dt, fam = FUNCS[func]
    assert fam == "iir"
    n_st = len(k)
    assert len(v) == n_st + 1 and state.shape == (x.shape[0], n_st) and n_st >= 1
    y = np.zeros_like(x)
    if dt == F32:
        s = state.astype(F32).copy()
        k, v = k.astype(F32), v.astype(F32)
        with np.errstate(all="ignore"):
            for n in range(x.shape[1]):
                f = x[:, n].astype(F32)
                acc = np.zeros(x.shape[0], F32)
                for j in range(n_st):
                    g = s[:, j].copy()
                    f = f - k[j] * g
                    gn = g + k[j] * f
                    acc = acc + gn * v[j]
                    if j:
                        s[:, j - 1] = gn
                s[:, n_st - 1] = f
                y[:, n] = acc + f * v[n_st]
        return y, s
    s = state.astype(np.int64)
    k, v = k.astype(np.int64), v.astype(np.int64)
    for n in range(x.shape[1]):
        f = x[:, n].astype(np.int64)
        acc = np.zeros(x.shape[0], np.int64)
        for j in range(n_st):
            g = s[:, j].copy()
            if dt == Q31:
                f = sat(f - wrap((g * k[j]) >> 31, 32), 32)
                gn = sat(g + wrap((f * k[j]) >> 31, 32), 32)
            else:
                f = sat(f - ((g * k[j]) >> 15), 16)
                gn = sat(((f * k[j]) >> 15) + g, 16)
            acc = acc + gn * v[j]                       # int64 wraps as the reference's q63_t does
            if j:
                s[:, j - 1] = gn
        s[:, n_st - 1] = f
        acc = acc + f * v[n_st]
        y[:, n] = wrap(acc >> 31, 32) if dt == Q31 else sat(wrap(acc >> 15, 32), 16)
    return y, s.astype(dt)


# ------------------------------------------------------------------ LMS / normalised LMS
def _recombine(acc, lshift, ushift):
    lo, hi = acc & 0xFFFFFFFF, (acc >> 32) & 0xFFFFFFFF
    return wrap(((lo >> lshift) | (hi << ushift)) & 0xFFFFFFFF, 32)


def lms(func, mu, post_shift, x, d, coeffs, state, ex=None, table=None):
    """x, d [S][B]; coeffs [S][T] (time-reversed); state [S][T - 1] (oldest first); normalised: ex [S][2]
    {energy, x0}.  Returns (out, err, new coeffs, new state, new ex or None)."""
    dt, fam = FUNCS[func]
    norm = fam == "nlms"
    assert fam in ("lms", "nlms") and (ex is not None) == norm
    n_s, n_b = x.shape
    taps = coeffs.shape[1]
    assert taps >= 1 and state.shape == (n_s, taps - 1) and d.shape == x.shape
    out, err = np.zeros_like(x), np.zeros_like(x)
    if dt == F32:
        mu = F32(mu)
        full = np.concatenate([state.astype(F32), x.astype(F32)], axis=1)
        c = coeffs.astype(F32).copy()
        if norm:
            energy, x0 = ex[:, 0].astype(F32).copy(), ex[:, 1].astype(F32).copy()
        with np.errstate(all="ignore"):
            for n in range(n_b):
                w = full[:, n:n + taps]
                if norm:
                    energy = energy - x0 * x0
                    energy = energy + x[:, n] * x[:, n]
                prod = w * c
                acc = np.zeros(n_s, F32)
                for i in range(taps):
                    acc = acc + prod[:, i]
                e = d[:, n] - acc
                out[:, n], err[:, n] = acc, e
                wt = (e * mu) / (energy + EPS_F32) if norm else e * mu
                c = c + wt[:, None] * w
                if norm:
                    x0 = w[:, 0].copy()
        nex = np.stack([energy, x0], axis=1) if norm else None
        return out, err, c, full[:, n_b:n_b + taps - 1].copy(), nex
    assert 0 <= post_shift <= MAX_POST_SHIFT[dt], "postShift outside the reference's defined range"
    mu = int(mu)
    full = np.concatenate([state.astype(np.int64), x.astype(np.int64)], axis=1)
    c = coeffs.astype(np.int64)
    if norm:
        table = recip_table() if table is None else table
        energy, x0 = ex[:, 0].astype(np.int64), ex[:, 1].astype(np.int64)
    for n in range(n_b):
        w = full[:, n:n + taps]
        acc = (w * c).sum(axis=1)                           # int64 wraps; any order gives the same words
        if dt == Q31:
            us = post_shift + 1
            y = _recombine(acc, 32 - us, us)
            e = wrap(d[:, n].astype(np.int64) - y, 32)
            alpha = wrap((e * mu) >> 31, 32)
            c = sat(c + wrap(((alpha[:, None] * w) >> 32) << 1, 32), 32)
        else:
            ls = 15 - post_shift
            y = sat(_recombine(acc, ls, 32 - ls), 16)
            e = wrap(d[:, n].astype(np.int64) - y, 16)
            if norm:
                xn = full[:, n + taps - 1]
                energy = sat(energy - ((x0 * x0) >> 15) + ((xn * xn) >> 15), 16)
                one, ps = recip_q15(wrap(energy + DELTA_Q15, 16), table)
                emu = wrap((e * mu) >> 15, 16)
                assert (ps <= 15).all()
                alpha = sat(wrap((emu * one) >> (15 - ps), 32), 16)
            else:
                alpha = wrap((e * mu) >> 15, 16)
            c = sat(c + ((alpha[:, None] * w) >> 15), 16)
            if norm:
                x0 = w[:, 0].copy()
        out[:, n], err[:, n] = y, e
    nex = np.stack([energy, x0], axis=1).astype(dt) if norm else None
    return out, err, c.astype(dt), full[:, n_b:n_b + taps - 1].astype(dt), nex


# ------------------------------------------------------------------ inputs for tests and benchmarks
def quantise(a, dt):
    if dt == F32:
        return np.asarray(a, dtype=F32)
    bits = 31 if dt == Q31 else 15
    return np.clip(np.round(np.asarray(a, dtype=np.float64) * 2.0 ** bits), -2 ** bits, 2 ** bits - 1).astype(dt)


def lattice_coeffs(func, stages, seed):
    """A stable lattice (|k| <= 0.9, most stages far smaller) with a bounded ladder: (k, v)."""
    dt, _ = FUNCS[func]
    rng = np.random.default_rng(seed)
    k = rng.uniform(-0.9, 0.9, stages) * np.where(np.arange(stages) < 4, 1.0, 0.25)
    v = rng.uniform(-1, 1, stages + 1) / (stages + 1)
    return quantise(k, dt), quantise(v, dt)


def signal(func, shape, seed, scale=0.5):
    dt, _ = FUNCS[func]
    return quantise(np.random.default_rng(seed).uniform(-scale, scale, shape), dt)


def default_mu(func):
    dt, fam = FUNCS[func]
    return F32(0.05 if fam == "lms" else 0.5) if dt == F32 else int(quantise(0.05 if fam == "lms" else 0.3, dt))
