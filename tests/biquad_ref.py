"""numpy restatement of the eight biquad cascade functions (reference scalar path), vectorised across
streams with a Python loop over time.  f32 kinds use np.float32 arithmetic (every product and sum
rounded, no FMA); fixed-point kinds use int64 with explicit wrap-around and saturation.  It must equal
tests/golden/biquad.npz (the reference's own outputs) bit for bit, and gives the expected values for
shapes the fixtures do not hold.

    y, new_state = run(func, coeffs, post_shift, x, state)

x [batch, CH*blockSize], state [batch, K*numStages] in the reference's layout, coeffs [NC*numStages].
"""
import numpy as np

# func -> (sample dtype, state dtype, state words / stage, coefficients / stage, channels)
FUNCS = {
    "arm_biquad_cascade_df1_f32": (np.float32, np.float32, 4, 5, 1),
    "arm_biquad_cascade_df1_q31": (np.int32, np.int32, 4, 5, 1),
    "arm_biquad_cascade_df1_fast_q31": (np.int32, np.int32, 4, 5, 1),
    "arm_biquad_cascade_df1_q15": (np.int16, np.int16, 4, 6, 1),
    "arm_biquad_cascade_df1_fast_q15": (np.int16, np.int16, 4, 6, 1),
    "arm_biquad_cas_df1_32x64_q31": (np.int32, np.int64, 4, 5, 1),
    "arm_biquad_cascade_df2T_f32": (np.float32, np.float32, 2, 5, 1),
    "arm_biquad_cascade_stereo_df2T_f32": (np.float32, np.float32, 4, 5, 2),
}
HAS_SHIFT = {f for f in FUNCS if f.endswith(("q31", "q15"))}

_I64 = np.int64


def _w32(v):
    """int64 -> the value of its low 32 bits, as int64."""
    return v.astype(np.int32).astype(_I64)


def _shl64(v, s):
    return (v.view(np.uint64) << np.uint64(s)).view(_I64)


def _mult32x64(x, y):
    return (((x & _I64(0xFFFFFFFF)) * y) >> _I64(32)) + ((x >> _I64(32)) * y)


def _df1_f32(c, ps, x, st):
    b0, b1, b2, a1, a2 = (np.float32(v) for v in c)
    x1, x2, y1, y2 = (st[:, i].copy() for i in range(4))
    y = np.empty_like(x)
    for n in range(x.shape[1]):
        xn = x[:, n]
        acc = b0 * xn
        acc = acc + b1 * x1
        acc = acc + b2 * x2
        acc = acc + a1 * y1
        acc = acc + a2 * y2
        x2, x1, y2, y1 = x1, xn, y1, acc
        y[:, n] = acc
    return y, np.stack([x1, x2, y1, y2], axis=1)


def _df1_fixed(kind):
    def run(c, ps, x, st):
        if kind in ("q15", "fast_q15"):
            b0, _, b1, b2, a1, a2 = (_I64(v) for v in c)
        else:
            b0, b1, b2, a1, a2 = (_I64(v) for v in c)
        x1, x2, y1, y2 = (st[:, i].astype(_I64) for i in range(4))
        if kind == "32x64":
            x1, x2 = _w32(x1), _w32(x2)                                     # (q31_t) pState[0], [1]
        y = np.empty(x.shape, dtype=_I64)
        xs = x.astype(_I64)
        for n in range(x.shape[1]):
            xn = xs[:, n]
            if kind == "q31":
                acc = b0 * xn + b1 * x1 + b2 * x2 + a1 * y1 + a2 * y2      # int64 wraps
                yn = _w32(acc >> _I64(31 - ps))
            elif kind == "fast_q31":
                r = _I64(1 << 31)
                acc = sum(((k * v + r) >> _I64(32)) for k, v in ((b0, xn), (b1, x1), (b2, x2), (a1, y1), (a2, y2)))
                yn = _w32(_shl64(_w32(acc), ps + 1))
            elif kind == "q15":
                acc = b0 * xn + b1 * x1 + b2 * x2 + a1 * y1 + a2 * y2
                yn = np.clip(_w32(acc >> _I64(15 - ps)), -32768, 32767)
            elif kind == "fast_q15":
                acc = _w32(b0 * xn + b1 * x1 + b2 * x2 + a1 * y1 + a2 * y2)
                yn = np.clip(acc >> _I64(15 - ps), -32768, 32767)
            else:                                                           # 32x64: y1, y2 are q63
                acc = xn * b0 + x1 * b1 + x2 * b2 + _mult32x64(y1, a1) + _mult32x64(y2, a2)
                yn = _w32(acc >> _I64(31 - ps))
                x2, x1, y2, y1 = x1, xn, y1, _shl64(acc, ps + 1)
                y[:, n] = yn
                continue
            x2, x1, y2, y1 = x1, xn, y1, yn
            y[:, n] = yn
        return y.astype(x.dtype), np.stack([x1, x2, y1, y2], axis=1).astype(st.dtype)
    return run


def _df2t_chan(c, x, d1, d2, stereo):
    b0, b1, b2, a1, a2 = (np.float32(v) for v in c)
    y = np.empty_like(x)
    for n in range(x.shape[1]):
        xn = x[:, n]
        acc = b0 * xn + d1
        if stereo:
            d1 = (b1 * xn + a1 * acc) + d2
        else:
            d1 = (b1 * xn + d2) + a1 * acc
        d2 = b2 * xn + a2 * acc
        y[:, n] = acc
    return y, d1, d2


def _df2t(c, ps, x, st):
    y, d1, d2 = _df2t_chan(c, x, st[:, 0].copy(), st[:, 1].copy(), False)
    return y, np.stack([d1, d2], axis=1)


def _stereo(c, ps, x, st):
    y = np.empty_like(x)
    ya, d1a, d2a = _df2t_chan(c, x[:, 0::2], st[:, 0].copy(), st[:, 1].copy(), True)
    yb, d1b, d2b = _df2t_chan(c, x[:, 1::2], st[:, 2].copy(), st[:, 3].copy(), True)
    y[:, 0::2], y[:, 1::2] = ya, yb
    return y, np.stack([d1a, d2a, d1b, d2b], axis=1)


_STAGE = {
    "arm_biquad_cascade_df1_f32": _df1_f32,
    "arm_biquad_cascade_df1_q31": _df1_fixed("q31"),
    "arm_biquad_cascade_df1_fast_q31": _df1_fixed("fast_q31"),
    "arm_biquad_cascade_df1_q15": _df1_fixed("q15"),
    "arm_biquad_cascade_df1_fast_q15": _df1_fixed("fast_q15"),
    "arm_biquad_cas_df1_32x64_q31": _df1_fixed("32x64"),
    "arm_biquad_cascade_df2T_f32": _df2t,
    "arm_biquad_cascade_stereo_df2T_f32": _stereo,
}


def run(func, coeffs, post_shift, x, state):
    dt, sdt, ks, nc, ch = FUNCS[func]
    x = np.ascontiguousarray(x, dtype=dt)
    state = np.ascontiguousarray(state, dtype=sdt)
    coeffs = np.asarray(coeffs)
    stages = len(coeffs) // nc
    assert x.ndim == 2 and x.shape[1] % ch == 0 and state.shape == (x.shape[0], ks * stages)
    new_state = np.empty_like(state)
    y = x
    with np.errstate(over="ignore", under="ignore"):
        for s in range(stages):
            y, new_state[:, ks * s:ks * (s + 1)] = _STAGE[func](coeffs[nc * s:nc * (s + 1)], int(post_shift), y,
                                                                state[:, ks * s:ks * (s + 1)])
    return y, new_state


def stable_coeffs(func, stages, post_shift, seed):
    """Coefficients for shapes outside the fixtures: stable sections (conjugate poles of radius 0.3 .. 0.7
    with |a1| < 1, so fixed-point words hold them at post_shift 0), numerator scaled to a peak magnitude
    response of 1, so long cascades neither blow up nor die out; quantised for the function's type."""
    dt, _, _, nc, _ = FUNCS[func]
    rng = np.random.default_rng(seed)
    z1 = np.exp(-1j * np.linspace(0, np.pi, 256))
    rows = []
    for _ in range(stages):
        r, t = rng.uniform(0.3, 0.7), rng.uniform(1.1, 2.0)
        a1, a2 = 2 * r * np.cos(t), -r * r
        b = np.array([1.0, rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)])
        b /= np.abs((b[0] + b[1] * z1 + b[2] * z1 * z1) / (1 - a1 * z1 - a2 * z1 * z1)).max()
        rows.append([*b, a1, a2])
    rows = np.array(rows)
    if dt == np.float32:
        return rows.astype(np.float32).reshape(-1)
    bits = 15 if dt == np.int16 else 31
    q = np.clip(np.round(rows / 2.0 ** post_shift * 2.0 ** bits), -2 ** bits, 2 ** bits - 1).astype(dt)
    if nc == 6:                                    # q15: {b0, 0, b1, b2, a1, a2}
        q = np.concatenate([q[:, :1], np.zeros((stages, 1), dt), q[:, 1:]], axis=1)
    return q.reshape(-1)
