"""numpy restatement of arm_mat_cmplx_mult_{f32,q31,q15} and the input generators of their tests.

Operands are the real arrays the functions see in memory: a [..., M, 2K] and b [..., K, 2N] of
interleaved (re, im) words, the result [..., M, 2N].  The complex product is the real product of a with
the embedded b' = embed(b) [..., 2K, 2N]:

    b'[2k][2n] = c    b'[2k][2n+1] = d    b'[2k+1][2n] = -d    b'[2k+1][2n+1] = c      (b[k][n] = c + jd)

  q15  (arm_mat_cmplx_mult_q15.c, !ARM_MATH_DSP): q63 sums of exact products, __SSAT(sum >> 15, 16); the call
       leaves b transposed (N rows of K complex words) in pScratch
  q31  (arm_mat_cmplx_mult_q31.c, scalar branch): q63 sums wrapping mod 2^64, clip_q63_to_q31(sum >> 31)
  f32  (arm_mat_cmplx_mult_f32.c): each product rounded, added in the order re += a c, im += b c,
       re -= b d, im += a d, k ascending from +0
"""
import numpy as np

KINDS = {"f32": np.float32, "q31": np.int32, "q15": np.int16}
BITS = {"q31": 31, "q15": 15}
# complex (M, K, N)
SHAPES = [(1, 1, 1), (3, 5, 2), (7, 33, 5), (17, 33, 9), (40, 40, 40), (5, 130, 3)]
TINY = np.finfo(np.float32).tiny


def embed(b):
    """b [..., K, 2N] -> b' [..., 2K, 2N].  -d wraps for the fixed-point minimum (use embed64 there)."""
    b = np.asarray(b)
    k, n2 = b.shape[-2:]
    out = np.empty(b.shape[:-2] + (2 * k, n2), dtype=b.dtype)
    c, d = b[..., 0::2], b[..., 1::2]
    out[..., 0::2, 0::2], out[..., 0::2, 1::2] = c, d
    with np.errstate(over="ignore"):
        out[..., 1::2, 0::2], out[..., 1::2, 1::2] = -d, c
    return out


def embed64(b):
    return embed(np.asarray(b).astype(np.int64))


def wrap_matmul64(a, b):
    """a [..., M, K] @ b [..., K, N] in int64, wrapping mod 2^64 (every partial product is exact: |x y| <= 2^62)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    with np.errstate(over="ignore"):
        acc = np.zeros(a.shape[:-1] + b.shape[-1:], dtype=np.uint64)
        for k in range(a.shape[-1]):
            acc += (a[..., :, k, None] * b[..., k, None, :]).view(np.uint64)
    return acc.view(np.int64)


def fixed_sums(kind, a, b):
    """The q63 sums before the shift (wrapped)."""
    assert kind in BITS
    return wrap_matmul64(a, embed64(b))


def mult_fixed(kind, a, b):
    dt = KINDS[kind]
    info = np.iinfo(dt)
    return np.clip(fixed_sums(kind, a, b) >> BITS[kind], info.min, info.max).astype(dt)


def scratch_q15(b):
    """pScratch after arm_mat_cmplx_mult_q15: b [K, 2N] transposed as complex, flat (2 K N words)."""
    b = np.asarray(b, dtype=np.int16)
    k, n2 = b.shape
    return np.ascontiguousarray(b.reshape(k, n2 // 2, 2).transpose(1, 0, 2)).reshape(-1)


def mult_f32_ref(a, b):
    """The reference's words: rounded products, mul-then-add in its order."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ar, ai = a[..., :, 0::2], a[..., :, 1::2]
    br, bi = b[..., :, 0::2], b[..., :, 1::2]
    re = np.zeros(a.shape[:-1] + (b.shape[-1] // 2,), dtype=np.float32)
    im = np.zeros_like(re)
    with np.errstate(under="ignore"):
        for k in range(b.shape[-2]):
            x, y = ar[..., :, k, None], ai[..., :, k, None]
            c, d = br[..., k, None, :], bi[..., k, None, :]
            re = re + x * c
            im = im + y * c
            re = re - y * d
            im = im + x * d
    out = np.empty(re.shape[:-1] + (2 * re.shape[-1],), dtype=np.float32)
    out[..., 0::2], out[..., 1::2] = re, im
    return out


def exact64(a, b):
    return np.matmul(np.asarray(a, dtype=np.float64), embed(np.asarray(b, dtype=np.float64)))


def bound(a, b):
    """2K 2^-24 (|A||B'|)ij + 2K 2^-150: the recursive-summation bound of the 2K-term f32 dot product.  The
    first term is the relative-error model fl(x) = x (1 + delta), |delta| <= 2^-24, which holds only while
    results are normal; under gradual underflow a rounded product or fma is x (1 + delta) + eta with
    |eta| <= 2^-150 (half the smallest subnormal; additions are exact there), once per term, which is the
    second term.  It matters only where every product is subnormal (at K = 1 such a product is off by up to
    2^-150 from float64 in any f32 arithmetic, the reference's included, against a first term near 2^-155)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    k2 = a.shape[-1]
    return k2 * 2.0 ** -24 * np.matmul(a, np.abs(embed(np.asarray(b, dtype=np.float64)))) + k2 * 2.0 ** -150


def saturated(kind, out):
    info = np.iinfo(KINDS[kind])
    return (out == info.min), (out == info.max)


# ------------------------------------------------------------------ inputs
def fill_fixed(kind, fill, shape, k, rng):
    """Words of `shape` for a product of complex depth k.  full: the whole range; scaled: |v| <= 2^bits /
    (2 sqrt(k)), so the 2k products of a sum are each <= 2^(2 bits) / (4k), |sum| <= 2^(2 bits - 1) and
    |sum >> bits| <= 2^(bits - 1): nothing saturates; min: every word the minimum; extreme: drawn from
    {min, max, 0, -1, 1}."""
    dt = KINDS[kind]
    info = np.iinfo(dt)
    if fill == "full":
        return rng.integers(info.min, info.max, shape, endpoint=True).astype(dt)
    if fill == "scaled":
        lim = int(2.0 ** BITS[kind] / (2.0 * np.sqrt(k)))
        return rng.integers(-lim, lim, shape, endpoint=True).astype(dt)
    if fill == "min":
        return np.full(shape, info.min, dtype=dt)
    if fill == "extreme":
        return rng.choice(np.array([info.min, info.max, 0, -1, 1], dtype=dt), shape)
    raise ValueError(fill)


def fill_f32(fill, shape, rng):
    """uniform [-1, 1); mixed: exponents over 2^-20 .. 2^20 with +-0; subnormal: |x y| in [2^-134, 2^-132)."""
    if fill == "uniform":
        return rng.uniform(-1, 1, shape).astype(np.float32)
    if fill == "mixed":
        v = rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.integers(-20, 21, shape)
        z = rng.uniform(0, 1, shape)
        v[z < 0.1] = 0.0
        v[(z >= 0.1) & (z < 0.2)] = -0.0
        return v.astype(np.float32)
    if fill == "subnormal":
        return (rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape) * 2.0 ** -66).astype(np.float32)
    raise ValueError(fill)


def operands(kind, fill, m, k, n, rng, batch=None):
    """(a, b) real arrays [(batch,) M, 2K] and [(batch,) K, 2N]."""
    pre = () if batch is None else (batch,)
    sa, sb = pre + (m, 2 * k), pre + (k, 2 * n)
    if kind == "f32":
        return fill_f32(fill, sa, rng), fill_f32(fill, sb, rng)
    return fill_fixed(kind, fill, sa, k, rng), fill_fixed(kind, fill, sb, k, rng)
