"""numpy restatement of the reference's quaternion functions (Source/QuaternionMathFunctions, the scalar branches built
with -ffp-contract=off) and the operands of tests/golden/quaternion.npz.  Every operation is one float32 operation,
in the order the reference writes it; sqrt and the division are correctly rounded in numpy as in C.

  norm         sqrt(((w*w + x*x) + y*y) + z*z)
  inverse      (w / s, -x / s, -y / s, -z / s) with s the sum of squares;  conjugate (w, -x, -y, -z)
  normalize    every word / norm
  product      the Hamilton product, each word's four products summed left to right
  to_rotation  arm_quaternion2rotation_f32;  from_rotation  arm_rotation2quaternion_f32 with branch() naming the branch
               each rotation takes (0: trace > 0; 1: r00 the strictly largest diagonal word; 2: r11 > r22; 3: the rest)
Every item is independent of its neighbours, so the expected words of a prefix or of a tiling of the operands are the
prefix or the tiling of the expected words.
"""
import zlib

import numpy as np

F = np.float32
MARK = F(1.5365222e+16)
FUNCS = ("quaternion_norm", "quaternion_inverse", "quaternion_conjugate", "quaternion_normalize",
         "quaternion2rotation", "rotation2quaternion")
WORDS = {"quaternion_norm": (4, 1), "quaternion_inverse": (4, 4), "quaternion_conjugate": (4, 4),
         "quaternion_normalize": (4, 4), "quaternion2rotation": (4, 9), "rotation2quaternion": (9, 4)}
RANDOM_Q = 224                                               # random quaternions before the special ones
RANDOM_R = 256                                               # rotations of unit quaternions before the other kinds


def same_word(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the restatement ------------------------------------------------------------------------------------------------
def _q(a):
    a = np.ascontiguousarray(a, dtype=F).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def squares(q):
    w, x, y, z = _q(q)
    with np.errstate(all="ignore"):
        return w * w + x * x + y * y + z * z


def norm(q):
    with np.errstate(all="ignore"):
        return np.sqrt(squares(q))


def inverse(q):
    w, x, y, z = _q(q)
    s = squares(q)
    with np.errstate(all="ignore"):
        return np.stack([w / s, -x / s, -y / s, -z / s], axis=1)


def conjugate(q):
    w, x, y, z = _q(q)
    return np.stack([w, -x, -y, -z], axis=1)


def normalize(q):
    n = norm(q)
    with np.errstate(all="ignore"):
        return np.stack([c / n for c in _q(q)], axis=1)


def product(a, b):
    """a [n, 4] times b [n, 4] or one quaternion b [4]."""
    a0, a1, a2, a3 = _q(a)
    b0, b1, b2, b3 = _q(b)
    with np.errstate(all="ignore"):
        return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                         a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                         a0 * b2 + a2 * b0 + a3 * b1 - a1 * b3,
                         a0 * b3 + a3 * b0 + a1 * b2 - a2 * b1], axis=1).astype(F)


def to_rotation(q):
    w, x, y, z = _q(q)
    two = F(2)
    with np.errstate(all="ignore"):
        q00, q11, q22, q33 = w * w, x * x, y * y, z * z
        q01, q02, q03, q12, q13, q23 = w * x, w * y, w * z, x * y, x * z, y * z
        return np.stack([q00 + q11 - q22 - q33, two * (q12 - q03), two * (q13 + q02),
                         two * (q12 + q03), q00 - q11 + q22 - q33, two * (q23 - q01),
                         two * (q13 - q02), two * (q23 + q01), q00 - q11 - q22 + q33], axis=1).astype(F)


def _r(r):
    r = np.ascontiguousarray(r, dtype=F).reshape(-1, 9)
    return [r[:, k] for k in range(9)]


def branch(r):
    """The branch of arm_rotation2quaternion_f32 each rotation takes: 0 .. 3."""
    r00, _, _, _, r11, _, _, _, r22 = _r(r)
    with np.errstate(all="ignore"):
        trace = r00 + r11 + r22
        return np.where(trace > 0, 0, np.where((r00 > r11) & (r00 > r22), 1, np.where(r11 > r22, 2, 3)))


def from_rotation(r):
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = _r(r)
    one, two, quarter = F(1), F(2), F(0.25)
    with np.errstate(all="ignore"):
        trace = r00 + r11 + r22
        out = []
        d = np.sqrt(trace + one) * two
        s = one / d
        out.append(np.stack([quarter * d, (r21 - r12) * s, (r02 - r20) * s, (r10 - r01) * s], axis=1))
        d = np.sqrt(one + r00 - r11 - r22) * two
        s = one / d
        out.append(np.stack([(r21 - r12) * s, quarter * d, (r01 + r10) * s, (r02 + r20) * s], axis=1))
        d = np.sqrt(one + r11 - r00 - r22) * two
        s = one / d
        out.append(np.stack([(r02 - r20) * s, (r01 + r10) * s, quarter * d, (r12 + r21) * s], axis=1))
        d = np.sqrt(one + r22 - r00 - r11) * two
        s = one / d
        out.append(np.stack([(r10 - r01) * s, (r02 + r20) * s, (r12 + r21) * s, quarter * d], axis=1))
    b = branch(r)
    return np.choose(b[:, None], out).astype(F)


def apply(func, src):
    return {"quaternion_norm": norm, "quaternion_inverse": inverse, "quaternion_conjugate": conjugate,
            "quaternion_normalize": normalize, "quaternion2rotation": to_rotation,
            "rotation2quaternion": from_rotation}[func](src)


# ---- the operands ---------------------------------------------------------------------------------------------------
def _special_quaternions():
    nan, inf, tiny = F(np.nan), F(np.inf), F(2.0 ** -140)
    return np.array([[0, 0, 0, 0], [-0.0, -0.0, -0.0, -0.0], [1, 0, 0, 0], [0, 0, 0, -1], [nan, 1, 2, 3],
                     [1, 2, nan, 3], [1, 2, 3, nan], [inf, 1, 1, 1], [1, -inf, 1, 1], [tiny, tiny, -tiny, tiny],
                     [tiny, 0, 0, 0], [3e19, 1, 1, 1], [1e19, -1e19, 1e19, 1e19], [1e-20, 1e-20, 1e-20, 1e-20],
                     [0.5, 0.5, 0.5, 0.5], [-0.5, 0.5, -0.5, 0.5]], dtype=F)


def quaternions(which="a"):
    """[RANDOM_Q + the special ones, 4]: half of the random ones are unit quaternions within rounding, half are
    scaled by 2^k, k in [-12, 12]; `which` "b" is a second, independent set (the products' other factor)."""
    rng = _rng("quaternions/" + which)
    q = rng.normal(0.0, 1.0, (RANDOM_Q, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[RANDOM_Q // 2:] *= 2.0 ** rng.integers(-12, 13, (RANDOM_Q - RANDOM_Q // 2, 1))
    special = _special_quaternions()
    if which == "b":
        special = special[::-1]
    return np.concatenate([q.astype(F), special])


def _special_rotations():
    nan = np.nan
    diag = lambda a, b, c: [a, 0, 0, 0, b, 0, 0, 0, c]     # noqa: E731
    return np.array([diag(1, 1, 1), diag(0, 0, 0), diag(1, -1, 0), diag(-1, 1, 0), diag(0, -1, 1), diag(-1, -1, -1),
                     diag(2, 2, -5), diag(-5, 2, 2), diag(nan, 2, 1), diag(nan, 1, 2), diag(1, nan, 2), diag(1, 2, nan),
                     [nan] * 9, [0, 1, 2, 3, 0, 5, 6, 7, 0], [-3, 1, 2, 3, -3, 5, 6, 7, -3],
                     [1, np.inf, 0, 0, 1, 0, 0, 0, 1]], dtype=F)


def rotations(seed=0):
    """[RANDOM_R + 64 + the special ones, 9]: the rotations of unit quaternions whose largest word cycles through w,
    x, y, z (so the four branches are each taken), 64 matrices of plain normal words (square roots of negative
    numbers), and the special ones: a trace of exactly 0, ties on the diagonal, NaNs on it."""
    rng = _rng(f"rotations/{seed}")
    q = rng.normal(0.0, 0.35, (RANDOM_R, 4))
    q[np.arange(RANDOM_R), np.arange(RANDOM_R) % 4] += rng.choice([-1.0, 1.0], RANDOM_R) * 1.5
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    plain = rng.normal(0.0, 1.0, (64, 9)).astype(F)
    return np.concatenate([to_rotation(q.astype(F)), plain, _special_rotations()])


def balanced(r):
    """Each of the four branches holds at least one eighth of the rotations."""
    return bool((np.bincount(branch(r), minlength=4) * 8 >= len(r)).all())
