"""numpy restatement of arm_vexp_f32 / arm_vlog_f32, the log-domain statistics, the linear / polynomial / rbf SVMs and
the Gaussian naive Bayes estimator (the reference's scalar branches built with -D__GNUC_PYTHON__ -DARM_MATH_LOOPUNROLL
-ffp-contract=off), and the case list of tests/golden/ml.npz.  expf and logf are the host libm's through ctypes; the
fixtures pin them (a host whose libm differs fails test_ml.py's restatement test, not the GPU tests' expectations,
which are the stored words).

  entropy             -chain(p * logf(p));  kullback_leibler  -chain(pA * logf(pB / pA))
  logsumexp           max by strict > from element 0, accum = chain(expf(x - max)), max + logf(accum);
  logsumexp_dot_prod  the same on a + b
  SVM                 per support vector dot = chain(in * sv) or chain((in - sv)^2); from sum = intercept, in row
                      order, sum += dual * dot | dual * exponent(gamma * dot + coef0, degree) | dual * expf(-gamma *
                      dot); class = classes[sum <= 0 ? 0 : 1]
  Bayes               per class acc1 = chain(logf((2 pi) * (sigma + eps))), acc2 = chain((in - theta)^2 / (sigma + eps)),
                      (-0.5 * acc1 - 0.5 * acc2) + logf(prior); the index by arm_max_f32 (replaced on out < v only)
Every chain starts from 0.0f and rounds each term before its add.
"""
import ctypes
import ctypes.util
import zlib

import numpy as np

F = np.float32
MARK = F(1.5365222e+16)
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 129, 1000)
SVS = (1, 2, 3, 5, 64, 65, 130)
CLASSES = (1, 2, 3, 7)
DEGREES = (1, 2, 3, 5)
ITEMS = 16                                                   # vectors per classifier case
LANE_MIN_BATCH = 4096                                        # chain_f32.hpp kSumLaneMinBatch
LOGDOM_FUNCS = ("entropy", "kullback_leibler", "logsumexp", "logsumexp_dot_prod")
LOGDOM_KINDS = ("prob", "logp", "zero", "nan0", "nanmid", "equal")
SVM_KINDS = ("linear", "polynomial", "rbf")
EXP_BOUNDS = (88.0, float.fromhex("0x1.62e42ep6"), float.fromhex("-0x1.9d1d9ep6"), float.fromhex("-0x1.9fe368p6"))
TWO_PI = F(2.0) * F(3.14159265358979)

_libm = None


def _m():
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for f in ("logf", "expf"):
            getattr(_libm, f).restype, getattr(_libm, f).argtypes = ctypes.c_float, [ctypes.c_float]
    return _libm


def _each(fn, x):
    x = np.asarray(x, dtype=F)
    return np.array([fn(float(v)) for v in x.reshape(-1)], dtype=F).reshape(x.shape)


def logf(x):
    """The host libm's logf on every word of a float32 array."""
    return _each(_m().logf, x)


def expf(x):
    """The host libm's expf on every word of a float32 array."""
    return _each(_m().expf, x)


def chain(t, axis=-1):
    """0.0f + t[0] + t[1] + ... along axis."""
    t = np.asarray(t, dtype=F)
    shape = list(t.shape)
    shape[axis] = 1
    return np.take(np.cumsum(np.concatenate([np.zeros(shape, F), t], axis=axis), axis=axis, dtype=F), -1, axis=axis)


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


# ---- vexp / vlog -------------------------------------------------------------------------------------------------
def _words(w):
    return np.asarray(w, dtype=np.uint32).view(F)


def vexp_inputs():
    """Every word within 64 of each branch boundary, signed zeros, infinities, NaNs, subnormals, the two inputs on
    which an unfused r differs, and 4096 random words."""
    parts = []
    for b in EXP_BOUNDS:
        w = int(np.asarray(b, dtype=F).view(np.uint32))
        parts.append(_words(np.arange(w - 64, w + 65, dtype=np.int64).astype(np.uint32)))
    parts.append(_words([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 1, 0x80000001,
                         0x007fffff, 0x807fffff, 0x00800000, 0x7f7fffff, 0xff7fffff]))
    parts.append(np.array([float.fromhex("0x1.04845ep+5"), float.fromhex("-0x1.f8cbb2p+5")], dtype=F))
    r = _rng("vexp")
    parts.append(r.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32).view(F))
    parts.append(r.uniform(-104.0, 89.0, 2048).astype(F))
    return np.concatenate(parts)


def vlog_inputs():
    """The classes tools/logf_check.cpp's subject distinguishes (1.0, zeros, infinities, negatives, NaNs, subnormals,
    every table interval and its edges) and 4096 random words."""
    parts = [_words([0x3f800000, 0, 0x80000000, 0x7f800000, 0xff800000, 0xbf800000, 0x7fc00000, 0xffc00000, 1,
                     0x007fffff, 0x00800000, 0x7f7fffff, 0x80000001, 0x3f7fffff, 0x3f800001])]
    edges = 0x3f330000 + (np.arange(0, 17, dtype=np.int64) << 19)
    parts.append(_words(np.concatenate([edges - 1, edges, edges + 1]).astype(np.uint32)))
    r = _rng("vlog")
    parts.append(r.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32).view(F))
    parts.append(np.exp(r.uniform(-87.0, 88.0, 2048)).astype(F))
    return np.concatenate(parts)


# ---- log-domain statistics ---------------------------------------------------------------------------------------
def logdom(func, a, b=None):
    a = np.asarray(a, dtype=F)
    with np.errstate(all="ignore"):
        if func == "entropy":
            return F(-chain(a * logf(a)))
        b = None if b is None else np.asarray(b, dtype=F)
        if func == "kullback_leibler":
            return F(-chain(a * logf(b / a)))
        x = a + b if func == "logsumexp_dot_prod" else a
        mx = x[0]
        for v in x[1:]:
            if v > mx:
                mx = v
        return F(mx + logf(chain(expf(x - mx))))


def logdom_case_names():
    return [f"{k}_{n}" for n in LENGTHS for k in LOGDOM_KINDS]


def logdom_operands(case):
    """(a, b) of a case, the same for the four functions (entropy and logsumexp use a alone)."""
    kind, n = case.rsplit("_", 1)
    n = int(n)
    r = _rng("logdom/" + case)

    def one():
        if kind == "logp":
            return r.uniform(-100.0, 100.0, n).astype(F)
        if kind == "equal":
            return np.full(n, F(r.uniform(0.01, 1.0)), dtype=F)
        v = r.uniform(0.01, 1.0, n)
        return (v / v.sum()).astype(F)
    a, b = one(), one()
    if kind == "zero":
        a[n // 2] = 0.0
    if kind == "nan0":
        a[0] = np.nan
    if kind == "nanmid":
        a[n - 1 if n < 3 else n // 2 + 1] = np.nan
    return a, b


# ---- SVM ---------------------------------------------------------------------------------------------------------
def svm_shapes():
    """(kind, nsv, dim, degree).  (130, 129) is past the 64 KiB the kernels stage in LDS."""
    shapes = [(nsv, 48) for nsv in SVS] + [(5, d) for d in LENGTHS] + [(130, 129)]
    cases = [(k, nsv, dim, 3 if k == "polynomial" else 0) for k in SVM_KINDS for nsv, dim in shapes]
    cases += [("polynomial", nsv, dim, deg) for nsv, dim in ((5, 5), (65, 48)) for deg in DEGREES if deg != 3]
    return cases


def svm_case_name(kind, nsv, dim, degree):
    return f"{kind}_{nsv}x{dim}" + (f"_d{degree}" if kind == "polynomial" else "")


def exponent(x, nb):
    r = x.copy()
    for _ in range(int(nb) - 1):
        r = (r * x).astype(F)
    return r


def svm_sums(kind, m, x):
    """The final sum of every row of x [items, dim]."""
    x = np.asarray(x, dtype=F)
    out = np.empty(x.shape[0], dtype=F)
    sv, dual = m["sv"], m["dual"]
    with np.errstate(all="ignore"):
        for i, v in enumerate(x):
            if kind == "rbf":
                d = v[None, :] - sv
                dot = chain(d * d) if sv.size else np.zeros(sv.shape[0], F)
                f = expf((-m["gamma"]) * dot)
            else:
                dot = chain(v[None, :] * sv) if sv.size else np.zeros(sv.shape[0], F)
                f = dot if kind == "linear" else exponent((m["gamma"] * dot + m["coef0"]).astype(F), m["degree"])
            s = m["intercept"]
            for t in (dual * f).astype(F):
                s = F(s + t)
            out[i] = s
    return out


def svm_classes(m, sums):
    return np.where(sums <= 0, m["classes"][0], m["classes"][1]).astype(np.int32)


def svm_model(kind, nsv, dim, degree, items=ITEMS, seed=""):
    """(model, x): random support vectors and inputs; the intercept is minus the median of the intercept-free sums, so
    each class takes about half of the items."""
    r = _rng(f"svm/{kind}/{nsv}x{dim}/{degree}/{items}{seed}")
    m = {"sv": r.uniform(-1.0, 1.0, (nsv, dim)).astype(F), "dual": r.uniform(-1.0, 1.0, nsv).astype(F),
         "classes": np.array([-3, 7], dtype=np.int32), "intercept": F(0), "degree": np.int32(degree),
         "coef0": F(0.5), "gamma": F(1.0 / max(1, dim)) if kind != "linear" else F(0)}
    x = r.uniform(-1.0, 1.0, (items, dim)).astype(F)
    m["intercept"] = F(-np.median(svm_sums(kind, m, x).astype(np.float64)))
    return m, x


SVM_SPECIAL_INTERCEPTS = np.array([-0.0, 0.0, 1.0, -1.0, np.nan], dtype=F)


def svm_special(kind):
    """(model with 3 support vectors of dimension 4, x [2, 4] whose row 0 holds a NaN)."""
    m, x = svm_model(kind, 3, 4, 2 if kind == "polynomial" else 0, items=2, seed="special")
    x[0, 2] = np.nan
    return m, x


# ---- naive Bayes -------------------------------------------------------------------------------------------------
def bayes_shapes():
    """(classes, dim).  (64, 129) is past the 64 KiB the kernel stages in LDS; (65, 5) takes two rounds of 64 lanes."""
    return [(c, d) for c in CLASSES for d in LENGTHS] + [(7, 48), (64, 129), (65, 5)]


def bayes_case_name(c, d):
    return f"bayes_{c}x{d}"


def bayes_model(c, d, items=ITEMS):
    """(model, x): item i is drawn close to the mean of class i % c."""
    r = _rng(f"bayes/{c}x{d}/{items}")
    theta = np.stack([r.permutation(np.linspace(-3.0, 3.0, c)) for _ in range(d)], axis=1) + r.uniform(-0.1, 0.1, (c, d))
    m = {"theta": theta.astype(F), "sigma": r.uniform(0.05, 0.2, (c, d)).astype(F), "eps": F(1e-3)}
    p = r.uniform(0.5, 1.0, c)
    m["priors"] = (p / p.sum()).astype(F)
    x = (m["theta"][np.arange(items) % c] + r.normal(0.0, 0.02, (items, d))).astype(F)
    return m, x


def bayes_predict(m, x):
    """(the classes' words [items, classes], the index [items])."""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        sigma = (m["sigma"] + m["eps"]).astype(F)
        half1 = (F(-0.5) * chain(logf((TWO_PI * sigma).astype(F)))).astype(F)
        lp = logf(m["priors"])
        d = x[:, None, :] - m["theta"][None, :, :]
        acc2 = chain(((d * d).astype(F) / sigma[None, :, :]).astype(F))
        prob = ((half1[None, :] - (F(0.5) * acc2).astype(F)).astype(F) + lp[None, :]).astype(F)
    idx = np.zeros(x.shape[0], dtype=np.uint32)
    for i, row in enumerate(prob):
        best = row[0]
        for k, v in enumerate(row):
            if best < v:
                best, idx[i] = v, k
    return prob, idx
