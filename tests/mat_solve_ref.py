"""numpy restatement of arm_mat_inverse_f32, arm_mat_cholesky_f32, arm_mat_ldlt_f32 and
arm_mat_solve_{lower,upper}_triangular_f32 (the reference's scalar branches), with the status and the partial
outputs an early return leaves, and the input generators of their tests.

Every operation is one float32 numpy operation, so each result is rounded where the C code rounds it
(contraction off): products before subtractions, `x * y / a` as multiply then divide, `1.0f / sqrtf(x)` as two
operations.  The element updates the reference does one at a time are done a row, a column or a block at a
time, which is exact because they are independent (see each function).

  inverse   Gauss-Jordan on [src | dst] with dst = I.  Column c: the pivot is the first row r >= c that wins the
            ascending scan fabsf(new) > fabsf(cur); swap (src from column c, dst whole rows) when the pivot is
            non-zero and not on the diagonal; a zero pivot returns SINGULAR with both matrices as they stand;
            the pivot row is multiplied by 1.0f / pivot; every other row does x = x - m * p with m = src[r][c]
            read before the row changes.  src is destroyed; its final words are part of the contract.
  cholesky  column i, rows j >= i: g = a[j][i] - sum_k G[i][k] G[j][k] (k ascending, one subtraction per k);
            G[i][i] <= 0 returns DECOMPOSITION_FAILURE with column i unscaled; else column i *= 1 / sqrt(G[i][i]).
            The strict upper triangle of dst is never written.
  solves    per right-hand-side column: tmp = a[i][j] - sum_k t[i][k] x[k][j] (k ascending for lower, descending
            from n - 1 for upper), x[i][j] = tmp / t[i][i].  A zero diagonal returns SINGULAR when it is reached,
            which is in column 0: only that column's earlier rows hold results.
  ldlt      as written, quirks included: see ldlt().
"""
import numpy as np

SUCCESS, SINGULAR, DECOMPOSITION_FAILURE = 0, -5, -7
F32 = np.float32
MARK = np.array([0x5A5A5A5A], dtype=np.uint32).view(np.float32)[0]      # pre-fill of output buffers (1.5e16)
MARK16 = np.uint16(0x5A5A)
FUNCS = ("inverse", "cholesky", "ldlt", "solve_lower", "solve_upper")
SIZES = (1, 2, 3, 4, 5, 8, 17, 33)
FAIL_SIZES = (2, 5, 17)


def marked(shape):
    return np.full(shape, MARK, dtype=np.float32)


def inverse(src):
    """-> (status, src after the call, dst)."""
    s = np.array(src, dtype=np.float32)
    n = s.shape[0]
    d = np.eye(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(n):
            sel, piv = c, s[c, c]
            for r in range(c + 1, n):
                if np.abs(s[r, c]) > np.abs(piv):
                    sel, piv = r, s[r, c]
            if piv == 0:
                return SINGULAR, s, d
            if sel != c:
                s[[c, sel], c:] = s[[sel, c], c:]
                d[[c, sel], :] = d[[sel, c], :]
            ip = F32(1.0) / piv
            s[c, c:] = s[c, c:] * ip
            d[c, :] = d[c, :] * ip
            m = s[:, c].copy()
            rows = np.arange(n) != c
            s[rows, c:] = s[rows, c:] - m[rows, None] * s[c, c:][None, :]
            d[rows, :] = d[rows, :] - m[rows, None] * d[c, :][None, :]
    # the reference's all-zero check after the loop cannot fire: the scaled diagonal is never 0
    return SUCCESS, s, d


def cholesky(src, dst=None):
    """-> (status, dst).  dst: the buffer's words before the call (default: MARK); pass src for the in-place
    alias."""
    a = np.array(src, dtype=np.float32)
    n = a.shape[0]
    g = marked((n, n)) if dst is None else np.array(dst, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            v = a[i:, i].copy()
            for k in range(i):
                v = v - g[i, k] * g[i:, k]
            g[i:, i] = v
            if g[i, i] <= 0:
                return DECOMPOSITION_FAILURE, g
            g[i:, i] = g[i:, i] * (F32(1.0) / np.sqrt(g[i, i]))
    return SUCCESS, g


def solve(t, a, lower, dst=None):
    """-> (status, dst).  t [n, n], a [n, cols]; dst: the buffer's words before the call (default: MARK)."""
    t = np.asarray(t, dtype=np.float32)
    a = np.array(a, dtype=np.float32)
    n, cols = a.shape
    x = marked((n, cols)) if dst is None else np.array(dst, dtype=np.float32)
    order = list(range(n)) if lower else list(range(n - 1, -1, -1))
    zero = [i for i in order if t[i, i] == 0]
    status = SUCCESS
    if zero:
        status, order, cols = SINGULAR, order[:order.index(zero[0])], min(cols, 1)
    with np.errstate(all="ignore"):
        for pos, i in enumerate(order):
            tmp = a[i, :cols].copy()
            for k in order[:pos]:
                tmp = tmp - t[i, k] * x[k, :cols]
            x[i, :cols] = tmp / t[i, i]
    return status, x


def ldlt(src):
    """-> (status, l, d, pp).  Pivot j: the first diagonal index >= k holding the strictly largest value above
    -FLT_MAX; rows then columns k, j swapped over the whole matrix; pp[k] = j; the loop stops at
    fabsf(a) < 1.0e-8f; trailing update A[w][x] = A[w][x] - A[w][k] * A[x][k] / a (reads column k only, which it
    does not write), then column k is divided by a.  Rank deficient: columns >= k zeroed and diag = k - 1 (so
    the last completed column keeps its pivot on l's diagonal).  The strict upper triangle is zeroed, d holds
    the first diag diagonal entries, l's get 1.0.  Always SUCCESS."""
    A = np.array(src, dtype=np.float32)
    n = A.shape[0]
    d = np.zeros((n, n), dtype=np.float32)
    pp = np.arange(n, dtype=np.uint16)
    full, k = True, 0
    with np.errstate(all="ignore"):
        for k in range(n):
            m, j = -np.finfo(np.float32).max, k
            for r in range(k, n):
                if A[r, r] > m:
                    m, j = A[r, r], r
            if j != k:
                A[[k, j], :] = A[[j, k], :]
                A[:, [k, j]] = A[:, [j, k]]
            pp[k] = j
            a = A[k, k]
            if np.abs(a) < F32(1.0e-8):
                full = False
                break
            col = A[k + 1:, k].copy()
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - (col[:, None] * col[None, :]) / a
            A[k + 1:, k] = col / a
        else:
            k = n
    diag = k
    if not full:
        diag -= 1
        A[:, k:] = 0
    A[np.triu_indices(n, 1)] = 0
    for i in range(max(diag, 0)):
        d[i, i] = A[i, i]
        A[i, i] = 1
    return SUCCESS, A, d, pp


# ------------------------------------------------------------------ inputs
def fill(kind, n, rng):
    """One n x n float32 matrix: uniform [-1, 1); mixed: exponents 2^-20 .. 2^20 with +-0 entries (forces pivot
    swaps); spd: B B^T with B n x (n + 3); tiny_spd: spd * 2^-130 (subnormal entries and products); rank: B B^T
    with B n x max(1, n / 2); lower / upper: triangular, off-diagonal [-1, 1), 1 <= |diag| < 2."""
    if kind == "uniform":
        return rng.uniform(-1, 1, (n, n)).astype(np.float32)
    if kind == "mixed":
        v = rng.uniform(0.5, 1.0, (n, n)) * rng.choice([-1.0, 1.0], (n, n)) * 2.0 ** rng.integers(-20, 21, (n, n))
        z = rng.uniform(0, 1, (n, n))
        v[z < 0.1] = 0.0
        v[(z >= 0.1) & (z < 0.2)] = -0.0
        return v.astype(np.float32)
    if kind in ("spd", "tiny_spd", "rank"):
        b = rng.uniform(-1, 1, (n, max(1, n // 2) if kind == "rank" else n + 3)).astype(np.float32)
        m = (b.astype(np.float64) @ b.astype(np.float64).T)
        return (m * 2.0 ** -130 if kind == "tiny_spd" else m).astype(np.float32)
    if kind in ("lower", "upper"):
        m = rng.uniform(-1, 1, (n, n))
        m = np.tril(m, -1) if kind == "lower" else np.triu(m, 1)
        m[np.arange(n), np.arange(n)] = rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)
        return m.astype(np.float32)
    raise ValueError(kind)


def rhs(n, cols, rng):
    return rng.uniform(-1, 1, (n, cols)).astype(np.float32)


def failing(func, which, n, rng):
    """Inputs whose failure is structural (exact zeros), so it does not depend on rounding.
    inverse: zero_first / zero_last (a zero column); cholesky: neg_diag (spd with entry n/2 of the diagonal
    negated); ldlt: zeros, rank; solves: zero_diag (entry n/2 of the diagonal zero)."""
    if func == "inverse":
        m = fill("uniform", n, rng)
        m[:, 0 if which == "zero_first" else n - 1] = 0
        return m
    if func == "cholesky":
        m = fill("spd", n, rng)
        m[n // 2, n // 2] = -m[n // 2, n // 2]
        return m
    if func == "ldlt":
        return np.zeros((n, n), dtype=np.float32) if which == "zeros" else fill("rank", n, rng)
    m = fill("lower" if func == "solve_lower" else "upper", n, rng)
    m[n // 2, n // 2] = 0
    return m


FILLS = {"inverse": ("uniform", "mixed", "spd"), "cholesky": ("spd", "tiny_spd"), "ldlt": ("spd", "tiny_spd")}
FAILS = {"inverse": ("zero_first", "zero_last"), "cholesky": ("neg_diag",), "ldlt": ("zeros", "rank"),
         "solve_lower": ("zero_diag",), "solve_upper": ("zero_diag",)}


def nonfinite(func, rng):
    """n = 5 with one +Inf and one NaN entry (inverse: uniform; cholesky: spd, both below the diagonal in
    columns 1 and 2 so that the decomposition meets them)."""
    m = fill("uniform" if func == "inverse" else "spd", 5, rng)
    m[3, 1], m[4, 2] = np.inf, np.nan
    return m


def case_names(func):
    """Every fixture case of func, in the order tools/make_golden_mat_solve.py writes them."""
    names = []
    if func in FILLS:
        names += [f"{f}_{n}" for f in FILLS[func] for n in SIZES]
        names.append(("uniform" if func == "inverse" else "spd") + "_64")
    else:
        names += [f"uniform_{n}x{c}" for n in SIZES for c in sorted({1, 3, n})]
        names.append("uniform_64x3")
    names += [f"{w}_{n}" + ("x3" if func.startswith("solve") else "") for w in FAILS[func] for n in FAIL_SIZES]
    if func in ("inverse", "cholesky"):
        names.append("nonfinite_5")
    if func == "cholesky":
        names += ["alias_spd_17", "alias_neg_diag_5"]
    if func.startswith("solve"):
        names += ["alias_uniform_17x3", "alias_zero_diag_5x3"]
    return names


def run(func, g, alias=False):
    """The restatement on a fixture's operands -> dict of the output arrays and status."""
    if func == "inverse":
        st, s, d = inverse(g["src"])
        return {"status": st, "src_after": s, "dst": d}
    if func == "cholesky":
        st, d = cholesky(g["src"], g["src"] if alias else None)
        return {"status": st, "dst": d}
    if func == "ldlt":
        st, l, d, pp = ldlt(g["src"])
        return {"status": st, "l": l, "d": d, "pp": pp}
    st, x = solve(g["t"], g["a"], func == "solve_lower", g["a"] if alias else None)
    return {"status": st, "dst": x}


def same_words(got, want, nan_positions=False):
    """Bit equality; nan_positions: the project's f32 rule for non-finite inputs (tests/test_f32_classes.py):
    non-NaN words bit-equal, NaNs at the same positions."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not nan_positions or got.dtype != np.float32:
        return got.tobytes() == want.tobytes()
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all()) and got.view(np.uint32)[~gn].tobytes() == want.view(np.uint32)[~wn].tobytes()
