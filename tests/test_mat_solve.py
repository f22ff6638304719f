"""arm_mat_inverse_f32, arm_mat_cholesky_f32, arm_mat_ldlt_f32, arm_mat_solve_{lower,upper}_triangular_f32 and
their batched forms.

The checker is committed data: tests/golden/mat_solve.npz holds the reference's own outputs, every output buffer
pre-filled with a marker word so the words a call leaves alone show (tools/make_golden_mat_solve.py);
tests/mat_solve_ref.py restates the five functions in numpy, failures and partial outputs included.
CPU: the fixture index is complete, the restatement equals the fixtures bit for bit, the failing inputs fail as
the issue states, the outputs solve their problem against float64, symbols and names exist.
GPU: everything is bit-exact, no tolerance: the drop-ins against every fixture (host and device pointers,
failures, in-place aliases), the batched forms against the restatement on every path (several items per
workgroup, one item per workgroup in LDS up to the switch point, one item in global memory past it, failing
items next to good ones in one workgroup, misaligned pData, NULL status, empty batch).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mat_solve_ref as mr
from cmsisdsp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "mat_solve.npz"))
INDEX = json.loads(str(GOLD["index"]))
FUNCS = list(mr.FUNCS)
DROPIN = {"inverse": "arm_mat_inverse_f32", "cholesky": "arm_mat_cholesky_f32", "ldlt": "arm_mat_ldlt_f32",
          "solve_lower": "arm_mat_solve_lower_triangular_f32", "solve_upper": "arm_mat_solve_upper_triangular_f32"}
SYMBOLS = list(DROPIN.values()) + [s + "_batch" for s in DROPIN.values()]
OUTPUTS = {"inverse": ("src_after", "dst"), "cholesky": ("dst",), "ldlt": ("l", "d", "pp"), "solve_lower": ("dst",),
           "solve_upper": ("dst",)}
# The largest n whose item fits the 160 KiB of LDS (cmsis-dsp_amd/csrc/kernels.hpp kMatSolveLds): the inverse
# holds [src | dst], 2 n^2 words (2 * 143^2 * 4 = 163,592 B; 144: 165,888 B); Cholesky and LDLT hold n rows of
# n | 1 words plus two words per item (201: 161,628 B; 202: 164,048 B).  One past it runs in global memory.
LDS_MAX_N = {"inverse": 143, "cholesky": 201, "ldlt": 201}
LDS_BYTES = 160 * 1024


def cases_of(func):
    return [c for f, c in INDEX if f == func]


def gold(func, case):
    k = f"{func}/{case}/"
    return {n[len(k):]: GOLD[n] for n in GOLD.files if n.startswith(k)}


def is_alias(case):
    return case.startswith("alias_")


def check_outputs(func, case, got, want):
    """Status equal; every output word bit-equal (nonfinite cases: the f32 rule, NaNs at the same positions)."""
    assert int(got["status"]) == int(want["status"]), (func, case, int(got["status"]), int(want["status"]))
    for k in OUTPUTS[func]:
        assert mr.same_words(got[k], want[k], case.startswith("nonfinite")), \
            (func, case, k, int((np.asarray(got[k]).view(np.uint8) != np.asarray(want[k]).view(np.uint8)).sum()))


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert {f for f, _ in INDEX} == set(FUNCS)
    for func in FUNCS:
        assert cases_of(func) == mr.case_names(func), func
        for case in cases_of(func):
            g = gold(func, case)
            assert g["status"].dtype == np.int32
            if func.startswith("solve"):
                n, cols = g["a"].shape
                assert g["t"].shape == (n, n) and g["dst"].shape == (n, cols) and g["dst"].dtype == np.float32
            else:
                n = g["src"].shape[0]
                assert g["src"].shape == (n, n) and g["src"].dtype == np.float32
                for k in OUTPUTS[func]:
                    assert g[k].shape == ((n,) if k == "pp" else (n, n)), (func, case, k)
                if func == "ldlt":
                    assert g["pp"].dtype == np.uint16


@pytest.mark.parametrize("func", FUNCS)
def test_restatement_equals_fixtures(func):
    for case in cases_of(func):
        g = gold(func, case)
        check_outputs(func, case, mr.run(func, g, is_alias(case)), g)


def test_fixture_statuses_and_untouched_words():
    """-5 for the singular inverse and the zero-diagonal solves, -7 for Cholesky, 0 for LDLT at rank 0 and 1
    too; and what a failure leaves: the marker in dst wherever the reference did not write."""
    mark = np.uint32(0x5A5A5A5A)
    for func in FUNCS:
        for case in cases_of(func):
            g, st = gold(func, case), int(gold(func, case)["status"])
            kind = case[len("alias_"):] if is_alias(case) else case
            fails = kind.startswith(mr.FAILS[func])
            if func == "ldlt":
                assert st == 0, case
            elif not kind.startswith(("nonfinite", "tiny")):
                assert st == {"inverse": -5, "cholesky": -7}.get(func, -5) if fails else st == 0, (func, case)
            if is_alias(case):
                continue
            if func == "cholesky":
                n = g["src"].shape[0]
                assert (g["dst"].view(np.uint32)[np.triu_indices(n, 1)] == mark).all(), case
                if fails:
                    bad = n // 2
                    assert (g["dst"].view(np.uint32)[:, bad + 1:] == mark).all(), case
                    assert g["dst"][bad, bad] <= 0, case                       # the unscaled diagonal
            if func.startswith("solve") and fails:
                n, z = g["a"].shape[0], g["a"].shape[0] // 2
                w = g["dst"].view(np.uint32)
                assert (w[:, 1:] == mark).all(), case
                rows = slice(z, n) if func == "solve_lower" else slice(0, z + 1)
                assert (w[rows, 0] == mark).all() and (w[:, 0] != mark).sum() == (z if func == "solve_lower" else n - 1 - z)
    g = gold("ldlt", "zeros_5")                 # rank 0: nothing but pp[0] = 0
    assert not g["l"].any() and not g["d"].any() and (g["pp"] == np.arange(5)).all()
    # rank 1 at n = 2: the 1.0e-8f cut is absolute, and the second pivot is rounding residue that may pass it
    # (it does here), so all that is fixed is the status, a unit lower-triangular l and a diagonal d
    g = gold("ldlt", "rank_2")
    assert g["l"][0, 1] == 0 and g["d"][0, 1] == 0 and g["d"][1, 0] == 0 and g["d"][0, 0] > 0
    stops = [c for c in cases_of("ldlt") if c.startswith("rank_") and not gold("ldlt", c)["d"][-1, -1]]
    assert stops, "no rank-deficient case stops early"


U = 2.0 ** -24


def residual_ratio(func, g, out):
    """max |residual| / (n u max(|factors| product)) in float64, u = 2^-24: the backward-error scale of an
    n-term f32 dot product."""
    f8 = lambda x: np.asarray(x, dtype=np.float64)      # noqa: E731
    a = f8(g["src"])
    n = a.shape[0]
    if func == "inverse":
        x = f8(out["dst"])
        res, scale = a @ x - np.eye(n), np.abs(a) @ np.abs(x)
    elif func == "cholesky":
        gg = np.tril(f8(out["dst"]))
        res, scale = gg @ gg.T - a, np.abs(gg) @ np.abs(gg.T)
    else:
        perm = np.arange(n)
        for k, j in enumerate(out["pp"]):
            perm[[k, j]] = perm[[j, k]]
        l, d = f8(out["l"]), f8(out["d"])
        res, scale = a[perm][:, perm] - l @ d @ l.T, np.abs(l) @ np.abs(d) @ np.abs(l.T)
    return float(np.max(np.abs(res)) / (n * U * np.max(scale)))


# twice the largest ratio of the reference's own fixture words (measured: see the docstring below)
RESIDUAL_BOUND = {"inverse": 2 * 0.50, "cholesky": 2 * 2.18, "ldlt": 2 * 0.20}


@pytest.mark.parametrize("func", ["inverse", "cholesky", "ldlt"])
def test_outputs_solve_their_problem_in_float64(func):
    """A A^-1 ~ I, G G^T ~ A and P A P^T ~ L D L^T on the successful uniform / spd cases, as
    max |residual| <= bound * n 2^-24 max(|A||A^-1|) (|G||G^T|, |L||D||L^T|).  The bound is not assumed: it is
    twice the largest ratio the reference's own fixture words reach, which is 0.499 for the inverse (uniform_1:
    two roundings on one word), 2.173 for Cholesky (spd_1: a * (1 / sqrt(a)) squared, three roundings against
    n = 1; 0.58 from n = 2 on) and 0.198 for LDLT (spd_2); the ratios fall as n grows (below 0.1 at n = 64).
    The restatement's words are held to it."""
    worst = 0.0
    for case in cases_of(func):
        g = gold(func, case)
        if not case.startswith(("uniform_", "spd_")) or int(g["status"]) != 0:
            continue
        r_ref = residual_ratio(func, g, g)
        r = residual_ratio(func, g, mr.run(func, g))
        worst = max(worst, r_ref)
        assert r <= RESIDUAL_BOUND[func], (case, r)
    print(f"{func}: largest fixture ratio {worst:.3f}")
    assert worst <= RESIDUAL_BOUND[func] / 2 * 1.001        # the recorded figure is the fixtures' own


def test_library_exports_mat_solve_symbols(dsp):
    assert len(set(SYMBOLS)) == 10 and set(SYMBOLS) == set(_abi.MAT_SOLVE)
    for n in SYMBOLS:
        assert callable(getattr(dsp.lib, n)), n
    for n in ("arm_mat_inverse", "arm_mat_cholesky", "arm_mat_ldlt", "arm_mat_solve_lower_triangular",
              "arm_mat_solve_upper_triangular", "mat_inverse_batch", "mat_cholesky_batch", "mat_ldlt_batch",
              "mat_solve_triangular_batch"):
        assert callable(getattr(dsp, n)), n


def test_cmsisdsp_module_exposes_mat_solve_names():
    import cmsisdsp as d
    for n in DROPIN.values():
        assert callable(getattr(d, n)), n


def test_struct_mirrors_unchanged():
    f = _abi.arm_matrix_instance_f32
    assert [x[0] for x in f._fields_] == ["numRows", "numCols", "pData"]
    assert (f.numRows.offset, f.numCols.offset, f.pData.offset, C.sizeof(f)) == (0, 2, 8, 16)


def test_lds_switch_points():
    """The sizes named above are the largest that fit, by the byte counts the launcher uses."""
    inv = lambda n: 4 * (((n * n + 3) & ~3) + n * n)            # noqa: E731
    pad = lambda n: 4 * (n * (n | 1) + 2) + 16                  # noqa: E731
    assert inv(LDS_MAX_N["inverse"]) <= LDS_BYTES < inv(LDS_MAX_N["inverse"] + 1)
    for f in ("cholesky", "ldlt"):
        assert pad(LDS_MAX_N[f]) <= LDS_BYTES < pad(LDS_MAX_N[f] + 1)


# ------------------------------------------------------------------ GPU: drop-in against the fixtures
def dropin(dsp, torch, func, g, where, alias=False):
    """The drop-in on host numpy arrays or device tensors, outputs pre-filled with the marker (alias: dst is
    the source buffer itself) -> the dict mat_solve_ref.run returns."""
    if where == "host":
        put, addr, words = (lambda x: x.copy()), (lambda t: t.ctypes.data), (lambda t: t)
    else:
        put, addr, words = (lambda x: torch.from_numpy(x.copy()).cuda()), (lambda t: t.data_ptr()), \
            (lambda t: t.cpu().numpy())

    def inst(t, shape):
        return _abi.arm_matrix_instance_f32(shape[0], shape[1], C.cast(addr(t), _abi.c_f32p))

    fn = getattr(dsp.lib, DROPIN[func])
    if func.startswith("solve"):
        t, a = put(g["t"]), put(g["a"])
        x = a if alias else put(mr.marked(g["a"].shape))
        st = fn(C.byref(inst(t, g["t"].shape)), C.byref(inst(a, g["a"].shape)), C.byref(inst(x, g["a"].shape)))
        out = {"dst": words(x)}
        assert words(t).tobytes() == g["t"].tobytes()
    else:
        shape = g["src"].shape
        s = put(g["src"])
        if func == "ldlt":
            l, d = put(mr.marked(shape)), put(mr.marked(shape))
            pp = put(np.full(shape[0], mr.MARK16, dtype=np.uint16).view(np.int16))
            st = fn(C.byref(inst(s, shape)), C.byref(inst(l, shape)), C.byref(inst(d, shape)), addr(pp))
            out = {"l": words(l), "d": words(d), "pp": words(pp).view(np.uint16)}
            assert words(s).tobytes() == g["src"].tobytes()
        else:
            d = s if alias else put(mr.marked(shape))
            st = fn(C.byref(inst(s, shape)), C.byref(inst(d, shape)))
            out = {"dst": words(d)}
            if func == "inverse":
                out["src_after"] = words(s)
            elif not alias:
                assert words(s).tobytes() == g["src"].tobytes()
    dsp._check_void(DROPIN[func])
    out["status"] = st
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("func", FUNCS)
def test_dropin_equals_fixtures(dsp, torch_gpu, func, where):
    """Every fixture: the successful cases, the failures with their untouched marker words, the in-place
    aliases and the non-finite case."""
    for case in cases_of(func):
        g = gold(func, case)
        check_outputs(func, case, dropin(dsp, torch_gpu, func, g, where, is_alias(case)), g)


@pytest.mark.gpu
def test_dropin_mixed_pointers(dsp, torch_gpu):
    """Host source with device destination and the reverse."""
    torch = torch_gpu
    g = gold("cholesky", "spd_17")
    for dev_src in (False, True):
        s, d = g["src"].copy(), mr.marked(g["src"].shape)
        ts, td = torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()
        S = _abi.arm_matrix_instance_f32(17, 17, C.cast(ts.data_ptr() if dev_src else s.ctypes.data, _abi.c_f32p))
        D = _abi.arm_matrix_instance_f32(17, 17, C.cast(d.ctypes.data if dev_src else td.data_ptr(), _abi.c_f32p))
        assert dsp.lib.arm_mat_cholesky_f32(C.byref(S), C.byref(D)) == 0
        dsp._check_void("arm_mat_cholesky_f32")
        assert (d if dev_src else td.cpu().numpy()).tobytes() == g["dst"].tobytes()


# ------------------------------------------------------------------ GPU: batched against the restatement
def make_items(func, n, batch, rng, fill=None, cols=3, fail=()):
    """Operands of `batch` items [(dict as a fixture's)]; the items in `fail` get the failing input."""
    items = []
    for i in range(batch):
        if func.startswith("solve"):
            t = mr.failing(func, "zero_diag", n, rng) if i in fail else mr.fill(func[len("solve_"):], n, rng)
            items.append({"t": t, "a": mr.rhs(n, cols, rng)})
        elif i in fail:
            items.append({"src": mr.failing(func, mr.FAILS[func][i % len(mr.FAILS[func])], n, rng)})
        else:
            items.append({"src": mr.fill(fill or ("uniform" if func == "inverse" else "spd"), n, rng)})
    return items


def offset_tensor(torch, x, off):
    """A device copy of x whose first word sits `off` elements past an allocation's (aligned) start."""
    buf = torch.zeros(x.size + off, dtype=torch.from_numpy(x).dtype, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    return view


def run_batch(dsp, torch, func, items, off=0, status=None):
    """The batched entry point on the stacked items, outputs pre-filled with the marker -> list of dicts."""
    dev = lambda x: offset_tensor(torch, np.ascontiguousarray(x), off)        # noqa: E731
    batch = len(items)
    if func.startswith("solve"):
        t, a = dev(np.stack([g["t"] for g in items])), dev(np.stack([g["a"] for g in items]))
        x = dev(mr.marked(a.shape))
        st = dsp.mat_solve_triangular_batch(t, a, x, lower=func == "solve_lower", status=status)
        outs = {"dst": x.cpu().numpy()}
    else:
        s = dev(np.stack([g["src"] for g in items]))
        if func == "ldlt":
            l, d = dev(mr.marked(s.shape)), dev(mr.marked(s.shape))
            pp = dev(np.full(s.shape[:2], mr.MARK16, dtype=np.uint16).view(np.int16))
            dsp.mat_ldlt_batch(s, l, d, pp)
            st = torch.zeros(batch, dtype=torch.int32)
            outs = {"l": l.cpu().numpy(), "d": d.cpu().numpy(), "pp": pp.cpu().numpy().view(np.uint16)}
        else:
            d = dev(mr.marked(s.shape))
            st = (dsp.mat_inverse_batch if func == "inverse" else dsp.mat_cholesky_batch)(s, d, status=status)
            outs = {"dst": d.cpu().numpy()}
            if func == "inverse":
                outs["src_after"] = s.cpu().numpy()
    st = np.zeros(batch, dtype=np.int32) if st is None else st.cpu().numpy()
    return [{**{k: v[i] for k, v in outs.items()}, "status": st[i]} for i in range(batch)]


def check_batch(func, items, got, label):
    for i, (g, o) in enumerate(zip(items, got)):
        check_outputs(func, f"{label} item {i}", o, mr.run(func, g))


# n x batch: several items per workgroup with a ragged last workgroup (257), n that is no power of two and no
# multiple of 4 (scalar staging), one item per workgroup at 64; fills: mixed forces pivot swaps in the inverse,
# rank stops LDLT early
SMALL = [(1, 257), (3, 257), (4, 257), (8, 257), (17, 9), (33, 9), (64, 3)]
BATCH_CASES = [(f, n, b, fill) for f in FUNCS for n, b in SMALL
               for fill in {"inverse": ("uniform", "mixed"), "ldlt": ("spd", "rank")}.get(f, (None,))
               if not (fill == "mixed" and n > 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("func,n,batch,fill", BATCH_CASES, ids=[f"{f}-{n}x{b}-{x}" for f, n, b, x in BATCH_CASES])
def test_batch_equals_restatement(dsp, torch_gpu, func, n, batch, fill):
    rng = np.random.default_rng([n, batch, FUNCS.index(func), len(fill or "")])
    items = make_items(func, n, batch, rng, fill, cols=3 if n != 8 else 8)
    check_batch(func, items, run_batch(dsp, torch_gpu, func, items), f"{func} {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 300])
@pytest.mark.parametrize("func", ["solve_lower", "solve_upper"])
def test_solve_batch_single_and_many_columns(dsp, torch_gpu, func, cols):
    """One right-hand side per item (one lane per item), and more columns than a workgroup has lanes."""
    rng = np.random.default_rng([cols, FUNCS.index(func)])
    items = make_items(func, 9, 5, rng, cols=cols)
    check_batch(func, items, run_batch(dsp, torch_gpu, func, items), func)


# One item at the largest n of the LDS path, and one past it on the global-memory path (LDS_MAX_N).  The
# solves keep x in LDS up to n = 64 (mat_solve.hip kSolveLdsMaxN; 64 is among the batched sizes above) and
# read it back from global memory from 65 on.
EDGE = [("inverse", 143), ("inverse", 150), ("cholesky", 201), ("cholesky", 210), ("ldlt", 201), ("ldlt", 210),
        ("solve_lower", 65), ("solve_upper", 65), ("solve_lower", 150), ("solve_upper", 150)]


@pytest.mark.gpu
@pytest.mark.parametrize("func,n", EDGE, ids=[f"{f}-{n}" for f, n in EDGE])
def test_batch_at_the_lds_switch_point(dsp, torch_gpu, func, n):
    assert func.startswith("solve") or n in (LDS_MAX_N[func], 150 if func == "inverse" else 210)
    rng = np.random.default_rng([n, FUNCS.index(func)])
    items = make_items(func, n, 2 if n == 65 else 1, rng)
    check_batch(func, items, run_batch(dsp, torch_gpu, func, items), f"{func} {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_global_memory_path_fails_like_the_reference(dsp, torch_gpu, func):
    """Past the LDS sizes, two items of which the first fails: status, partial outputs and the neighbour."""
    n = 150 if func in ("inverse", "solve_lower", "solve_upper") else 210
    rng = np.random.default_rng([n, 2, FUNCS.index(func)])
    items = make_items(func, n, 2, rng, fail=(0,))
    got = run_batch(dsp, torch_gpu, func, items)
    check_batch(func, items, got, f"{func} {n}")
    if func != "ldlt":
        assert [int(o["status"]) for o in got] == [-7 if func == "cholesky" else -5, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("func", FUNCS)
def test_failing_items_share_a_workgroup_with_good_ones(dsp, torch_gpu, func):
    """n = 4, 130 items, items 0, 5 and 64 fail: a workgroup holds 32 (inverse) or 64 (Cholesky, LDLT) items,
    so 0 and 5 fail next to good items of their workgroup and 64 in another.  Every neighbour bit-exact, the
    failing items' partial outputs as the reference leaves them, one status per item."""
    fail = (0, 5, 64)
    rng = np.random.default_rng([4, 130, FUNCS.index(func)])
    items = make_items(func, 4, 130, rng, fail=fail)
    got = run_batch(dsp, torch_gpu, func, items)
    check_batch(func, items, got, func)
    st = np.array([int(o["status"]) for o in got])
    if func == "ldlt":
        assert not st.any()
        # items 0 and 64 are all zero (rank 0); item 5 has rank 2, where the cut depends on rounding residue
        assert all(not got[i]["d"].any() for i in (0, 64)) and all(got[i]["d"][3, 3] for i in (1, 4, 6, 63, 65, 129))
    else:
        bad = -7 if func == "cholesky" else -5
        assert (st[list(fail)] == bad).all() and (np.delete(st, fail) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,batch", [(8, 5), (33, 3)])
@pytest.mark.parametrize("func", FUNCS)
def test_batch_pdata_offset_by_one_element(dsp, torch_gpu, func, n, batch):
    """pData one element past a 16-B aligned address: the staging drops to 4-B accesses."""
    rng = np.random.default_rng([n, batch, 1, FUNCS.index(func)])
    items = make_items(func, n, batch, rng)
    check_batch(func, items, run_batch(dsp, torch_gpu, func, items, off=1), func)


@pytest.mark.gpu
@pytest.mark.parametrize("func", ["inverse", "cholesky", "solve_lower", "solve_upper"])
def test_batch_null_status(dsp, torch_gpu, func):
    rng = np.random.default_rng([5, FUNCS.index(func)])
    items = make_items(func, 5, 7, rng, fail=(2,))
    got = run_batch(dsp, torch_gpu, func, items, status=False)
    for o in got:
        o["status"] = 0
    for i, (g, o) in enumerate(zip(items, got)):
        want = mr.run(func, g)
        want["status"] = 0
        check_outputs(func, f"item {i}", o, want)


@pytest.mark.gpu
@pytest.mark.parametrize("func", ["cholesky", "solve_lower", "solve_upper"])
def test_batch_aliases(dsp, torch_gpu, func):
    """Cholesky into its source and a solve into its right-hand side, batched."""
    torch = torch_gpu
    rng = np.random.default_rng([6, FUNCS.index(func)])
    items = make_items(func, 6, 40, rng, fail=(3,))
    if func == "cholesky":
        s = torch.from_numpy(np.stack([g["src"] for g in items])).cuda()
        st = dsp.mat_cholesky_batch(s, s)
        out = s.cpu().numpy()
    else:
        t = torch.from_numpy(np.stack([g["t"] for g in items])).cuda()
        a = torch.from_numpy(np.stack([g["a"] for g in items])).cuda()
        st = dsp.mat_solve_triangular_batch(t, a, a, lower=func == "solve_lower")
        out = a.cpu().numpy()
    st = st.cpu().numpy()
    for i, g in enumerate(items):
        check_outputs(func, f"item {i}", {"dst": out[i], "status": st[i]}, mr.run(func, g, alias=True))


@pytest.mark.gpu
def test_empty_batch_zero_size_and_size_mismatch(dsp, torch_gpu):
    torch = torch_gpu
    F = _abi.arm_matrix_instance_f32
    buf = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    stat = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    pp = torch.full((16,), 3, dtype=torch.int16, device="cuda")
    p, ps, none = C.cast(buf.data_ptr(), _abi.c_f32p), C.c_void_p(stat.data_ptr()), C.c_void_p(None)

    def m(r, c):
        return C.byref(F(r, c, p))

    lib, ok, mism = dsp.lib, dsp.ARM_MATH_SUCCESS, dsp.ARM_MATH_SIZE_MISMATCH
    for batch, n in ((0, 4), (3, 0)):                                       # successful no-ops
        assert lib.arm_mat_inverse_f32_batch(m(n, n), m(n, n), batch, ps, none) == ok
        assert lib.arm_mat_cholesky_f32_batch(m(n, n), m(n, n), batch, ps, none) == ok
        assert lib.arm_mat_ldlt_f32_batch(m(n, n), m(n, n), m(n, n), C.c_void_p(pp.data_ptr()), batch, none) == ok
        assert lib.arm_mat_solve_lower_triangular_f32_batch(m(n, n), m(n, 2), m(n, 2), batch, ps, none) == ok
        assert lib.arm_mat_solve_upper_triangular_f32_batch(m(n, n), m(n, 2), m(n, 2), batch, ps, none) == ok
    for f in (lib.arm_mat_inverse_f32, lib.arm_mat_cholesky_f32):
        assert f(m(3, 4), m(3, 4)) == mism and f(m(3, 3), m(4, 4)) == mism
    assert lib.arm_mat_inverse_f32_batch(m(3, 4), m(3, 4), 1, ps, none) == mism
    assert lib.arm_mat_cholesky_f32_batch(m(3, 3), m(4, 4), 1, ps, none) == mism
    assert lib.arm_mat_ldlt_f32(m(3, 3), m(3, 3), m(4, 4), C.c_void_p(pp.data_ptr())) == mism
    assert lib.arm_mat_ldlt_f32_batch(m(3, 4), m(3, 3), m(3, 3), C.c_void_p(pp.data_ptr()), 1, none) == mism
    for f, fb in ((lib.arm_mat_solve_lower_triangular_f32, lib.arm_mat_solve_lower_triangular_f32_batch),
                  (lib.arm_mat_solve_upper_triangular_f32, lib.arm_mat_solve_upper_triangular_f32_batch)):
        for shapes in (((3, 4), (3, 2), (3, 2)), ((3, 3), (4, 2), (4, 2)), ((3, 3), (3, 2), (3, 1)),
                       ((3, 3), (3, 2), (4, 2))):
            args = [m(*s) for s in shapes]
            assert f(*args) == mism and fb(*args, 1, ps, none) == mism, shapes
    assert lib.arm_mat_inverse_f32(None, m(3, 3)) == dsp.ARM_MATH_ARGUMENT_ERROR
    assert lib.arm_mat_ldlt_f32(m(3, 3), m(3, 3), m(3, 3), None) == dsp.ARM_MATH_ARGUMENT_ERROR
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 7).all() and (stat.cpu().numpy() == 9).all() and (pp.cpu().numpy() == 3).all()


# ------------------------------------------------------------------ GPU: cmsisdsp
@pytest.mark.gpu
def test_cmsisdsp_module_mat_solve(torch_gpu):
    """The reference wrapper's shapes: (status, dst), (status, l, d, perm); Cholesky's dst zero-filled before
    the call; the caller's arrays are never modified."""
    import cmsisdsp as d
    g = gold("inverse", "mixed_8")
    src = g["src"].copy()
    st, inv = d.arm_mat_inverse_f32(src)
    assert st == 0 and inv.tobytes() == g["dst"].tobytes() and src.tobytes() == g["src"].tobytes()
    st, inv = d.arm_mat_inverse_f32(gold("inverse", "zero_last_5")["src"])
    assert st == -5 and inv.tobytes() == gold("inverse", "zero_last_5")["dst"].tobytes()
    for case in ("spd_17", "neg_diag_5"):
        g = gold("cholesky", case)
        st, ch = d.arm_mat_cholesky_f32(g["src"])
        want = np.where(g["dst"].view(np.uint32) == 0x5A5A5A5A, np.float32(0), g["dst"])
        assert st == int(g["status"]) and ch.tobytes() == want.tobytes(), case
    for case in ("spd_8", "rank_5"):
        g = gold("ldlt", case)
        st, l, dd, perm = d.arm_mat_ldlt_f32(g["src"])
        assert st == 0 and l.tobytes() == g["l"].tobytes() and dd.tobytes() == g["d"].tobytes()
        assert perm.dtype == np.int16 and perm.tobytes() == g["pp"].tobytes()
    for func in ("solve_lower", "solve_upper"):
        g = gold(func, "uniform_17x3")
        st, x = getattr(d, DROPIN[func])(g["t"], g["a"])
        assert st == 0 and x.shape == (17, 3) and x.tobytes() == g["dst"].tobytes()
