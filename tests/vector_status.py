"""The degenerate calls of the vector and matrix families and what the library answers to them: the case list behind
tests/golden/vector_api_status.json (tools/make_golden_vector_status.py records it, tests/test_gpu_vector_status.py
replays it).

The families are the f32 solves, the basic matrix functions, complex math with max / min, statistics, basic math and
the support functions: every drop-in and its _batch form, named from the FUNCS lists of the *_ref.py modules and
looked up among the library's exported symbols.  A call works on 4 items of 12 words (complex: 6 samples; the
barycenter: 3 vectors of 4 words); matrices are 3 x 4, the solves' triangular and square ones 3 x 3.  Per function:

  null:<x>       each pointer operand null in turn (a matrix: the instance; nulldata:<x>: its pData)
  batch0         batch == 0 (the _batch forms)
  zero:<len>     a length or a matrix dimension of zero
  alias:<d>=<s>  a result that is exactly a source;  offset:<d>=<s>: one source element into it
  overlap:<d>    two results at one address
  stride:<len>   the second source's stride one below the length (the _batch forms that take one)

The alias / offset / overlap rows are left out for the matrix functions and the solves, which have no overlap rule:
they would launch a kernel on racing operands.  Every other row is either refused before any launch or a valid call
on buffers with room to spare.  The batched forms get device pointers; a drop-in gets device pointers as well, and
its alias / offset / overlap rows once more with host pointers (<row>@host), where a partial overlap is staged apart
and is a valid call.

A row records [status, last error set, changed]: the return value (None of a void function; "nan" / "num" of
arm_weighted_average_f32), whether arm_mi355x_last_error() is non-zero afterwards, and the names of the buffers
whose bytes differ from before the call (results start filled with 0x5A).
"""
import ctypes as C

import numpy as np

import basic_math_ref as bm
import cmplx_math_ref as cm
import mat_basic_ref as mb
import mat_solve_ref as ms
import statistics_ref as st
import support_ref as sr

ITEMS, WORDS = 4, 12
SLOT = 1024                     # bytes per buffer: the largest operand is 4 items x 24 words x 4 bytes
DT = dict(bm.MDT, u32=np.uint32)
SOLVE_NAMES = {"inverse": "arm_mat_inverse_f32", "cholesky": "arm_mat_cholesky_f32", "ldlt": "arm_mat_ldlt_f32",
               "solve_lower": "arm_mat_solve_lower_triangular_f32", "solve_upper": "arm_mat_solve_upper_triangular_f32"}


class Model:
    """One function pair: bufs {name: (role, type, words per item)}, insts {name: (rows, cols, buffer)} with symbolic
    dimensions, lens {name: value}, the argument tokens of the drop-in and of the _batch form, and whether the overlap
    rule applies.  Tokens: ("p", buf) ("opt", buf: never null) ("inst", name) ("sinst", class) ("len", name)
    ("stride", len) ("v", value) ("batch",) ("stream",)."""

    def __init__(self, name, bufs, dropin, batch, lens, rule=True, insts=None):
        self.name, self.bufs, self.lens, self.rule, self.insts = name, bufs, lens, rule, insts or {}
        self.forms = {name: dropin, name + "_batch": batch}


P, LEN, V, TAIL = (lambda b: ("p", b)), (lambda k="n": ("len", k)), (lambda v: ("v", v)), [("batch",), ("stream",)]


def _vector(name, bufs, args, n=WORDS, batch_args=None):
    return Model(name, bufs, args, (batch_args or args) + TAIL, {"n": n})


def _basic(func):
    op, t = bm.split(func)
    name = f"arm_{func}"
    a, b, d = ("src", t, WORDS), ("src", t, WORDS), ("dst", t, WORDS)
    one = 0.5 if t == "f32" else 3
    if op == "dot_prod":
        bufs = {"a": a, "b": b, "r": ("dst", bm.DOT_OUT[t], 1)}
        return _vector(name, bufs, [P("a"), P("b"), LEN(), P("r")], batch_args=[P("a"), P("b"), ("stride", "n"), LEN(), P("r")])
    if bm.two_sources(func):
        return _vector(name, {"a": a, "b": b, "d": d}, [P("a"), P("b"), P("d"), LEN()])
    mid = {"offset": [V(one)], "scale": [V(one)] + ([] if t == "f32" else [V(0)]), "shift": [V(1)]}.get(op)
    if mid is not None:
        return _vector(name, {"a": a, "d": d}, [P("a")] + mid + [P("d"), LEN()])
    if op == "clip":
        return _vector(name, {"a": a, "d": d}, [P("a"), P("d"), V(-one), V(one), LEN()])
    return _vector(name, {"a": a, "d": d}, [P("a"), P("d"), LEN()])


def _search(name, t, idx):
    bufs = {"a": ("src", t, WORDS), "r": ("dst", t, 1)}
    if idx:
        bufs["i"] = ("dst", "u32", 1)
    return _vector(name, bufs, [P("a"), LEN(), P("r")] + ([P("i")] if idx else []))


def _cmplx(func):
    name = f"arm_{func}"
    if not func.startswith("cmplx_"):
        return _search(name, func.rsplit("_", 1)[1], True)
    op, t = func[len("cmplx_"):].rsplit("_", 1)
    n = WORDS // 2
    a = ("src", t, WORDS)
    if op == "dot_prod":
        out = ("dst", cm.DOT_OUT[t], 1)
        return _vector(name, {"a": a, "b": a, "re": out, "im": out}, [P("a"), P("b"), LEN(), P("re"), P("im")], n,
                       [P("a"), P("b"), ("stride", "n"), LEN(), P("re"), P("im")])
    if op in ("mult_cmplx", "mult_real"):
        b = ("src", t, WORDS if op == "mult_cmplx" else n)
        return _vector(name, {"a": a, "b": b, "d": ("dst", t, WORDS)}, [P("a"), P("b"), P("d"), LEN()], n)
    return _vector(name, {"a": a, "d": ("dst", t, WORDS if op == "conj" else n)}, [P("a"), P("d"), LEN()], n)


def _stat(func):
    name = f"arm_{func}"
    if func == "cmplx_mag_fast_q15":
        return _vector(name, {"a": ("src", "q15", WORDS), "d": ("dst", "q15", WORDS // 2)}, [P("a"), P("d"), LEN()],
                       WORDS // 2)
    op, t = func.rsplit("_", 1)
    if op in st.SEARCH_IDX or op in st.SEARCH_NO_IDX:
        return _search(name, t, op in st.SEARCH_IDX)
    r = ("dst", st.POWER_OUT[t] if op == "power" else t, 1)
    if op == "mse":
        return _vector(name, {"a": ("src", t, WORDS), "b": ("src", t, WORDS), "r": r}, [P("a"), P("b"), LEN(), P("r")])
    return _vector(name, {"a": ("src", t, WORDS), "r": r}, [P("a"), LEN(), P("r")])


def _support(func, abi):
    name = f"arm_{func}"
    if func in sr.CONVERSIONS or func in sr.COPIES:
        s, d = sr.types(func) if func in sr.CONVERSIONS else (func.rsplit("_", 1)[1],) * 2
        return _vector(name, {"a": ("src", s, WORDS), "d": ("dst", d, WORDS)}, [P("a"), P("d"), LEN()])
    if func in sr.FILLS:
        t = func.rsplit("_", 1)[1]
        return _vector(name, {"d": ("dst", t, WORDS)}, [V(0.5 if t == "f32" else 3), P("d"), LEN()])
    f32 = ("src", "f32", WORDS)
    if func in sr.SORTS:
        inst = abi.arm_sort_instance_f32 if func == "sort_f32" else abi.arm_merge_sort_instance_f32
        return Model(name, {"a": f32, "d": ("dst", "f32", WORDS)}, [("sinst", inst), P("a"), P("d"), LEN()],
                     [P("a"), P("d"), LEN(), V(1)] + TAIL, {"n": WORDS})
    if func == "weighted_average_f32":
        return Model(name, {"a": f32, "w": f32, "r": ("dst", "f32", 1)}, [P("a"), P("w"), LEN()],
                     [P("a"), P("w"), ("stride", "n"), LEN(), P("r")] + TAIL, {"n": WORDS})
    assert func == "barycenter_f32", func
    bufs = {"a": f32, "w": ("src", "f32", 3), "d": ("dst", "f32", 4)}
    return Model(name, bufs, [P("a"), P("w"), P("d"), LEN("nv"), LEN("dim")],
                 [P("a"), P("w"), ("stride", "nv"), P("d"), LEN("nv"), LEN("dim")] + TAIL, {"nv": 3, "dim": 4})


def _mat_basic(func):
    op, t = mb.split(func)
    name = f"arm_mat_{func}"
    I = lambda k: ("inst", k)                                               # noqa: E731
    m = ("src", t, WORDS)
    if op in ("add", "sub"):
        return Model(name, {"a": m, "b": m, "d": ("dst", t, WORDS)}, [I("A"), I("B"), I("D")],
                     [I("A"), I("B"), I("D")] + TAIL, {"R": 3, "C": 4}, False,
                     {"A": ("R", "C", "a"), "B": ("R", "C", "b"), "D": ("R", "C", "d")})
    if op == "scale":
        args = [I("A"), V(0.5 if t == "f32" else 3)] + ([] if t == "f32" else [V(0)]) + [I("D")]
        return Model(name, {"a": m, "d": ("dst", t, WORDS)}, args, args + TAIL, {"R": 3, "C": 4}, False,
                     {"A": ("R", "C", "a"), "D": ("R", "C", "d")})
    if op in ("trans", "cmplx_trans"):
        w = WORDS * (2 if op == "cmplx_trans" else 1)
        return Model(name, {"a": ("src", t, w), "d": ("dst", t, w)}, [I("A"), I("D")], [I("A"), I("D")] + TAIL,
                     {"R": 3, "C": 4}, False, {"A": ("R", "C", "a"), "D": ("C", "R", "d")})
    assert op == "vec_mult", func
    return Model(name, {"a": m, "v": ("src", t, 4), "d": ("dst", t, 3)}, [I("A"), P("v"), P("d")],
                 [I("A"), ("stride", "RC"), P("v"), P("d")] + TAIL, {"R": 3, "C": 4}, False, {"A": ("R", "C", "a")})


def _solve(func):
    name = SOLVE_NAMES[func]
    I = lambda k: ("inst", k)                                               # noqa: E731
    sq, rhs = ("src", "f32", 9), ("src", "f32", WORDS)
    status = ("dst", "q31", 1)
    if func in ("inverse", "cholesky"):
        return Model(name, {"a": sq, "d": ("dst", "f32", 9), "s": status}, [I("A"), I("D")],
                     [I("A"), I("D"), ("batch",), ("opt", "s"), ("stream",)], {"N": 3}, False,
                     {"A": ("N", "N", "a"), "D": ("N", "N", "d")})
    if func == "ldlt":
        bufs = {"a": sq, "l": ("dst", "f32", 9), "d": ("dst", "f32", 9), "pp": ("dst", "u16", 3)}
        args = [I("A"), I("L"), I("D"), P("pp")]
        return Model(name, bufs, args, args + TAIL, {"N": 3}, False,
                     {"A": ("N", "N", "a"), "L": ("N", "N", "l"), "D": ("N", "N", "d")})
    return Model(name, {"t": sq, "a": rhs, "x": ("dst", "f32", WORDS), "s": status}, [I("T"), I("A"), I("X")],
                 [I("T"), I("A"), I("X"), ("batch",), ("opt", "s"), ("stream",)], {"N": 3, "C": 4}, False,
                 {"T": ("N", "N", "t"), "A": ("N", "C", "a"), "X": ("N", "C", "x")})


def models(dsp):
    """Every function pair of the six families, by drop-in name.  The names come from the *_ref.py lists; each must be
    an exported symbol, and together they must be what the ctypes tables of the six families declare."""
    abi = dsp._abi
    out = [_solve(f) for f in ms.FUNCS] + [_mat_basic(f) for f in mb.FUNCS] + [_cmplx(f) for f in cm.FUNCS] + \
        [_stat(f) for f in st.FUNCS] + [_basic(f) for f in bm.FUNCS] + [_support(f, abi) for f in sr.FUNCS]
    names = sorted(n for m in out for n in m.forms)
    assert len(set(names)) == len(names)
    missing = [n for n in names if not hasattr(dsp.lib, n)]
    assert not missing, f"not exported: {missing}"
    declared = set()
    for table in (abi.MAT_SOLVE, abi.MAT_BASIC, abi.CMPLX_MATH, abi.STATISTICS, abi.BASIC_MATH, abi.SUPPORT):
        declared |= set(table)
    declared -= {"arm_sqrt_q15", "arm_sort_init_f32", "arm_merge_sort_init_f32"}    # a scalar and two initialisers
    assert declared == set(names), sorted(declared ^ set(names))
    return {m.name: m for m in out}


def function_names(dsp):
    return sorted(n for m in models(dsp).values() for n in m.forms)


def rows(model, form):
    """The degenerate calls of one form: [(row name, {what to change})]."""
    batch = form.endswith("_batch")
    toks = model.forms[form]
    out = []
    for tok in toks:
        if tok[0] in ("p", "inst", "sinst"):
            key = tok[1] if tok[0] != "sinst" else "S"
            out.append((f"null:{key}", {"null": key}))
            if tok[0] == "inst":
                out.append((f"nulldata:{key}", {"nulldata": key}))
    if batch:
        out.append(("batch0", {"batch": 0}))
    out += [(f"zero:{k}", {"lens": {k: 0}}) for k in model.lens]
    out += [(f"stride:{t[1]}", {"stride": -1}) for t in toks if t[0] == "stride"]
    if model.rule:
        dst = [t[1] for t in toks if t[0] == "p" and model.bufs[t[1]][0] == "dst"]
        src = [t[1] for t in toks if t[0] == "p" and model.bufs[t[1]][0] == "src"]
        pairs = [(f"alias:{d}={s}", {"at": (d, s, 0)}) for d in dst for s in src] + \
            [(f"offset:{d}={s}", {"at": (d, s, 1)}) for d in dst for s in src] + \
            [(f"overlap:{d}", {"at": (d, dst[0], 0)}) for d in dst[1:]]
        out += pairs
        if not batch:
            out += [(n + "@host", dict(c, host=True)) for n, c in pairs]
    return out


def _image(model):
    """The bytes every buffer holds before a call: sources a small repeating pattern, results the marker."""
    names = list(model.bufs)
    img = np.full((len(names), SLOT), 0x5A, dtype=np.uint8)
    for k, name in enumerate(names):
        role, t, words = model.bufs[name]
        if role == "src":
            dt = np.dtype(DT[t])
            v = (np.arange(SLOT // dt.itemsize) % 7 + 1)
            img[k] = (v * 0.125 if t == "f32" else v).astype(dt).view(np.uint8)
    return names, img


def replay(dsp, torch, only=None):
    """{function: {row: [status, last error set, changed buffers]}} of the loaded library."""
    lib = dsp.lib
    out = {}
    for model in models(dsp).values():
        names, img = _image(model)
        dev = torch.empty(img.shape, dtype=torch.uint8, device="cuda:0")
        himg = torch.from_numpy(img)
        host = img.copy()
        for form in model.forms:
            if only and form not in only:
                continue
            fn = getattr(lib, form)
            res = out[form] = {}
            for row, ch in rows(model, form):
                on_host = ch.get("host", False)
                dev.copy_(himg)
                host[:] = img
                base = host.ctypes.data if on_host else dev.data_ptr()
                ptr = {n: base + k * SLOT for k, n in enumerate(names)}
                if "at" in ch:
                    d, s, elems = ch["at"]
                    ptr[d] = ptr[s] + elems * np.dtype(DT[model.bufs[s][1]]).itemsize
                lens = dict(model.lens, **ch.get("lens", {}))
                lens["RC"] = lens.get("R", 0) * lens.get("C", 0)
                keep, args = [], []
                for tok in model.forms[form]:
                    kind = tok[0]
                    if kind in ("p", "opt"):
                        args.append(None if ch.get("null") == tok[1] else ptr[tok[1]])
                    elif kind == "inst":
                        r, c, buf = model.insts[tok[1]]
                        cls = dsp._abi.MAT_INST[model.bufs[buf][1]]
                        m = cls(lens[r], lens[c], None if ch.get("nulldata") == tok[1] else
                                C.cast(ptr[buf], cls._fields_[2][1]))
                        keep.append(m)
                        args.append(None if ch.get("null") == tok[1] else C.byref(m))
                    elif kind == "sinst":
                        s = tok[1](4, 1) if tok[1] is dsp._abi.arm_sort_instance_f32 else tok[1](1, None)
                        keep.append(s)
                        args.append(None if ch.get("null") == "S" else C.byref(s))
                    elif kind == "len":
                        args.append(lens[tok[1]])
                    elif kind == "stride":
                        args.append(lens[tok[1]] + ch.get("stride", 0))
                    elif kind == "v":
                        args.append(tok[1])
                    elif kind == "batch":
                        args.append(ch.get("batch", ITEMS))
                    else:
                        args.append(None)                                   # the stream
                lib.arm_mi355x_clear_error()
                status = fn(*args)
                torch.cuda.synchronize()
                err = lib.arm_mi355x_last_error() != 0
                if isinstance(status, float):
                    status = "nan" if status != status else "num"
                after = host if on_host else dev.cpu().numpy()
                changed = [n for k, n in enumerate(names) if after[k].tobytes() != img[k].tobytes()]
                res[row] = [status, bool(err), changed]
        lib.arm_mi355x_clear_error()
    return out
