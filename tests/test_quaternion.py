"""arm_quaternion_{norm,inverse,conjugate,normalize,product,product_single}_f32, arm_quaternion2rotation_f32 and
arm_rotation2quaternion_f32, each as a drop-in and (product_single excepted) as a _batch form
(cmsis-dsp_amd/csrc/quaternion.hip).

The checker is committed data: tests/golden/quaternion.npz holds the reference's own outputs
(tools/make_golden_quaternion.py); tests/quaternion_ref.py restates the functions in numpy, and the generator asserted
it against the reference item by item.  Every comparison is bit-exact; NaN results are compared by position
(f32_classes.assert_same_words).  Every item is independent of its neighbours, so the expected words of any selection
of the stored operands are the same selection of the stored outputs: the GPU tests select `n` items cyclically from the
first special one on (the zero quaternion, NaNs; the trace of exactly 0, NaNs on the diagonal), which for the counts
past the stored ones tiles the set.

CPU: the fixture index with the branch balance, the restatement against every fixture, the exported symbols, the Python
names.  GPU: all eight functions at 1, 3, 64, 65 and 4099 quaternions, bStride 0 and 4, marker bytes around every
output, the sources unchanged, every operand one element off 16-byte alignment, in place, the drop-ins on host and on
device pointers, every refusal writing nothing, one call per kernel with 65,535 * 64 + 2 items, one stream-order check
and one chain on device tensors with no host copy in between."""
import json
import os
import subprocess

import numpy as np
import pytest

import quaternion_ref as qr
from cmsisdsp_amd import _abi
from devbuf import Dev, marker, untouched
from f32_classes import assert_same_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "quaternion.npz"))
IDX = json.loads(str(GOLD["index"]))
F = np.float32
SUCCESS, ARGUMENT_ERROR = 0, -1
COUNTS = (1, 3, 64, 65, 4099)
BIG = 65535 * 64 + 2                      # blocks of 256 items: past 65,535 * 64 + 1 items a 16-bit grid dimension fails
OPS = qr.FUNCS + ("product", "product_shared")
SYMBOLS = [f"arm_{f}_f32" for f in qr.FUNCS] + ["arm_quaternion_product_f32"]


@pytest.fixture(autouse=True)
def no_stale_error(dsp):
    """The last error is per thread and outlives a test: start every test here without one."""
    dsp.lib.arm_mi355x_clear_error()


def words(op):
    return (4, 4) if op.startswith("product") else qr.WORDS[op]


def select(op, n):
    """-> (a [n, wa], b or None, the reference's words [n, wd]) for n items taken cyclically from the first special
    one on."""
    wa, wd = words(op)
    src = qr.rotations(IDX["rotation_seed"]) if wa == 9 else qr.quaternions("a")
    first = qr.RANDOM_R + 64 if wa == 9 else qr.RANDOM_Q
    pick = (first + np.arange(n)) % src.shape[0]
    out = GOLD[f"{op}/out"].reshape(src.shape[0], wd)[pick]
    b = None
    if op == "product":
        b = qr.quaternions("b")[pick]
    elif op == "product_shared":
        b = qr.quaternions("b")[0]
    return src[pick], b, out


# ------------------------------------------------------------------ CPU
def test_fixture_index_is_complete():
    assert IDX["funcs"] == list(qr.FUNCS) and set(qr.WORDS) == set(_abi.QUATERNION_FUNCS) == set(qr.FUNCS)
    assert all(qr.WORDS[f] == _abi.QUATERNION_FUNCS[f] for f in qr.FUNCS)
    qa, rot = qr.quaternions("a"), qr.rotations(IDX["rotation_seed"])
    assert IDX["quaternions"] == qa.shape[0] >= 65 and IDX["rotations"] == rot.shape[0] >= 65
    for op in OPS:
        wa, wd = words(op)
        assert GOLD[f"{op}/out"].shape == ((rot if wa == 9 else qa).shape[0] * wd,), op
    assert (qa[qr.RANDOM_Q] == 0).all() and np.isnan(qa[qr.RANDOM_Q:]).any()       # the zero quaternion, NaNs
    assert np.isnan(GOLD["quaternion_inverse/out"].reshape(-1, 4)[qr.RANDOM_Q]).all()      # it divides by 0
    assert np.isnan(GOLD["quaternion_normalize/out"].reshape(-1, 4)[qr.RANDOM_Q]).all()
    counts = np.bincount(GOLD["branch"], minlength=4)                             # the balance condition
    assert counts.sum() == rot.shape[0] and (counts * 8 >= rot.shape[0]).all(), counts
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "quaternion.npz")) < 64 << 10


def test_restatement_equals_every_fixture():
    qa, qb, rot = qr.quaternions("a"), qr.quaternions("b"), qr.rotations(IDX["rotation_seed"])
    assert [qr.crc(qa), qr.crc(qb), qr.crc(rot)] == GOLD["crc"].tolist()
    for f in qr.FUNCS:
        src = rot if qr.WORDS[f][0] == 9 else qa
        assert_same_words(qr.apply(f, src).reshape(-1), GOLD[f"{f}/out"], f)
    assert_same_words(qr.product(qa, qb).reshape(-1), GOLD["product/out"], "product")
    assert_same_words(qr.product(qa, qb[0]).reshape(-1), GOLD["product_shared/out"], "product_shared")
    assert np.array_equal(qr.branch(rot), GOLD["branch"])


def test_probed_facts_hold_in_the_fixtures():
    rot = qr.rotations(IDX["rotation_seed"])
    special = rot[qr.RANDOM_R + 64:]
    br = GOLD["branch"][qr.RANDOM_R + 64:]
    trace0 = [i for i, r in enumerate(special) if not np.isnan(r).any() and r[0] + r[4] + r[8] == 0]
    assert trace0 and all(br[i] != 0 for i in trace0)       # a trace of exactly 0 goes on to the second test
    assert any(br[i] == 1 for i in trace0)
    allnan = [i for i, r in enumerate(special) if np.isnan(r).all()]
    assert allnan and all(br[i] == 3 for i in allnan)       # a NaN trace with no true comparison ends in the last branch
    q = GOLD["rotation2quaternion/out"].reshape(-1, 4)
    assert q[qr.RANDOM_R + 64].tolist() == [1.0, 0.0, 0.0, 0.0]                 # the identity


def test_library_exports_the_symbols(dsp):
    names = SYMBOLS + [s + "_batch" for s in SYMBOLS] + ["arm_quaternion_product_single_f32"]
    assert len(set(names)) == 15 and set(names) == set(_abi.QUATERNION)
    out = subprocess.run(["nm", "-D", "--defined-only", dsp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(names) <= exported
    for header, batch in (("arm_math.h", False), ("arm_math_mi355x.h", True)):
        text = open(os.path.join(ROOT, "include", header)).read()
        for n in names:
            if n.endswith("_batch") == batch:
                assert f" {n}(" in text, (header, n)


def test_python_names_exist(dsp):
    import cmsisdsp as d
    for n in SYMBOLS + ["arm_quaternion_product_single_f32"]:
        assert "cmsis_" + n in getattr(d, n).__doc__, n
    assert not hasattr(d, "arm_quaternion_norm_f16")
    for n in ("arm_quaternion_f32", "arm_quaternion_product_f32", "quaternion_batch", "quaternion_product_batch"):
        assert callable(getattr(dsp, n)), n


# ------------------------------------------------------------------ GPU
def batch_call(dsp, torch, op, a, b, n, offs=(0, 0, 0), b_stride=None, out=None):
    """arm_<op>_f32_batch on device copies -> (status, the result or the untouched marker, the sources afterwards)."""
    wa, wd = words(op)
    da = Dev(torch, a, offs[0])
    dd = Dev(torch, marker((n, wd), F) if out is None else out, offs[1])
    st = torch.cuda.current_stream().cuda_stream
    if op.startswith("product"):
        db = Dev(torch, b, offs[2])
        if b_stride is None:
            b_stride = 4 if op == "product" else 0
        status = dsp.lib.arm_quaternion_product_f32_batch(da.ptr, db.ptr, b_stride, dd.ptr, n, st)
    else:
        db = None
        status = getattr(dsp.lib, f"arm_{op}_f32_batch")(da.ptr, dd.ptr, n, st)
    torch.cuda.synchronize()
    return status, dd.get(), (da.get(), None if db is None else db.get())


def same_bytes(x, y):
    return np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_batch_equals_the_reference(dsp, torch_gpu, op):
    for n in COUNTS:
        a, b, want = select(op, n)
        status, got, (a1, b1) = batch_call(dsp, torch_gpu, op, a, b, n)
        assert status == SUCCESS, (op, n)
        assert_same_words(got, want, f"{op} n={n}")
        assert same_bytes(a1, a) and (b is None or same_bytes(b1, b)), (op, n, "a source changed")


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_batch_one_element_off_alignment(dsp, torch_gpu, op):
    a, b, want = select(op, 65)
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 2, 1)):
        status, got, (a1, b1) = batch_call(dsp, torch_gpu, op, a, b, 65, offs)
        assert status == SUCCESS, (op, offs)
        assert_same_words(got, want, f"{op} offs={offs}")
        assert same_bytes(a1, a), (op, offs)


@pytest.mark.gpu
def test_batch_in_place(dsp, torch_gpu):
    torch = torch_gpu
    st = torch.cuda.current_stream().cuda_stream
    for op in ("quaternion_inverse", "quaternion_conjugate", "quaternion_normalize", "product", "product_shared"):
        a, b, want = select(op, 65)
        for off in (0, 1):
            d = Dev(torch, a, off)
            if op.startswith("product"):
                db = Dev(torch, b)
                status = dsp.lib.arm_quaternion_product_f32_batch(d.ptr, db.ptr, 4 if op == "product" else 0, d.ptr,
                                                                  65, st)
            else:
                status = getattr(dsp.lib, f"arm_{op}_f32_batch")(d.ptr, d.ptr, 65, st)
            torch.cuda.synchronize()
            assert status == SUCCESS, op
            assert_same_words(d.get(), want, f"{op} in place")
    a, b, want = select("product", 65)                       # the result over the second factor
    da, d = Dev(torch, a), Dev(torch, b)
    assert dsp.lib.arm_quaternion_product_f32_batch(da.ptr, d.ptr, 4, d.ptr, 65, st) == SUCCESS
    torch.cuda.synchronize()
    assert_same_words(d.get(), want, "product over b")


@pytest.mark.gpu
def test_drop_ins_on_host_and_device_pointers(dsp, torch_gpu):
    torch = torch_gpu
    import cmsisdsp as d
    for op in qr.FUNCS:
        a, _, want = select(op, 65)
        assert_same_words(getattr(d, f"arm_{op}_f32")(a.reshape(-1)).reshape(want.shape), want, op)
        wa, wd = words(op)
        da, dd = Dev(torch, a, 1), Dev(torch, marker((65, wd), F), 1)
        getattr(dsp.lib, f"arm_{op}_f32")(da.ptr, dd.ptr, 65)          # synchronous: no synchronize() here
        assert dsp.last_error()[0] == 0
        assert_same_words(dd.get(), want, op + " on device pointers")
        assert same_bytes(da.get(), a)
    a, b, want = select("product", 65)
    assert_same_words(d.arm_quaternion_product_f32(a.reshape(-1), b.reshape(-1)).reshape(-1, 4), want, "product")
    assert_same_words(d.arm_quaternion_product_single_f32(a[3], b[3]), want[3], "product_single")
    x = a.copy()                                             # in place on host memory
    dsp.lib.arm_quaternion_conjugate_f32(x.ctypes.data, x.ctypes.data, 65)
    assert dsp.last_error()[0] == 0
    assert_same_words(x, select("quaternion_conjugate", 65)[2], "conjugate in place on the host")
    out = marker((65, 4), F)
    dsp.lib.arm_quaternion_norm_f32(a.ctypes.data, out.ctypes.data, 0)           # nbQuaternions == 0
    assert dsp.last_error()[0] == 0 and untouched(out)


@pytest.mark.gpu
def test_refusals_write_nothing(dsp, torch_gpu):
    torch = torch_gpu
    lib = dsp.lib
    st = torch.cuda.current_stream().cuda_stream
    for op in OPS:
        a, b, _ = select(op, 65)
        wa, wd = words(op)
        if op.startswith("product"):
            for stride in (1, 3, 8, 65):
                status, got, _ = batch_call(dsp, torch, op, a, qr.quaternions("b")[:65], 65, b_stride=stride)
                assert status == ARGUMENT_ERROR and untouched(got), (op, stride)
            da, db, dd = Dev(torch, a), Dev(torch, qr.quaternions("b")[:65]), Dev(torch, marker((65, 4), F))
            for pa, pb, pd in ((None, db.ptr, dd.ptr), (da.ptr, None, dd.ptr), (da.ptr, db.ptr, None)):
                assert lib.arm_quaternion_product_f32_batch(pa, pb, 4, pd, 65, st) == ARGUMENT_ERROR, op
            assert lib.arm_quaternion_product_f32_batch(None, None, 4, None, 0, st) == SUCCESS       # an empty call
        else:
            da, dd = Dev(torch, a), Dev(torch, marker((65, wd), F))
            fn = getattr(lib, f"arm_{op}_f32_batch")
            assert fn(None, dd.ptr, 65, st) == ARGUMENT_ERROR and fn(da.ptr, None, 65, st) == ARGUMENT_ERROR, op
            assert fn(None, None, 0, st) == SUCCESS and fn(da.ptr, dd.ptr, 0, st) == SUCCESS, op
        torch.cuda.synchronize()
        assert untouched(dd.get()) and same_bytes(da.get(), a), op
        assert dsp.last_error()[0] == 0, op                  # these refusals are a status, not a last error
        # a result that overlaps a source without being it: one buffer, the result one item further on
        both = Dev(torch, np.concatenate([a.reshape(-1), np.zeros(wa + wd * 65, F)]))
        before = both.get().copy()
        dst = both.ptr + 4 * wa
        if op.startswith("product"):
            status = lib.arm_quaternion_product_f32_batch(both.ptr, db.ptr, 4, dst, 65, st)
            status2 = lib.arm_quaternion_product_f32_batch(da.ptr, both.ptr, 4, dst, 65, st)
        else:
            status = status2 = getattr(lib, f"arm_{op}_f32_batch")(both.ptr, dst, 65, st)
        torch.cuda.synchronize()
        assert status == status2 == ARGUMENT_ERROR and same_bytes(both.get(), before), (op, "overlap")
        assert dsp.last_error()[0] != 0, op                  # the overlap refusal is recorded, as in every family
        lib.arm_mi355x_clear_error()
    # the drop-ins are void: a refusal is the last error
    a, _, _ = select("quaternion_norm", 4)
    out = marker((4,), F)
    lib.arm_quaternion_norm_f32(None, out.ctypes.data, 4)
    assert dsp.last_error()[0] != 0 and untouched(out)
    lib.arm_mi355x_clear_error()
    x = np.concatenate([a.reshape(-1), marker((4,), F)])
    before = x.copy()
    lib.arm_quaternion_inverse_f32(x.ctypes.data, x.ctypes.data + 4, 4)           # overlapping host buffers are staged
    assert dsp.last_error()[0] == 0                                               # apart: the reference's words
    assert_same_words(x[1:17], qr.inverse(before[:16]).reshape(-1), "inverse, overlapping host buffers")
    lib.arm_mi355x_clear_error()


@pytest.mark.gpu
@pytest.mark.parametrize("op", ("quaternion_norm", "quaternion_inverse", "quaternion_conjugate", "quaternion_normalize",
                                "product", "quaternion2rotation", "rotation2quaternion"))
def test_batch_past_a_16_bit_grid(dsp, torch_gpu, op):
    """One call per kernel (product and product_shared are one) with more items than 65,535 blocks of 64 hold."""
    torch = torch_gpu
    wa, wd = words(op)
    a, b, want = select(op, 4099)
    reps = -(-BIG // 4099)
    big = lambda x: np.tile(x, (reps, 1))[:BIG]              # noqa: E731
    ta = torch.from_numpy(big(a)).cuda()
    out = torch.full((BIG + 8, wd), float("nan"), dtype=torch.float32, device="cuda")
    if op == "product":
        tb = torch.from_numpy(big(b)).cuda()
        dsp.quaternion_product_batch(ta, tb, out[:BIG])
    else:
        dsp.quaternion_batch(op, ta, out[:BIG])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[BIG:]).all(), "words past the end"
    assert_same_words(got[:BIG], big(want), op)


@pytest.mark.gpu
def test_source_written_on_the_calls_stream(dsp, torch_gpu):
    """The sources hold other valid words until the call's own stream, behind a device-side delay, writes the true
    ones immediately before the call; work on any other stream, or a host read, would see the stale words."""
    torch = torch_gpu
    rot, _, want_q = select("rotation2quaternion", 4099)
    qa, qb, want_p = select("product_shared", 4099)
    true_r, true_a, true_b = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (rot, qa, qb))
    r = torch.from_numpy(np.roll(rot, 1, axis=0).copy()).cuda()
    a = torch.from_numpy(np.roll(qa, 1, axis=0).copy()).cuda()
    b = torch.from_numpy(qr.quaternions("b")[1].copy()).cuda()
    out_q = torch.full((4099, 4), float("nan"), dtype=torch.float32, device="cuda")
    out_p = torch.full((4099, 4), float("nan"), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(40_000_000)
        r.copy_(true_r)
        a.copy_(true_a)
        b.copy_(true_b)
        dsp.quaternion_batch("rotation2quaternion", r, out_q, stream=side)
        dsp.quaternion_product_batch(a, b, out_p, stream=side)
        busy = not side.query()
    side.synchronize()
    assert busy, "the delay ended before the calls were enqueued: the check showed nothing"
    assert_same_words(out_q.cpu().numpy(), want_q, "rotation2quaternion")
    assert_same_words(out_p.cpu().numpy(), want_p, "product with one shared quaternion")
    assert not qr.same_word(qr.from_rotation(np.roll(rot, 1, axis=0)), want_q)   # the stale words give another result
