"""examples/least_squares_dropin.c: X = inv(A^T A) A^T B with arm_mat_trans_f32, arm_mat_mult_f32 and
arm_mat_inverse_f32 on host buffers, compiled against include/ and linked to libcmsisdsp_mi355x.so only.

The operands are 16 x 4 and 16 x 3, built from a seed with the singular values of A in [1, 2], so cond2(A) <= 2.
X must agree with the float64 least-squares solution within BOUND = 8 m cond2(A)^2 2^-24 = 2^-15 (m = 16 rows)
in relative max-norm: forming A^T A squares the condition number, and each of the three products adds at most
its inner dimension (<= m) times 2^-24."""
import os
import subprocess

import numpy as np
import pytest

import mat_solve_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_build")
LIBDIR = os.path.join(ROOT, "cmsis-dsp_amd", "lib")
M, N, P = 16, 4, 3
BOUND = 8 * M * 2.0 ** 2 * 2.0 ** -24


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "least_squares_dropin")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "least_squares_dropin.c"), "-L" + LIBDIR, "-lcmsisdsp_mi355x", "-lm",
                    "-o", exe, "-Wl,-rpath," + LIBDIR], check=True, capture_output=True)
    return exe


def operands(seed=31):
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((M, N)))
    v, _ = np.linalg.qr(rng.standard_normal((N, N)))
    s = np.concatenate(([1.0, 2.0], rng.uniform(1.0, 2.0, N - 2)))
    a = ((u * s) @ v.T).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, (M, P)).astype(np.float32)
    sv = np.linalg.svd(a.astype(np.float64), compute_uv=False)
    assert 0.999 <= sv[-1] and sv[0] <= 2.001
    return a, b


def rel_error(x, a, b):
    want = np.linalg.lstsq(a.astype(np.float64), b.astype(np.float64), rcond=None)[0]
    return float(np.abs(x.astype(np.float64) - want).max() / np.abs(want).max())


def test_example_compiles_and_links():
    assert os.path.exists(build())


def test_restatement_chain_is_inside_the_bound(oracle):
    """numpy transpose, the stated k-ordered fmaf-chain product (oracle.mat_mult_fmaf) and mat_solve_ref's
    inverse: the words the example is expected to write.  Recorded: the chain's error is 1.21e-7, BOUND is
    3.05e-5 (2^-15), a margin of about 250."""
    a, b = operands()
    at = np.ascontiguousarray(a.T)
    ata = oracle.mat_mult_fmaf(at, a)[1]
    st, _, inv = mr.inverse(ata)
    assert st == 0
    x = oracle.mat_mult_fmaf(oracle.mat_mult_fmaf(inv, at)[1], b)[1]
    err = rel_error(x, a, b)
    print(f"restatement chain: relative max-norm error {err:.3e}, bound {BOUND:.3e}")
    assert err <= BOUND


@pytest.mark.gpu
def test_example_runs_on_gpu(torch_gpu, oracle):
    exe = build()
    a, b = operands()
    inp, res = os.path.join(OUT, "least_squares_in.bin"), os.path.join(OUT, "least_squares_out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([M, N, P], dtype=np.uint32).tobytes() + a.tobytes() + b.tobytes())
    if os.path.exists(res):
        os.remove(res)
    r = subprocess.run([exe, inp, res], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"OK {M} {N} {P}", r.stdout + r.stderr
    w = np.fromfile(res, dtype=np.float32)
    sizes = [N * M, N * N, N * N, N * M, N * P]
    assert w.size == sum(sizes)
    at, ata, inv, pinv, x = (p.reshape(s) for p, s in zip(np.split(w, np.cumsum(sizes)[:-1]),
                                                           [(N, M), (N, N), (N, N), (N, M), (N, P)]))
    assert at.tobytes() == np.ascontiguousarray(a.T).tobytes()
    err = rel_error(x, a, b)
    print(f"example: relative max-norm error {err:.3e}, bound {BOUND:.3e}")
    assert err <= BOUND
    # every step equals the stated semantics of the three calls, bit for bit
    assert ata.tobytes() == oracle.mat_mult_fmaf(at, a)[1].tobytes()
    assert inv.tobytes() == mr.inverse(ata)[2].tobytes()
    assert pinv.tobytes() == oracle.mat_mult_fmaf(inv, at)[1].tobytes()
    assert x.tobytes() == oracle.mat_mult_fmaf(pinv, b)[1].tobytes()
