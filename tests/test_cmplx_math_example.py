"""examples/fft_bin_example_full.c: the FFT-bin example's unchanged call sequence, arm_cfft_f32 then
arm_cmplx_mag_f32 then arm_max_f32 on host buffers, compiled against include/ and linked to
libcmsisdsp_mi355x.so only.  The input file is the one tests/test_examples.py writes for fft_bin_dropin; the peak
is bin 213."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_build")
LIBDIR = os.path.join(ROOT, "cmsis-dsp_amd", "lib")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "fft_bin_example_full")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "fft_bin_example_full.c"), "-L" + LIBDIR, "-lcmsisdsp_mi355x", "-lm",
                    "-o", exe, "-Wl,-rpath," + LIBDIR], check=True, capture_output=True)
    return exe


def test_example_compiles_and_links():
    assert os.path.exists(build())


@pytest.mark.gpu
def test_example_runs_on_gpu(torch_gpu):
    exe = build()
    x = np.load(os.path.join(ROOT, "tests", "golden", "reference_patterns.npz"))["kat_fftbin_input"]
    inp = os.path.join(OUT, "fftbin_input.f32")
    x.astype(np.float32).tofile(inp)
    r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "SUCCESS 213", r.stdout + r.stderr
