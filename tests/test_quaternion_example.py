"""examples/quaternion_example.c: normalize, norm, the products, inverse, conjugate and the two rotation conversions on
host buffers through the C ABI, compiled against include/ and linked to libcmsisdsp_mi355x.so only; the program checks
its results and prints SUCCESS."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_build")
LIBDIR = os.path.join(ROOT, "cmsis-dsp_amd", "lib")


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "quaternion_example")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "quaternion_example.c"), "-L" + LIBDIR, "-lcmsisdsp_mi355x", "-lm",
                    "-o", exe, "-Wl,-rpath," + LIBDIR], check=True, capture_output=True)
    return exe


def test_example_compiles_and_links():
    assert os.path.exists(build())


@pytest.mark.gpu
def test_example_runs_on_gpu(torch_gpu):
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("SUCCESS"), r.stdout + r.stderr
    assert "FAILURE" not in r.stdout and len(r.stdout.strip().splitlines()) == 6
