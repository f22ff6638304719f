"""GPU: a plain bench.py run and --dump-outputs.  A plain run prints the headline line without
the --full extras (parity, config3, cpu_baseline); two runs with the same arguments write the
same arrays; and the arrays are what W + K alternating forward / inverse launches leave of the
seeded batch, however many clock-settle launches came before."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, STEPS, WARMUP, N = 4096, 3, 2, 1024


def _start(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                             "--warmup", str(WARMUP), "--batch", str(BATCH), "--dump-outputs", out_dir],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_repeatably(dsp, torch_gpu, tmp_path):
    from cmsisdsp_amd import parallel
    torch = torch_gpu
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    procs = [_start(d) for d in dirs]
    outs = [p.communicate(timeout=110) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    lines = [so.splitlines() for so, _ in outs]
    assert all(len(ln) == 1 for ln in lines), lines
    line = json.loads(lines[0][0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert line["full"] is False and line["unit"] == "Gsamples/s" and line["dtype"] == "f32"
    assert not {"parity", "config3", "cpu_baseline"} & set(line)
    assert line["value"] == pytest.approx(BATCH * N / (line["ms_per_step"] * 1e-3) * 1e-9, rel=1e-2)  # both rounded
    assert line["dumped_outputs"] == {"data": [BATCH, 2 * N]}
    a, b = (np.load(os.path.join(d, "data.npy")) for d in dirs)
    assert os.listdir(dirs[0]) == ["data.npy"] and a.dtype == np.float32
    assert a.tobytes() == b.tobytes()

    g = torch.Generator(device="cuda")
    g.manual_seed(parallel.seed_for(0))
    data = (torch.rand(BATCH * 2 * N, generator=g, device="cuda", dtype=torch.float32) - 0.5).view(BATCH, 2 * N)
    S = dsp.const_instance(f"arm_cfft_sR_f32_len{N}")
    for s in range(WARMUP + STEPS):
        dsp.cfft_batch(S, data, s & 1, 1)
    torch.cuda.synchronize()
    assert a.tobytes() == data.cpu().numpy().tobytes()
