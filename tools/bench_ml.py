#!/usr/bin/env python3
"""Throughput of vexp / vlog, the log-domain statistics, the SVMs and naive Bayes on one GPU.

    python tools/bench_ml.py [ew|logdom|svm|bayes ...] [--gib G] [--window MS]

Timing is tools/bench_cmplx.py's: a clock-settle phase, then REPEATS windows of about --window ms between HIP events;
a line reports the best window, the repeat spread and the fraction of the 8 TB/s HBM peak its algorithmic bytes reach.

  ew      arm_vexp_f32_batch / arm_vlog_f32_batch over G GiB (default 1) of source words (read once, written once),
          next to arm_mat_add_f32_batch on the same tensor in the same run.
  logdom  entropy, kullback_leibler, logsumexp, logsumexp_dot_prod at item lengths 64 and 1024, G GiB of source words
          per call, each next to arm_dot_prod_f32_batch on the same tensors in the same run.
  svm     the three SVMs at (130 support vectors, dimension 48) and (1024, 64), 2^17 and 2^14 items, next to a torch
          formulation of the same decision function on the same tensors (matmul / cdist, exp, matmul: a comparison, not
          a bar, since its sums are not ordered).
  bayes   7 and 64 classes at dimension 48, 2^17 items, next to a torch formulation (broadcast, sum, argmax).
  ref [--ref DIR]   (alone, no GPU) the reference's scalar predict functions on one CPU thread, the same shapes.

The first and last item of every result are checked bit for bit against tests/ml_ref.py first."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ml_ref as mr  # noqa: E402

SVM_SHAPES = ((130, 48, 1 << 17), (1024, 64, 1 << 14))
BAYES_SHAPES = ((7, 48, 1 << 17), (64, 48, 1 << 17))


def gpu_modules():
    global torch, bc, dsp
    import torch
    import bench_cmplx as bc
    import cmsisdsp_amd as dsp


def emit(workload, n, batch, ok, ms, steps, nbytes, **extra):
    best = min(ms)
    line = {"workload": workload, "n": n, "batch": batch, "bitexact_first_last": ok,
            "value": round(batch / (best * 1e-3) * 1e-6, 4), "unit": "M items/s",
            "ms": [round(k, 4) for k in ms], "spread": round((max(ms) - best) / best, 4), "steps": steps,
            "roofline": {"bound": "hbm", "bytes": nbytes, "peak_TBps": bc.HBM_TBPS,
                         "frac": round(nbytes / (best * 1e-3) / (bc.HBM_TBPS * 1e12), 4)}}
    line.update(extra)
    line["version"] = dsp.version()
    print(json.dumps(line), flush=True)


def run_ew(gib):
    ok_all = True
    n = 1024
    batch = max(1, int(gib * 2 ** 30 / (4 * n)))
    gen = torch.Generator(device="cuda").manual_seed(29)
    src = torch.rand((batch, n), generator=gen, device="cuda", dtype=torch.float32) * 170.0 - 85.0
    dst = torch.zeros_like(src)
    third = torch.zeros_like(src)
    for name, x, fn in (("vexp", src, mr.expf), ("vlog", src.abs() + 1e-30, mr.logf)):
        x = x.contiguous()
        ours = lambda: dsp.fast_math_batch(name, x, dst)                            # noqa: E731
        ours()
        torch.cuda.synchronize()
        ok = all(mr.same_word(dst[i].cpu().numpy(), fn(x[i].cpu().numpy())) for i in (0, batch - 1))
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        line = {}
        bc.yardstick(line, "yardstick", "arm_mat_add_f32_batch, same tensors (three streams)",
                     lambda: dsp.mat_add_batch(x.view(batch, 32, 32), dst.view(batch, 32, 32), third.view(batch, 32, 32)),
                     min(ms))
        line["yardstick"]["frac"] = round(12 * n * batch / (min(line["yardstick"]["ms"]) * 1e-3) / (bc.HBM_TBPS * 1e12), 4)
        emit(f"{name}_f32", n, batch, ok, ms, steps, 8 * n * batch, **line)
    return ok_all


def run_logdom(gib):
    ok_all = True
    gen = torch.Generator(device="cuda").manual_seed(31)
    for n in (64, 1024):
        batch = max(1, int(gib * 2 ** 30 / (8 * n)))
        a = torch.rand((batch, n), generator=gen, device="cuda", dtype=torch.float32) + 0.01
        b = torch.rand((batch, n), generator=gen, device="cuda", dtype=torch.float32) + 0.01
        res = torch.zeros(batch, dtype=torch.float32, device="cuda")
        yname, yf = "arm_dot_prod_f32_batch, same tensors", lambda: dsp.dot_prod_batch(a, b, res)   # noqa: E731
        for func in mr.LOGDOM_FUNCS:
            two = func in ("kullback_leibler", "logsumexp_dot_prod")
            ours = lambda: dsp.logdom_batch(func, a, b if two else None, res)      # noqa: E731
            ours()
            torch.cuda.synchronize()
            ok = all(mr.same_word(res[i].cpu().numpy(), mr.logdom(func, a[i].cpu().numpy(), b[i].cpu().numpy()))
                     for i in (0, batch - 1))
            ok_all = ok_all and ok
            ms, steps = bc.measure(ours)
            line = {}
            bc.yardstick(line, "yardstick", yname, yf, min(ms))
            emit(f"{func}_f32", n, batch, ok, ms, steps, (8 if two else 4) * n * batch, **line)
        del a, b
    return ok_all


def torch_svm(kind, m, x):
    if kind == "rbf":
        f = torch.exp(-m["gamma"] * torch.cdist(x, m["sv"]) ** 2)
    else:
        f = x @ m["sv"].T
        if kind == "polynomial":
            f = (m["gamma"] * f + m["coef0"]) ** m["degree"]
    return f @ m["dual"] + m["intercept"]


def run_svm(_gib):
    ok_all = True
    for nsv, dim, items in SVM_SHAPES:
        for kind in mr.SVM_KINDS:
            m, _ = mr.svm_model(kind, nsv, dim, 3 if kind == "polynomial" else 0, items=64)
            gen = torch.Generator(device="cuda").manual_seed(37)
            x = torch.rand((items, dim), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1
            t = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and v.ndim else v)
                 for k, v in m.items()}
            S, keep = dsp.svm_instance(kind, m["intercept"], t["dual"], t["sv"], t["classes"], int(m["degree"]),
                                       float(m["coef0"]), float(m["gamma"]))
            res = torch.zeros(items, dtype=torch.int32, device="cuda")
            dec = torch.zeros(items, dtype=torch.float32, device="cuda")
            ours = lambda: dsp.svm_predict_batch(kind, S, x, res, dec)              # noqa: E731
            ours()
            torch.cuda.synchronize()
            ends = x[[0, items - 1]].cpu().numpy()
            ok = mr.same_word(dec[[0, items - 1]].cpu().numpy(), mr.svm_sums(kind, m, ends))
            ok_all = ok_all and ok
            ms, steps = bc.measure(ours)
            tm = {"sv": t["sv"], "dual": t["dual"], "gamma": float(m["gamma"]), "coef0": float(m["coef0"]),
                  "degree": int(m["degree"]), "intercept": float(m["intercept"])}
            line = {"flops_per_item": (3 if kind == "rbf" else 2) * nsv * dim,
                    "Gflops": round((3 if kind == "rbf" else 2) * nsv * dim * items / (min(ms) * 1e-3) * 1e-9, 1),
                    "model_in_lds": nsv * (dim | 1) + nsv <= 16384}
            bc.yardstick(line, "torch", "torch formulation (unordered sums), same tensors",
                         lambda: torch_svm(kind, tm, x), min(ms))
            emit(f"svm_{kind}_predict_f32 {nsv}x{dim}", dim, items, ok, ms, steps, 4 * dim * items + 8 * items, **line)
    return ok_all


def run_bayes(_gib):
    ok_all = True
    for c, d, items in BAYES_SHAPES:
        m, _ = mr.bayes_model(c, d)
        gen = torch.Generator(device="cuda").manual_seed(41)
        x = torch.rand((items, d), generator=gen, device="cuda", dtype=torch.float32) * 6 - 3
        th, sg, pr = (torch.from_numpy(m[k]).cuda() for k in ("theta", "sigma", "priors"))
        S, keep = dsp.bayes_instance(th, sg, pr, m["eps"])
        prob = torch.zeros((items, c), dtype=torch.float32, device="cuda")
        cls = torch.zeros(items, dtype=torch.int32, device="cuda")
        ours = lambda: dsp.bayes_predict_batch(S, x, prob, cls)                     # noqa: E731
        ours()
        torch.cuda.synchronize()
        wprob, widx = mr.bayes_predict(m, x[[0, items - 1]].cpu().numpy())
        ok = mr.same_word(prob[[0, items - 1]].cpu().numpy(), wprob) and \
            cls[[0, items - 1]].cpu().numpy().tolist() == widx.tolist()
        ok_all = ok_all and ok
        ms, steps = bc.measure(ours)
        sig = sg + float(m["eps"])
        const = -0.5 * torch.log(2 * np.pi * sig).sum(1) + torch.log(pr)

        def torch_bayes():
            p = const[None, :] - 0.5 * (((x[:, None, :] - th[None]) ** 2) / sig[None]).sum(2)
            return p, p.argmax(1)
        line = {"flops_per_item": 4 * c * d, "Gflops": round(4 * c * d * items / (min(ms) * 1e-3) * 1e-9, 1)}
        bc.yardstick(line, "torch", "torch formulation (unordered sums), same tensors", torch_bayes, min(ms))
        emit(f"gaussian_naive_bayes_predict_f32 {c} classes x {d}", d, items, ok, ms, steps,
             4 * d * items + 4 * c * items + 4 * items, **line)
    return ok_all


def run_ref(ref):
    """The reference's scalar predict functions (oracle/ref.mk's flags) on one CPU thread; needs the reference tree."""
    import ctypes as C
    import subprocess
    import tempfile
    import time
    sys.path.insert(0, os.path.join(ROOT, "cmsis-dsp_amd", "cmsisdsp_amd"))
    import _abi
    src = os.path.join(ref, "Source")
    files = [os.path.join(src, "SVMFunctions", f"arm_svm_{k}_{f}_f32.c") for k in mr.SVM_KINDS for f in ("init", "predict")]
    files += [os.path.join(src, "BayesFunctions", "arm_gaussian_naive_bayes_predict_f32.c"),
              os.path.join(src, "StatisticsFunctions", "arm_max_f32.c")]
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libml_ref.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-D__GNUC_PYTHON__", "-DARM_MATH_LOOPUNROLL", "-ffp-contract=off", "-w",
                        "-shared", "-I" + os.path.join(ref, "Include"), "-I" + os.path.join(ref, "PrivateInclude"),
                        *files, "-o", so, "-lm"], check=True)
        lib = C.CDLL(so)
        for name, (res, args) in _abi.ML.items():
            if "svm" in name or "bayes" in name:
                if not name.endswith("_batch"):
                    getattr(lib, name).restype, getattr(lib, name).argtypes = res, args

        def best_of(call, reps):
            best = 1e9
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                best = min(best, (time.perf_counter() - t0) / reps)
            return best
        for nsv, dim, _ in SVM_SHAPES:
            for kind in mr.SVM_KINDS:
                m, x = mr.svm_model(kind, nsv, dim, 3 if kind == "polynomial" else 0, items=64)
                S = _abi.SVM_KINDS[kind][0]()
                extra = {"linear": [], "polynomial": [3, float(m["coef0"]), float(m["gamma"])],
                         "rbf": [float(m["gamma"])]}[kind]
                getattr(lib, f"arm_svm_{kind}_init_f32")(C.byref(S), nsv, dim, float(m["intercept"]),
                                                         m["dual"].ctypes.data, m["sv"].ctypes.data,
                                                         m["classes"].ctypes.data, *extra)
                out = np.zeros(1, np.int32)
                fn, v = getattr(lib, f"arm_svm_{kind}_predict_f32"), x[0].copy()
                t = best_of(lambda: fn(C.byref(S), v.ctypes.data, out.ctypes.data), max(200, 2 ** 24 // (nsv * dim)))
                print(json.dumps({"workload": f"reference arm_svm_{kind}_predict_f32 {nsv}x{dim}, one CPU thread",
                                  "us_per_item": round(t * 1e6, 3), "M_items_per_s": round(1e-6 / t, 4)}), flush=True)
        for c, d, _ in BAYES_SHAPES:
            m, x = mr.bayes_model(c, d)
            S = _abi.arm_gaussian_naive_bayes_instance_f32(d, c, m["theta"].ctypes.data, m["sigma"].ctypes.data,
                                                           m["priors"].ctypes.data, float(m["eps"]))
            prob, v = np.zeros(c, np.float32), x[0].copy()
            fn = lib.arm_gaussian_naive_bayes_predict_f32
            t = best_of(lambda: fn(C.byref(S), v.ctypes.data, prob.ctypes.data, None), max(200, 2 ** 22 // (c * d)))
            print(json.dumps({"workload": f"reference arm_gaussian_naive_bayes_predict_f32 {c} classes x {d}, one CPU thread",
                              "us_per_item": round(t * 1e6, 3), "M_items_per_s": round(1e-6 / t, 4)}), flush=True)
    return True


def main():
    args = sys.argv[1:]
    gib = 1.0
    if "ref" in args:
        i = args.index("--ref") if "--ref" in args else -1
        import re
        mk = open(os.path.join(ROOT, "oracle", "ref.mk")).read()                   # the default tree of oracle/ref.mk
        return run_ref(args[i + 1] if i >= 0 else re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1))
    gpu_modules()
    for flag in ("--gib", "--window"):
        if flag in args:
            i = args.index(flag)
            if flag == "--gib":
                gib = float(args[i + 1])
            else:
                bc.window_ms = float(args[i + 1])
            del args[i:i + 2]
    groups = args or ["ew", "logdom", "svm", "bayes"]
    bad = []
    for name, fn in (("ew", run_ew), ("logdom", run_logdom), ("svm", run_svm), ("bayes", run_bayes)):
        if name in groups and not fn(gib):
            bad.append(name)
    if bad:
        sys.exit(f"not bit-exact: {bad}")


if __name__ == "__main__":
    main()
