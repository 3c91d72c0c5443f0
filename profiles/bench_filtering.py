"""Benchmark of xsarsea_amd.gradients.filtering_parameters on a float32 device raster (speckle, structure, rain blobs, NaN land:
the test scene tiled).  HIP events around warm whole calls and around each stage, then one `rocprofv3 --kernel-trace --stats`
run of this script (a fresh child process) for the per-kernel times.  For comparison the same run times the existing
`Gradients` front end at factor 1, sqrt(R2(sigma0)) then local_gradients (k_grad_r2, k_grad_local).  Prints one JSON line and
writes profiles/filtering_bench.json and profiles/filtering_kernel_stats.csv.

    python profiles/bench_filtering.py [--size 20000] [--steps 5] [--warmup 2] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def scene(torch, n):
    import filtering_ref as fr
    tile = torch.from_numpy(fr.full_tile()).cuda()
    reps = -(-n // tile.shape[0])
    return tile.repeat(reps, reps)[:n, :n].contiguous()


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def median_ms(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([timed(torch, fn)[1] for _ in range(steps)]))


def workload(a):
    import torch
    from xsarsea_amd import _build, gradients as G
    n = a.size
    t = scene(torch, n)
    torch.cuda.synchronize()
    ms_call = median_ms(torch, lambda: G.filtering_parameters(t), a.steps, a.warmup)
    # per stage: the same four calls filtering_parameters makes
    call = G._Call(t)
    L2 = n // 2
    r2, g3, c = (call.empty((L2, L2), np.float64) for _ in range(3))
    q4, out = call.empty((L2 // 2, L2 // 2), np.float64), call.empty((5, L2, L2), np.float64)
    dt, P = call.xsw_dtype(t), call.ptr
    stages = {
        "k_grad_r2 sqrt on load": (lambda: call.run(lambda ctx, mem: ctx.grad_r2_sqrt_raw(n, n, dt, mem, P(t), P(r2)), [t]),
                                   n * n * 4 + L2 * L2 * 8),
        "k_grad_local sqrt on load, no G2": (lambda: call.run(lambda ctx, mem: ctx.grad_local_sqrt_raw(n, n, dt, mem, P(t), None, P(g3), P(c)), [t]),
                                            n * n * 4 + L2 * L2 * 16),
        "k_grad_smooth (coarsen)": (lambda: call.run(lambda ctx, mem: ctx.grad_smooth_raw(L2, L2, mem, True, P(r2), P(q4)), [r2]),
                                    L2 * L2 * 8 + (L2 // 2) ** 2 * 8),
        "k_grad_filter": (lambda: call.run(lambda ctx, mem: ctx.grad_filter_raw(L2, L2, mem, P(r2), P(g3), P(c), P(q4), P(out)), [r2]),
                          L2 * L2 * 64),
    }
    stage_ms = {k: median_ms(torch, fn, a.steps, 1) for k, (fn, _) in stages.items()}
    traffic = {k: int(b) for k, (_, b) in stages.items()}
    # the existing front end at factor 1, for scale: ampl = sqrt(R2(sigma0)) (n/2), local_gradients(ampl) (n/4 outputs)
    ampl = G._r2(t, True)
    stage_ms["existing k_grad_r2 f1 (Gradients)"] = median_ms(torch, lambda: G._r2(t, True), a.steps, 1)
    stage_ms["existing k_grad_local f1 (Gradients)"] = median_ms(torch, lambda: G._local(ampl), a.steps, 1)
    fms = stage_ms["k_grad_filter"]
    return {
        "workload": "filtering_parameters", "raster": [n, n], "dtype": "float32", "ms_per_call": round(ms_call, 3),
        "sigma0_mpix_per_s": round(n * n / (ms_call * 1e-3) / 1e6, 1),
        "stage_ms": {k: round(v, 3) for k, v in stage_ms.items()}, "stage_ms_sum": round(sum(stage_ms[k] for k in stages), 3),
        "algorithmic_bytes_by_kernel": traffic,
        "k_grad_filter_fraction_of_hbm_peak": round(traffic["k_grad_filter"] / (fms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
        "k_grad_filter_over_existing_k_grad_local_f1": round(fms / stage_ms["existing k_grad_local f1 (Gradients)"], 3),
        "hbm_fraction_of_peak_whole_call": round(sum(traffic.values()) / (ms_call * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
        "measured": "ms_per_call, stage_ms (HIP events, median of warm repetitions); kernel stats file (rocprofv3 kernel trace)",
        "read_from_the_code": "algorithmic_bytes_by_kernel (compulsory traffic: each raster read or written once)",
        "device": torch.cuda.get_device_name(0), "code_object_sha256": _build.code_object_sha256(),
    }


def kernel_trace(a):
    """One rocprofv3 --kernel-trace --stats run of this script's workload in a fresh process; keeps the kernel stats table."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as td:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "filtering", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--size", str(a.size), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel stats file")
        dst = os.path.join(HERE, "filtering_kernel_stats.csv")
        shutil.copyfile(found[0], dst)
    with open(dst) as f:
        rows = [r for r in csv.DictReader(f) if "k_grad" in r["Name"]]
    out = {}
    for r in rows:
        name = re.search(r"k_grad_\w+(<[^>]*>)?", r["Name"]).group(0)
        out[name] = {"calls": int(r["Calls"]), "average_ms": round(float(r["AverageNs"]) / 1e6, 4), "min_ms": round(int(r["MinNs"]) / 1e6, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help="the traced run: the workload only, nothing written")
    a = ap.parse_args()
    res = workload(a)
    if a.child:
        return
    if not a.no_trace:
        res["kernel_trace_ms"] = kernel_trace(a)
    with open(os.path.join(HERE, "filtering_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
