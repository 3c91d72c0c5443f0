"""Benchmark of xsarsea_amd.gradients in the notebook configuration (windows_sizes=[1600, 3200], downscales_factors=[1, 2],
window_step=1) on a float32 device raster with streaks, speckle and NaN land patches.  Prints one JSON line: sigma0 Mpixels/s of
the whole histogram call, per-kernel ms (HIP events around each stage), algorithmic bytes and their fraction of HBM peak, and a
CPU baseline (the test restatement, tests/gradients_ref.py, on a crop).

    python profiles/bench_gradients.py [--size 20000] [--steps 5] [--warmup 2] [--crop 2048 | --crop 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
WS, DF = [1600, 3200], [1, 2]


def scene(torch, n, seed=1):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    y = torch.arange(n, device=dev, dtype=torch.float32)[:, None]
    x = torch.arange(n, device=dev, dtype=torch.float32)[None, :]
    th = torch.where(y < n / 2, 0.5, -0.8) + torch.where(x < n / 2, 0.0, 0.6)
    t = 0.08 * (1 + 0.3 * torch.sin((x * torch.cos(th) + y * torch.sin(th)) * (2 * np.pi / 24)))
    t *= 1 + 0.2 * torch.randn((n, n), generator=g, device=dev)
    t[: n // 7, (3 * n) // 4:] = float("nan")
    t[((y - 0.6 * n) ** 2 + (x - 0.25 * n) ** 2) < (0.075 * n) ** 2] = float("nan")
    return t


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crop", type=int, default=2048, help="CPU baseline crop side (0: no baseline)")
    a = ap.parse_args()

    import torch
    from xsarsea_amd import gradients as G

    n = a.size
    t = scene(torch, n)
    torch.cuda.synchronize()
    run = lambda: G.Gradients(t, windows_sizes=WS, downscales_factors=DF, window_step=1).histogram
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        h, ms = timed(torch, run)
        times.append(ms)
    ms_call = float(np.median(times))
    nwin = int(np.prod(h.weight.shape[2:4]))

    # per stage, HIP events around each kernel call (the same calls `histogram` makes)
    stage_ms, traffic = {}, {}
    line = np.arange(n)
    at = G.Gradients2D(t, window_size=WS[0]).windows_at
    for f in DF:
        src, (area_ms) = (t, 0.0) if f == 1 else timed(torch, lambda: G._area(t, f))
        if f > 1:
            stage_ms[f"k_grad_area f{f}"] = area_ms
            traffic[f"k_grad_area f{f}"] = n * n * 4 + (n // f) ** 2 * 4
        m = n // f
        ampl, stage_ms[f"k_grad_r2 f{f}"] = timed(torch, lambda: G._r2(src, True))
        traffic[f"k_grad_r2 f{f}"] = m * m * 4 + (m // 2) ** 2 * 8
        (g2, g3, c), stage_ms[f"k_grad_local f{f}"] = timed(torch, lambda: G._local(ampl))
        traffic[f"k_grad_local f{f}"] = (m // 2) ** 2 * 8 + (m // 4) ** 2 * 32
        lc = G.coarsen_coords(G.coarsen_coords(G.coarsen_coords(line, f) if f > 1 else line, 2), 2)
        rows = G.nearest_indexer(lc, at["line"])
        for ws in WS:
            w = G.window_pixels(ws, lc, lc)
            _, stage_ms[f"k_grad_hist f{f} w{w}"] = timed(torch, lambda: G._hist(g2, c, w, rows, rows, 72))
            traffic[f"k_grad_hist f{f} w{w}"] = len(rows) ** 2 * w * w * 24  # each window's (G2, c) read once
        del ampl, g2, g3, c
    total_bytes = sum(traffic.values())
    res = {
        "workload": "gradients_histogram", "raster": [n, n], "dtype": "float32", "windows_sizes": WS, "downscales_factors": DF,
        "window_step": 1, "windows": nwin, "ms_per_call": round(ms_call, 3), "ms_calls": [round(x, 3) for x in times],
        "sigma0_mpix_per_s": round(n * n / (ms_call * 1e-3) / 1e6, 1),
        "kernel_ms": {k: round(v, 3) for k, v in stage_ms.items()},
        "kernel_ms_sum": round(sum(stage_ms.values()), 3),
        "algorithmic_bytes": int(total_bytes),
        "algorithmic_bytes_by_kernel": {k: int(v) for k, v in traffic.items()},
        "hbm_fraction_of_peak": round(total_bytes / (ms_call * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
    }
    if a.crop:
        import gradients_ref as ref
        crop = t[: a.crop, : a.crop].cpu().numpy()
        cl = np.arange(a.crop)
        t0 = time.perf_counter()
        ref.histogram(crop, cl, cl, windows_sizes=tuple(WS), downscales_factors=tuple(DF), window_step=1)
        cpu_s = time.perf_counter() - t0
        res["cpu_baseline"] = {"what": "tests/gradients_ref.py (numpy/scipy restatement), one thread", "crop": [a.crop, a.crop],
                               "seconds": round(cpu_s, 3), "sigma0_mpix_per_s": round(a.crop ** 2 / cpu_s / 1e6, 3)}
        res["speedup_vs_cpu_baseline"] = round(res["sigma0_mpix_per_s"] / res["cpu_baseline"]["sigma0_mpix_per_s"], 1)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
