"""Benchmark of the masked direction histograms (xsarsea_amd.gradients with min_F / mask) in the notebook configuration
(windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=1) on the 20000 x 20000 float32 tiled rain scene of the tests.
HIP events, median of warm repetitions, the variants of one comparison alternating inside one loop.  Prints one JSON line:

  hist_ms            per (factor, window): the unmasked kernel, the masked kernel with an all-ones mask and with the min_F mask,
                     and their ratios to the unmasked kernel of the same run
  keep_ms            k_grad_keep alone (float64 F at block 2; a uint8 sigma0-grid mask at blocks 4 and 8) against its bytes
  call_ms            Gradients(min_F=0.7).histogram beside the unmasked call plus one filtering_parameters call per field
  unmasked_reference the unmasked call on the scene of profiles/bench_gradients.py, to compare with profiles/gradients_bench.json

    python profiles/bench_gradients_masked.py [--size 20000] [--steps 7] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "profiles"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
WS, DF, MIN_F = [1600, 3200], [1, 2], 0.7


def alternating(torch, fns, steps, warmup):
    """Median ms of each fn, the fns taking turns inside every repetition (HIP events around each call)."""
    times = [[] for _ in fns]
    for rep in range(warmup + steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times], [[round(x, 3) for x in t] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import torch
    import filtering_ref as fr
    from bench_gradients import scene as streak_scene
    from xsarsea_amd import gradients as G

    n = a.size
    tile = torch.from_numpy(fr.full_tile()).cuda()
    reps = -(-n // tile.shape[0])
    t = tile.repeat(reps, reps)[:n, :n].contiguous()
    torch.cuda.synchronize()
    line = np.arange(n)
    at = G.Gradients2D(t, window_size=WS[0]).windows_at

    hist_ms, keep_share = {}, {}
    for f in DF:
        field = G._Field(t, line, line, f, min_F=MIN_F)
        g2, c, lgl, lgs = field.lg
        koch = field.keep
        ones = torch.ones_like(koch)
        keep_share[f"f{f}"] = round(float(koch.float().mean()), 4)
        rows = G.nearest_indexer(lgl, at["line"])
        for ws in WS:
            w = G.window_pixels(ws, lgl, lgs)
            fns = [lambda: G._hist(g2, c, w, rows, rows, 72), lambda: G._hist(g2, c, w, rows, rows, 72, keep=ones),
                   lambda: G._hist(g2, c, w, rows, rows, 72, keep=koch)]
            (plain, m1, mk), raw = alternating(torch, fns, a.steps, a.warmup)
            hist_ms[f"f{f} w{w}"] = {"unmasked": round(plain, 3), "masked_all_ones": round(m1, 3), "masked_min_F": round(mk, 3),
                                     "ratio_all_ones": round(m1 / plain, 4), "ratio_min_F": round(mk / plain, 4), "ms": raw}
        del field, g2, c, koch, ones
    tot = {k: round(sum(v[k] for v in hist_ms.values()), 3) for k in ("unmasked", "masked_all_ones", "masked_min_F")}
    tot["ratio_all_ones"] = round(tot["masked_all_ones"] / tot["unmasked"], 4)
    tot["ratio_min_F"] = round(tot["masked_min_F"] / tot["unmasked"], 4)

    # k_grad_keep alone against its bytes
    keep_ms = {}
    F = G.filtering_parameters(t).F
    u8 = (t > 0.04).to(torch.uint8)
    cases = {"f64 block 2 (F, half -> quarter resolution)": (lambda: G.keep_mask(F, threshold=MIN_F, block=2), F.numel() * 8 + F.numel() // 4),
             "u8 block 4 (sigma0-grid mask, factor 1)": (lambda: G.keep_mask(u8, block=4), u8.numel() + u8.numel() // 16),
             "u8 block 8 (sigma0-grid mask, factor 2)": (lambda: G.keep_mask(u8, block=8), u8.numel() + u8.numel() // 64)}
    for name, (fn, nbytes) in cases.items():
        (ms,), raw = alternating(torch, [fn], a.steps, a.warmup)
        keep_ms[name] = {"ms": round(ms, 4), "bytes": int(nbytes), "gb_per_s": round(nbytes / ms / 1e6, 1),
                         "fraction_of_hbm_peak": round(nbytes / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4), "all_ms": raw[0]}
    del F, u8

    # the whole call beside what it replaces
    masked_call = lambda: G.Gradients(t, windows_sizes=WS, downscales_factors=DF, min_F=MIN_F).histogram
    plain_call = lambda: G.Gradients(t, windows_sizes=WS, downscales_factors=DF).histogram

    def separate():
        h = plain_call()
        for f in DF:
            G.filtering_parameters(t if f == 1 else G._area(t, f))
        return h
    (cm, cp, cs), raw = alternating(torch, [masked_call, plain_call, separate], a.steps, a.warmup)
    call_ms = {"Gradients(min_F).histogram": round(cm, 3), "unmasked Gradients.histogram": round(cp, 3),
               "unmasked + filtering_parameters per field": round(cs, 3), "ms": raw}

    # the unmasked call on the scene of profiles/bench_gradients.py (profiles/gradients_bench.json: 19.7 ms)
    del t
    s = streak_scene(torch, n)
    torch.cuda.synchronize()
    (ref_ms,), raw = alternating(torch, [lambda: G.Gradients(s, windows_sizes=WS, downscales_factors=DF, window_step=1).histogram], a.steps,
                                 a.warmup)
    res = {"workload": "gradients_histogram_masked", "raster": [n, n], "dtype": "float32", "windows_sizes": WS, "downscales_factors": DF,
           "min_F": MIN_F, "kept_share": keep_share, "steps": a.steps, "warmup": a.warmup, "hist_ms": hist_ms, "hist_ms_total": tot,
           "keep_ms": keep_ms, "call_ms": call_ms,
           "unmasked_reference": {"scene": "profiles/bench_gradients.py", "ms_per_call": round(ref_ms, 3), "ms": raw[0]},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
