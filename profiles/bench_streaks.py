"""Benchmark of xsarsea_amd.streaks on a 20000 x 20000 raster in the notebook configuration (windows_sizes=[1600, 3200],
downscales_factors=[1, 2], window_step=1: 13 x 13 windows, 4 histograms each).  HIP events, median of warm repetitions.  Prints one
JSON line and writes it to profiles/streaks_bench.json:

  - k_streaks_ancillary alone (32 B per pixel) as a fraction of the 8 TB/s HBM peak, beside k_detrend float64 -> float64 (16 B per
    pixel) measured in the same run
  - streaks_direction + ancillary_from_streaks as the user calls them, beside Gradients(...).histogram
  - the peak kernel's call against the torch-ops route it replaces (nanmean, circ_smooth, argmax with its host round trip)

    python profiles/bench_streaks.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/streaks_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_gradients import DF, HBM_PEAK_GBS, WS, scene, timed  # noqa: E402  (same folder)


def median_ms(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = [timed(torch, fn)[1] for _ in range(steps)]
    return float(np.median(times)), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streaks_bench.json"))
    a = ap.parse_args()

    import torch
    from xsarsea_amd import _device, _lib, gradients as G, streaks as S

    n = a.size
    dev = torch.device("cuda")
    sigma0 = scene(torch, n)
    gen = torch.Generator(device=dev).manual_seed(2)
    anc = torch.view_as_complex(6 * torch.randn((n, n, 2), generator=gen, device=dev, dtype=torch.float64))
    anc[: n // 7, (3 * n) // 4:] = complex(float("nan"), float("nan"))
    torch.cuda.synchronize()

    hist_ms, hist_all = median_ms(torch, lambda: G.Gradients(sigma0, windows_sizes=WS, downscales_factors=DF, window_step=1).histogram,
                                  a.steps, a.warmup)
    h = G.Gradients(sigma0, windows_sizes=WS, downscales_factors=DF, window_step=1).histogram
    nl, ns, na = (int(v) for v in h.weight.shape[-3:])

    dir_ms, _ = median_ms(torch, lambda: S.streaks_direction(h), a.steps, a.warmup)
    s = S.streaks_direction(h)
    anc_ms, anc_all = median_ms(torch, lambda: S.ancillary_from_streaks(s, anc), a.steps, a.warmup)
    both_ms, _ = median_ms(torch, lambda: S.ancillary_from_streaks(S.streaks_direction(h), anc), a.steps, a.warmup)

    # the kernels alone: the raw entry points on prepared device buffers
    call = G._Call(anc)
    w, r = h.weight.reshape(-1, nl, ns, na).contiguous(), h.used_ratio.reshape(-1, nl, ns).contiguous()
    idx, wo, ro = call.empty((nl, ns), np.int32), call.empty((nl, ns), np.float64), call.empty((nl, ns), np.float64)
    peak_ms, _ = median_ms(torch, lambda: call.run(lambda ctx, mem: ctx.streaks_peak_raw(w.shape[0], nl * ns, na, mem, True, w.data_ptr(), r.data_ptr(),
                                                                                      idx.data_ptr(), wo.data_ptr(), ro.data_ptr()), [w, r]),
                           a.steps, a.warmup)

    def torch_route():  # what a user did by hand: a dozen small launches and a host round trip for the peak
        m = G.circ_smooth(torch.nanmean(w, dim=0))
        i = torch.argmax(torch.nan_to_num(m, nan=0.0), dim=-1).cpu().numpy()
        return h.angles[i] + np.pi / 2

    torch_ms, _ = median_ms(torch, torch_route, a.steps, a.warmup)

    dirs = s.resolve(anc)
    lf, lt = S.bracket(s.line, np.arange(n))
    sf, st = S.bracket(s.sample, np.arange(n))
    lf, lt, sf, st = (S._small(call, v, t) for v, t in ((lf, np.int32), (lt, np.float64), (sf, np.int32), (st, np.float64)))
    out = call.empty((n, n), np.complex128)
    kern_ms, kern_all = median_ms(torch, lambda: call.run(lambda ctx, mem: ctx.streaks_ancillary_raw(
        n, n, mem, anc.data_ptr(), nl, ns, dirs.data_ptr(), lf.data_ptr(), lt.data_ptr(), sf.data_ptr(), st.data_ptr(), out.data_ptr()),
        [anc, dirs]), a.steps, a.warmup)
    del out

    # the yardstick: k_detrend float64 -> float64 on a raster of the same shape, same session
    x = torch.rand((n, n), device=dev, dtype=torch.float64) + 0.5
    y = torch.empty_like(x)
    ratio = np.linspace(0.8, 1.2, n)
    ctx = _lib.default_context(torch.cuda.current_device())

    def detrend():
        with _device.on_current_stream(ctx, dev):
            ctx.detrend_raw(n, n, _lib.XSW_F64, _lib.XSW_F64, _lib.MEM_DEVICE, x.data_ptr(), ratio, y.data_ptr())

    det_ms, det_all = median_ms(torch, detrend, a.steps, a.warmup)

    frac = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
    res = {
        "workload": "streaks", "raster": [n, n], "windows": [nl, ns], "histograms_per_window": int(w.shape[0]), "n_angles": na,
        "windows_sizes": WS, "downscales_factors": DF, "steps": a.steps, "warmup": a.warmup,
        "k_streaks_ancillary_ms": round(kern_ms, 3), "k_streaks_ancillary_ms_all": kern_all,
        "k_streaks_ancillary_bytes": 32 * n * n, "k_streaks_ancillary_fraction_of_hbm_peak": frac(32 * n * n, kern_ms),
        "k_detrend_f64_f64_ms": round(det_ms, 3), "k_detrend_f64_f64_ms_all": det_all, "k_detrend_bytes": 16 * n * n,
        "k_detrend_fraction_of_hbm_peak": frac(16 * n * n, det_ms),
        "streaks_direction_ms": round(dir_ms, 3), "ancillary_from_streaks_ms": round(anc_ms, 3), "ancillary_from_streaks_ms_all": anc_all,
        "streaks_direction_plus_ancillary_from_streaks_ms": round(both_ms, 3),
        "gradients_histogram_ms": round(hist_ms, 3), "gradients_histogram_ms_all": hist_all,
        "k_streaks_peak_call_ms": round(peak_ms, 4), "torch_ops_route_ms": round(torch_ms, 4),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
