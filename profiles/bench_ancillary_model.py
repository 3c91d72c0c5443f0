"""Benchmark of xsarsea_amd.ancillary on a 20000 x 20000 raster: a 0.1 degree regional model grid under the scene and a 10 x 21
tie-point grid.  HIP events, median of warm repetitions.  Prints one JSON line and writes it to profiles/ancillary_model_bench.json:

  - k_ancillary_model alone (16 B written per pixel, nothing streamed in) for float32 and float64 model grids, as a fraction of the
    8 TB/s HBM peak
  - k_streaks_ancillary on a raster of the same shape (32 B per pixel), measured in the same run
  - the pinned host-to-device copy of a complex128 raster of that size: the step the call replaces
  - ancillary_from_model as the user calls it (host checks, table uploads, launch)

    python profiles/bench_ancillary_model.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/ancillary_model_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_gradients import HBM_PEAK_GBS  # noqa: E402  (same folder)
from bench_streaks import median_ms  # noqa: E402


def scene(n):
    """A descending-pass scene of about 2.4 x 1.9 degrees: the tie grid (10 lines x 21 samples) and the model grid around it."""
    tie_line, tie_sample = np.linspace(0, n - 1, 10), np.linspace(0, n - 1, 21)
    fl, fs = tie_line[:, None] / (n - 1), tie_sample[None, :] / (n - 1)
    lon = -12.3 + 2.4 * fs - 0.45 * fl + 0.02 * fs * fl
    lat = 46.9 - 1.9 * fl - 0.35 * fs
    heading = -167.5 + 1.2 * fl + 0.8 * fs
    mlon, mlat = -14.0 + 0.1 * np.arange(51), 48.0 - 0.1 * np.arange(41)
    rng = np.random.default_rng(1)
    yy, xx = np.meshgrid(mlat, mlon, indexing="ij")
    u = 9 * np.cos(0.8 * xx + 0.3 * yy) + rng.normal(0, 1, xx.shape)
    v = 7 * np.sin(0.5 * xx - 0.6 * yy) + rng.normal(0, 1, xx.shape)
    return tie_line, tie_sample, lon, lat, heading, mlon, mlat, u, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ancillary_model_bench.json"))
    a = ap.parse_args()

    import torch
    from xsarsea_amd import TiePoints, _lib, ancillary_from_model, streaks as S
    from xsarsea_amd._raster import _Call, _small

    n = a.size
    dev = torch.device("cuda")
    tie_line, tie_sample, lon, lat, heading, mlon, mlat, u, v = scene(n)
    tp = TiePoints(tie_line, tie_sample, lon, lat, heading)

    # the public call, numpy model fields in, device raster out
    call_ms, call_all = median_ms(torch, lambda: ancillary_from_model(u, v, mlon, mlat, tp, shape=(n, n), device=dev), a.steps, a.warmup)
    anc = ancillary_from_model(u, v, mlon, mlat, tp, shape=(n, n), device=dev)
    inside = float((~torch.isnan(anc.real)).double().mean())

    # the kernel alone: the raw entry point on prepared device buffers (the latitude axis descends: read backwards, as the call does)
    call = _Call(anc)
    lf, lt = S.bracket(tp.line, np.arange(n))
    sf, st = S.bracket(tp.sample, np.arange(n))
    lf, lt, sf, st = (_small(call, x, t) for x, t in ((lf, np.int32), (lt, np.float64), (sf, np.int32), (st, np.float64)))
    tables = [_small(call, x, np.float64) for x in (tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading)]
    out = call.empty((n, n), np.complex128)
    dlon, dlat = float(mlon[-1] - mlon[0]) / (len(mlon) - 1), float(mlat[0] - mlat[-1]) / (len(mlat) - 1)
    kern = {}
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        tu, tv = (_small(call, x[::-1], dt) for x in (u, v))
        xdt = _lib.XSW_F32 if dt == np.float32 else _lib.XSW_F64
        kern[name] = median_ms(torch, lambda: call.run(lambda ctx, mem: ctx.ancillary_model_raw(
            n, n, mem, xdt, tu.data_ptr(), tv.data_ptr(), len(mlat), len(mlon), float(mlon[0]), dlon, 0, float(mlat[-1]), dlat, len(tp.line),
            len(tp.sample), *(t.data_ptr() for t in tables), lf.data_ptr(), lt.data_ptr(), sf.data_ptr(), st.data_ptr(), out.data_ptr()),
            [tu, tv]), a.steps, a.warmup)
    ro, ra = torch.view_as_real(out), torch.view_as_real(anc)  # `out` holds the float64 run: the public call's own launch
    same = bool(torch.equal(torch.isnan(ro), torch.isnan(ra)) and torch.equal(torch.nan_to_num(ro), torch.nan_to_num(ra)))
    del ro, ra

    # k_streaks_ancillary beside it: 13 x 13 resolved directions spread over the same raster, the model raster as its a-priori input
    gen = torch.Generator(device=dev).manual_seed(2)
    ang = torch.rand((13, 13), generator=gen, device=dev, dtype=torch.float64) * np.pi
    dirs = torch.polar(torch.ones_like(ang), ang)
    wl, ws = np.linspace(800, n - 800, 13), np.linspace(800, n - 800, 13)
    wlf, wlt = S.bracket(wl, np.arange(n))
    wsf, wst = S.bracket(ws, np.arange(n))
    wlf, wlt, wsf, wst = (_small(call, x, t) for x, t in ((wlf, np.int32), (wlt, np.float64), (wsf, np.int32), (wst, np.float64)))
    streaks_ms, streaks_all = median_ms(torch, lambda: call.run(lambda ctx, mem: ctx.streaks_ancillary_raw(
        n, n, mem, anc.data_ptr(), 13, 13, dirs.data_ptr(), wlf.data_ptr(), wlt.data_ptr(), wsf.data_ptr(), wst.data_ptr(), out.data_ptr()),
        [anc, dirs]), a.steps, a.warmup)

    # what the call replaces: the raster built on the host, copied over the link from page-locked memory
    pinned = torch.empty((n, n), dtype=torch.complex128, pin_memory=True)
    pinned.copy_(anc)
    torch.cuda.synchronize()
    copy_ms, copy_all = median_ms(torch, lambda: out.copy_(pinned, non_blocking=True), a.steps, a.warmup)

    frac = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
    res = {
        "workload": "ancillary_model", "raster": [n, n], "model_grid": [len(mlat), len(mlon)], "model_step_deg": 0.1,
        "tie_grid": [len(tp.line), len(tp.sample)], "steps": a.steps, "warmup": a.warmup, "pixels_inside_the_grid": round(inside, 4),
        "k_ancillary_model_f32_ms": round(kern["f32"][0], 3), "k_ancillary_model_f32_ms_all": kern["f32"][1],
        "k_ancillary_model_f64_ms": round(kern["f64"][0], 3), "k_ancillary_model_f64_ms_all": kern["f64"][1],
        "k_ancillary_model_bytes": 16 * n * n,
        "k_ancillary_model_f32_fraction_of_hbm_peak": frac(16 * n * n, kern["f32"][0]),
        "k_ancillary_model_f64_fraction_of_hbm_peak": frac(16 * n * n, kern["f64"][0]),
        "raw_entry_equals_public_call": same,
        "k_streaks_ancillary_ms": round(streaks_ms, 3), "k_streaks_ancillary_ms_all": streaks_all, "k_streaks_ancillary_bytes": 32 * n * n,
        "k_streaks_ancillary_fraction_of_hbm_peak": frac(32 * n * n, streaks_ms),
        "pinned_h2d_complex128_ms": round(copy_ms, 3), "pinned_h2d_complex128_ms_all": copy_all,
        "pinned_h2d_complex128_gbs": round(16 * n * n / (copy_ms * 1e-3) / 1e9, 2),
        "ancillary_from_model_call_ms": round(call_ms, 3), "ancillary_from_model_call_ms_all": call_all,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
