"""Benchmark of xsarsea_amd.landmask on a 20000 x 20000 raster under the 10 x 21 tie grid of bench_ancillary_model.py.  HIP events,
median of warm repetitions with every repetition listed.  Prints one JSON line and writes it to profiles/landmask_bench.json.

Three synthetic coastlines: none within the scene's latitudes (open ocean), about 1e4 edges and about 1e5 edges crossing the scene
(a wiggly coast running north-south through it, and islands).  For each, in the same run:

  - k_land_mask (XSW_LAND_PATH=bands, the plan's own band count) and k_land_mask_direct (every pixel against every edge): the raw
    entry on prepared device buffers
  - land_mask as the user calls it (host plan, table uploads, launch)
  - edges listed per band (from the plan: the bound on edges tested per pixel) and the share of the 8 TB/s HBM peak the 1 B per
    pixel makes
and once per run k_ancillary_model (the same geolocation arithmetic, 16 B per pixel) and the page-locked upload of a 0.4 GB host
mask, which the call replaces.  The direct kernel on 1e5 edges takes seconds per run: it gets --direct-steps repetitions.

    python profiles/bench_landmask.py [--size 20000] [--steps 7] [--warmup 2] [--direct-steps 3] [--out profiles/landmask_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_ancillary_model import scene  # noqa: E402  (same folder)
from bench_gradients import HBM_PEAK_GBS  # noqa: E402
from bench_streaks import median_ms  # noqa: E402


def coast(n_edges, lat_a, lat_b, seed):
    """A coastline of about n_edges edges between latitudes lat_a < lat_b: land east of a wiggly line near longitude -11 (four
    fifths of the edges), and a dozen star-shaped islands west of it."""
    rng = np.random.default_rng(seed)
    m = max(int(0.8 * n_edges), 8)
    y = np.linspace(lat_a, lat_b, m)
    x = -11.0 + 0.35 * np.sin(3.1 * y) + 0.08 * np.sin(41.0 * y) + np.cumsum(rng.normal(0, 0.6 / m, m)) + rng.normal(0, 0.0003, m)
    rings = [np.concatenate([np.stack([x, y], axis=1), [[-5.0, lat_b], [-5.0, lat_a]]])]
    per = max((n_edges - m) // 12, 3)
    for k in range(12):
        t = 2 * np.pi * np.arange(per) / per
        r = (0.03 + 0.05 * rng.uniform()) * (1 + 0.3 * np.cos(5 * t) + 0.1 * np.cos(17 * t + k))
        cx, cy = -12.4 + 0.9 * rng.uniform(), lat_a + (lat_b - lat_a) * (0.1 + 0.8 * (k + 0.5) / 12)
        rings.append(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1))
    return rings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--direct-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "landmask_bench.json"))
    a = ap.parse_args()

    import torch
    from xsarsea_amd import Coastline, TiePoints, _lib, land_mask, landmask, streaks as S
    from xsarsea_amd._raster import _Call, _small

    n = a.size
    dev = torch.device("cuda")
    tie_line, tie_sample, lon, lat, heading, mlon, mlat, u, v = scene(n)
    tp = TiePoints(tie_line, tie_sample, lon, lat, heading)
    out = torch.empty((n, n), dtype=torch.uint8, device=dev)
    call = _Call(out)
    lf, lt = S.bracket(tp.line, np.arange(n))
    sf, st = S.bracket(tp.sample, np.arange(n))
    lf, lt, sf, st = (_small(call, x, t) for x, t in ((lf, np.int32), (lt, np.float64), (sf, np.int32), (st, np.float64)))
    tlon, tlat, tcos, tsin = (_small(call, x, np.float64) for x in (tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading))
    frac = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 5)

    os.environ.pop("XSW_LAND_BANDS", None)
    cases = {}
    for name, rings in (("open_ocean", coast(10000, 60.0, 62.0, 1)), ("coast_1e4", coast(10000, 43.0, 49.0, 2)), ("coast_1e5", coast(100000, 43.0, 49.0, 3))):
        c = Coastline(rings)
        p = landmask.plan(c, tp)
        edges = _small(call, p.edges, np.float64) if len(p.edges) else None
        bstart, bedges = (_small(call, x, np.int32) for x in (p.band_start, p.band_edges)) if len(p.band_edges) else (None, None)
        res = {"edges": int(len(c.edges)), "edges_kept_by_the_plan": int(len(p.edges)), "n_bands": int(p.n_bands),
               "edges_listed_per_band_mean": round(p.mean_band_edges, 1),
               "edges_listed_per_band_max": int(np.diff(p.band_start).max()), "band_height_deg": p.h}
        masks = {}
        for path in ("bands", "direct"):
            os.environ["XSW_LAND_PATH"] = path
            nb = p.n_bands if bstart is not None else 0
            raw = lambda: call.run(lambda ctx, mem: ctx.land_mask_raw(
                n, n, mem, len(tp.line), len(tp.sample), tlon.data_ptr(), tlat.data_ptr(), lf.data_ptr(), lt.data_ptr(), sf.data_ptr(), st.data_ptr(),
                len(p.edges), None if edges is None else edges.data_ptr(), nb, None if bstart is None else bstart.data_ptr(), len(p.band_edges),
                None if bedges is None else bedges.data_ptr(), p.lat0, p.h, None, 0, out.data_ptr()), [])
            slow = path == "direct" and len(p.edges) > 20000
            ms, ms_all = median_ms(torch, raw, a.direct_steps if slow else a.steps, 1 if slow else a.warmup)
            masks[path] = out.clone()
            res[f"{path}_ms"], res[f"{path}_ms_all"] = round(ms, 3), ms_all
            res[f"{path}_fraction_of_hbm_peak"] = frac(n * n, ms)
        res["bands_equals_direct"] = bool(torch.equal(masks["bands"], masks["direct"]))
        res["land_share"] = round(float((masks["bands"] == 0).double().mean()), 4)
        os.environ["XSW_LAND_PATH"] = "bands"
        call_ms, call_all = median_ms(torch, lambda: land_mask(c, tp, shape=(n, n), device=dev), a.steps, a.warmup)
        res["land_mask_call_ms"], res["land_mask_call_ms_all"] = round(call_ms, 3), call_all
        res["raw_entry_equals_public_call"] = bool(torch.equal(land_mask(c, tp, shape=(n, n), device=dev), masks["bands"]))
        cases[name] = res
        del masks
    os.environ.pop("XSW_LAND_PATH", None)

    # k_ancillary_model beside it: the same geolocation arithmetic, 16 B per pixel
    anc = torch.empty((n, n), dtype=torch.complex128, device=dev)
    tu, tv = (_small(call, x[::-1], np.float64) for x in (u, v))
    dlon, dlat = float(mlon[-1] - mlon[0]) / (len(mlon) - 1), float(mlat[0] - mlat[-1]) / (len(mlat) - 1)
    anc_ms, anc_all = median_ms(torch, lambda: call.run(lambda ctx, mem: ctx.ancillary_model_raw(
        n, n, mem, _lib.XSW_F64, tu.data_ptr(), tv.data_ptr(), len(mlat), len(mlon), float(mlon[0]), dlon, 0, float(mlat[-1]), dlat, len(tp.line),
        len(tp.sample), tlon.data_ptr(), tlat.data_ptr(), tcos.data_ptr(), tsin.data_ptr(), lf.data_ptr(), lt.data_ptr(), sf.data_ptr(),
        st.data_ptr(), anc.data_ptr()), [tu, tv]), a.steps, a.warmup)
    del anc

    # what the call replaces: the mask built on the host, copied over the link from page-locked memory
    pinned = torch.empty((n, n), dtype=torch.uint8, pin_memory=True)
    pinned.copy_(out)
    torch.cuda.synchronize()
    copy_ms, copy_all = median_ms(torch, lambda: out.copy_(pinned, non_blocking=True), a.steps, a.warmup)

    res = {"workload": "land_mask", "raster": [n, n], "tie_grid": [len(tp.line), len(tp.sample)], "steps": a.steps, "warmup": a.warmup,
           "direct_steps_above_20000_edges": a.direct_steps, "chunk_edges": _lib.land_chunk_edges(), "mask_bytes": n * n, "coastlines": cases,
           "k_ancillary_model_f64_ms": round(anc_ms, 3), "k_ancillary_model_f64_ms_all": anc_all,
           "pinned_h2d_uint8_ms": round(copy_ms, 3), "pinned_h2d_uint8_ms_all": copy_all,
           "pinned_h2d_uint8_gbs": round(n * n / (copy_ms * 1e-3) / 1e9, 2), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
