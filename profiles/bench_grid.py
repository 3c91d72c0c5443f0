"""Benchmark of xsarsea_amd.grid (k_wind_grid, csrc/xsw_cells.hip) on a 20000 x 20000 raster: the flagship scene inverted to
co-pol grid codes and their complex128 expansion as the two sources, geolocated by the tie grid of bench_ancillary_model.py.  HIP
events, median of warm repetitions, the variants taking turns inside every repetition.  Prints one JSON line and writes it to
profiles/grid_bench.json:

  - xsw_wind_grid from complex128 winds (16 B read per pixel) and from codes (4 B), on grids of 0.1 and 0.01 degree, each on the
    default path and on XSW_GRID_PATH=direct (every pixel's five 64-bit adds straight to global memory)
  - beside them, in the same run: k_ancillary_model (the same per-pixel geolocation arithmetic, 16 B written where k_wind_grid
    reads 16 B) and k_cells at 100 x 100 pixels
  - one grid whose bins are smaller than a pixel, on the 4000 x 4000 corner of the raster, where no pre-aggregation helps: the
    rate of 64-bit integer global atomics, in adds and in added bytes per second

    python profiles/bench_grid.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/grid_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_ancillary_model import scene  # noqa: E402  (same folder)

GRIDS = {"0.1": (-13.0, 0.1, 35, 44.5, 0.1, 30), "0.01": (-13.0, 0.01, 350, 44.5, 0.01, 300)}
SUB = 4000                  # the raster of the sub-pixel grid
SUB_STEP = 5e-5             # its bins, degrees: a pixel is 1.2e-4 by 0.95e-4 degrees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grid_bench.json"))
    a = ap.parse_args()

    import torch
    import bench  # the scene generator of the flagship benchmark (repository root)
    from xsarsea_amd import TiePoints, _lib, streaks as S

    n = a.size
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ctx.upload_luts(co=bench.build_product_lut()[1])
    inc, s_vv, anc = bench.make_scene(n, n, n, 0, 20260320 + 2, dev)
    codes = torch.empty((n, n), dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE
    ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(codes))
    del anc, inc, s_vv
    wind = torch.empty((n, n), dtype=torch.complex128, device=dev)
    ctx.expand_codes_raw(n * n, DEV, F64, p(codes), None, p(wind), None)
    ctx.synchronize()

    def geometry(m, span):
        """Tie tables and per-pixel brackets on the device for an m x m raster covering `span` of the benchmark scene."""
        tie_line, tie_sample, lon, lat, heading, mlon, mlat, u, v = scene(m)
        lon, lat = lon[0, 0] + span * (lon - lon[0, 0]), lat[0, 0] + span * (lat - lat[0, 0])
        tp = TiePoints(tie_line, tie_sample, lon, lat, heading)
        put = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
        lf, lt = S.bracket(tp.line, np.arange(m))
        sf, st = S.bracket(tp.sample, np.arange(m))
        tables = [put(x, np.float64) for x in (tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading)]
        tables += [put(lf, np.int32), put(lt, np.float64), put(sf, np.int32), put(st, np.float64)]
        return tp, tables, (mlon, mlat, u, v)

    tp, tables, (mlon, mlat, mu, mv) = geometry(n, 1.0)
    variants, results, pixels = {}, {}, {}

    def grid_call(src, t, m, tp_, tables_, grid, path):
        lon0, dlon, n_lon, lat0, dlat, n_lat = grid
        sums = torch.zeros((5, n_lat, n_lon), dtype=torch.int64, device=dev)
        kind = _lib.CELLS_C128 if src == "complex128" else _lib.CELLS_CODES

        def run():
            if path == "default":
                os.environ.pop("XSW_GRID_PATH", None)
            else:
                os.environ["XSW_GRID_PATH"] = path
            ctx.wind_grid_raw(m, m, DEV, kind, p(t), None, len(tp_.line), len(tp_.sample), *(p(x) for x in tables_), lon0, dlon, n_lon, 0, lat0, dlat,
                              n_lat, p(sums))
        return run, sums

    for src, t in (("complex128", wind), ("codes", codes)):
        for gname, grid in GRIDS.items():
            for path in ("default", "direct"):
                name = f"{src} {gname} {path}"
                variants[name], results[name] = grid_call(src, t, n, tp, tables, grid, path)
                pixels[name] = n * n

    # the sub-pixel grid on the raster's corner, at the scene's own pixel spacing
    m = min(SUB, n)
    tp_s, tables_s, _ = geometry(m, m / 20000.0)
    lo, hi = tp_s.longitude.min(), tp_s.longitude.max()
    la, lb = tp_s.latitude.min(), tp_s.latitude.max()
    sub_grid = (float(lo), SUB_STEP, int((hi - lo) / SUB_STEP) + 1, float(la), SUB_STEP, int((lb - la) / SUB_STEP) + 1)
    wind_s, codes_s = wind[:m, :m].contiguous(), codes[:m, :m].contiguous()
    for src, t in (("complex128", wind_s), ("codes", codes_s)):
        for path in ("default", "direct"):
            name = f"{src} sub-pixel {path}"
            variants[name], results[name] = grid_call(src, t, m, tp_s, tables_s, sub_grid, path)
            pixels[name] = m * m

    # beside them: k_ancillary_model (float64 model grid; the latitude axis descends: read backwards, as the public call does) ...
    put = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    tu, tv = put(mu[::-1], np.float64), put(mv[::-1], np.float64)
    out = torch.empty((n, n), dtype=torch.complex128, device=dev)
    dlon, dlat = float(mlon[-1] - mlon[0]) / (len(mlon) - 1), float(mlat[0] - mlat[-1]) / (len(mlat) - 1)
    variants["k_ancillary_model"] = lambda: ctx.ancillary_model_raw(n, n, DEV, F64, p(tu), p(tv), len(mlat), len(mlon), float(mlon[0]), dlon, 0,
                                                                    float(mlat[-1]), dlat, len(tp.line), len(tp.sample), *(p(x) for x in tables), p(out))
    # ... and k_cells at 100 x 100 pixels, from both sources
    shape = (-(-n // 100), -(-n // 100))
    co = [torch.empty(shape, dtype=dt, device=dev) for dt in (torch.int32, torch.complex128, torch.float64, torch.float64, torch.float64)]
    for src, kind, t in (("complex128", _lib.CELLS_C128, wind), ("codes", _lib.CELLS_CODES, codes)):
        variants[f"k_cells {src} 100x100"] = (lambda kind=kind, t=t: ctx.wind_cells_raw(n, n, DEV, kind, p(t), None, 100, 100, 0, 0, *[None] * 8,
                                                                                       *(p(x) for x in co), None, None, None, None))

    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.steps):  # alternating: one repetition of every variant per round
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    os.environ.pop("XSW_GRID_PATH", None)
    med = {k: float(np.median(v)) for k, v in times.items()}

    # every variant of one grid ran equally often: both paths and both sources hold the same sums
    same = {}
    for gname in list(GRIDS) + ["sub-pixel"]:
        ref = results[f"complex128 {gname} default"]
        same[gname] = bool(all(torch.equal(results[f"{src} {gname} {path}"], ref) for src in ("complex128", "codes") for path in ("default", "direct")))
    reps = a.warmup + a.steps
    added = {g: int(results[f"complex128 {g} default"][0].sum().item()) // reps for g in list(GRIDS) + ["sub-pixel"]}
    occupied = {g: int((results[f"complex128 {g} default"][0] > 0).sum().item()) for g in list(GRIDS) + ["sub-pixel"]}
    sub_ms = med["complex128 sub-pixel direct"]
    res = {"workload": "grid", "raster": [n, n], "tie_grid": [len(tp.line), len(tp.sample)], "steps": a.steps, "warmup": a.warmup,
           "grids": {**{k: list(v) for k, v in GRIDS.items()}, "sub-pixel": list(sub_grid)}, "sub_pixel_raster": [m, m],
           "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "ratio_to_k_ancillary_model": {k: round(med[k] / med["k_ancillary_model"], 3) for k in pixels if pixels[k] == n * n},
           "default_over_direct": {f"{src} {g}": round(med[f"{src} {g} default"] / med[f"{src} {g} direct"], 3)
                                   for src in ("complex128", "codes") for g in list(GRIDS) + ["sub-pixel"]},
           "pixels_added_per_call": added, "occupied_bins": occupied,
           "int64_atomic_adds_per_second_direct_sub_pixel": round(5 * added["sub-pixel"] / (sub_ms * 1e-3), 0),
           "int64_atomic_added_bytes_per_second_direct_sub_pixel": round(40 * added["sub-pixel"] / (sub_ms * 1e-3), 0),
           "paths_and_sources_give_equal_sums": same, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
