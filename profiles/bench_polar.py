"""Benchmark of xsarsea_amd.polar (k_wind_polar, csrc/xsw_cells.hip) on a 20000 x 20000 raster: the flagship scene inverted to
co-pol grid codes and their complex128 expansion as the two sources, geolocated by the tie grid of bench_ancillary_model.py, the
centre in the middle of the scene.  HIP events, median of warm repetitions, the variants taking turns inside every repetition.
Prints one JSON line and writes it to profiles/polar_bench.json:

  - xsw_wind_polar from complex128 winds (16 B read per pixel) and from codes (4 B), in rings of 2 km with 4 sectors and of 1 km
    with 72 sectors, each on XSW_GRID_PATH=lds (the default) and =direct
  - beside them, in the same run: k_wind_grid on bins of 0.1 degree from both sources (the same bytes, the same three stages) and
    k_ancillary_model (the same per-pixel geolocation)
  - the ratio of every staged variant to k_wind_grid of the same source in this run
  - the two crossed bin sets (1 km with 4 sectors, 2 km with 72) from complex128 on the staged path: which of rings and sectors costs

    python profiles/bench_polar.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/polar_bench.json]

--cases / --paths restrict the polar variants (profiles/collect_polar_counters.sh runs one case per process under rocprofv3).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_ancillary_model import scene  # noqa: E402  (same folder)
from bench_grid import GRIDS  # noqa: E402

POLAR = {"2km x 4": (2.0, 4), "1km x 72": (1.0, 72)}
CROSSED = {"1km x 4": (1.0, 4), "2km x 72": (2.0, 72)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "polar_bench.json"))
    ap.add_argument("--cases", default=",".join(POLAR), help="comma-separated names of the polar bin sets to run")
    ap.add_argument("--paths", default="lds,direct")
    a = ap.parse_args()
    cases, paths = [c for c in POLAR if c in a.cases.split(",")], a.paths.split(",")
    full = cases == list(POLAR) and paths == ["lds", "direct"]

    import torch
    import bench  # the scene generator of the flagship benchmark (repository root)
    from xsarsea_amd import TiePoints, _lib, streaks as S
    from xsarsea_amd.polar import PolarSpec

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

    tie_line, tie_sample, lon, lat, heading, mlon, mlat, mu, mv = scene(n)
    tp = TiePoints(tie_line, tie_sample, lon, lat, heading)
    put = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    lf, lt = S.bracket(tp.line, np.arange(n))
    sf, st = S.bracket(tp.sample, np.arange(n))
    tables = [put(x, np.float64) for x in (tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading)]
    tables += [put(lf, np.int32), put(lt, np.float64), put(sf, np.int32), put(st, np.float64)]
    centre = (float(0.5 * (tp.longitude.min() + tp.longitude.max())), float(0.5 * (tp.latitude.min() + tp.latitude.max())))
    # rings out to the scene's farthest corner: every valid pixel is added
    reach = 111.2 * float(np.hypot((tp.longitude.max() - tp.longitude.min()) * np.cos(np.deg2rad(centre[1])), tp.latitude.max() - tp.latitude.min())) / 2.0

    variants, results = {}, {}

    def set_path(path):
        if path == "default":
            os.environ.pop("XSW_GRID_PATH", None)
        else:
            os.environ["XSW_GRID_PATH"] = path

    def polar_call(kind, t, dr_km, n_theta, path):
        spec = PolarSpec(centre, (dr_km, int(reach / dr_km) + 2), n_theta)
        cos_c, sin_c, bsin, bcos = spec.tables()
        bsin, bcos = put(bsin, np.float64), put(bcos, np.float64)
        sums = torch.zeros((6,) + spec.shape, dtype=torch.int64, device=dev)

        def run():
            set_path(path)
            ctx.wind_polar_raw(n, n, DEV, kind, p(t), None, len(tp.line), len(tp.sample), *(p(x) for x in tables), spec.lon_c, spec.lat_c, cos_c, sin_c,
                               spec.dr_km, spec.n_r, spec.n_theta, p(bsin), p(bcos), p(sums))
        return run, sums

    sources = (("complex128", _lib.CELLS_C128, wind), ("codes", _lib.CELLS_CODES, codes))
    for src, kind, t in sources:
        for pname in cases:
            for path in paths:
                name = f"{src} {pname} {path}"
                variants[name], results[name] = polar_call(kind, t, *POLAR[pname], path)
    if full:
        for pname, (dr_km, n_theta) in CROSSED.items():
            variants[f"complex128 {pname} lds"], results[f"complex128 {pname} lds"] = polar_call(_lib.CELLS_C128, wind, dr_km, n_theta, "lds")

    # beside them: k_wind_grid on 0.1 degree, both sources ...
    lon0, dlon, n_lon, lat0, dlat, n_lat = GRIDS["0.1"]
    grid_sums = {}
    for src, kind, t in sources:
        grid_sums[src] = torch.zeros((5, n_lat, n_lon), dtype=torch.int64, device=dev)

        def run(kind=kind, t=t, sums=grid_sums[src]):
            set_path("default")
            ctx.wind_grid_raw(n, n, DEV, kind, p(t), None, len(tp.line), len(tp.sample), *(p(x) for x in tables), lon0, dlon, n_lon, 0, lat0, dlat, n_lat,
                              p(sums))
        variants[f"k_wind_grid {src} 0.1"] = run
    # ... and k_ancillary_model (float64 model grid; the latitude axis descends: read backwards, as the public call does)
    tu, tv = put(mu[::-1], np.float64), put(mv[::-1], np.float64)
    out = torch.empty((n, n), dtype=torch.complex128, device=dev)
    mdlon, mdlat = float(mlon[-1] - mlon[0]) / (len(mlon) - 1), float(mlat[0] - mlat[-1]) / (len(mlat) - 1)
    variants["k_ancillary_model"] = lambda: ctx.ancillary_model_raw(n, n, DEV, F64, p(tu), p(tv), len(mlat), len(mlon), float(mlon[0]), mdlon, 0,
                                                                    float(mlat[-1]), mdlat, len(tp.line), len(tp.sample), *(p(x) for x in tables), p(out))

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

    if not full:  # a restricted run (counter collection): the times alone
        print(json.dumps({"workload": "polar", "raster": [n, n], "ms": {k: round(v, 3) for k, v in med.items()}}))
        return

    # every variant of one set of bins ran equally often: both paths and both sources hold the same sums
    reps = a.warmup + a.steps
    same, added, occupied = {}, {}, {}
    for pname in POLAR:
        ref = results[f"complex128 {pname} lds"]
        same[pname] = bool(all(torch.equal(results[f"{src} {pname} {path}"], ref) for src in ("complex128", "codes") for path in ("lds", "direct")))
        added[pname] = int(ref[0].sum().item()) // reps
        occupied[pname] = int((ref[0] > 0).sum().item())
    grid_added = int(grid_sums["complex128"][0].sum().item()) // reps
    res = {"workload": "polar", "raster": [n, n], "tie_grid": [len(tp.line), len(tp.sample)], "steps": a.steps, "warmup": a.warmup,
           "centre": list(centre), "bins": {k: [v[0], int(reach / v[0]) + 2, v[1]] for k, v in {**POLAR, **CROSSED}.items()}, "grid": list(GRIDS["0.1"]),
           "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "ratio_to_k_wind_grid": {f"{src} {pname}": round(med[f"{src} {pname} lds"] / med[f"k_wind_grid {src} 0.1"], 3)
                                    for src in ("complex128", "codes") for pname in POLAR},
           "ratio_to_k_ancillary_model": {k: round(med[k] / med["k_ancillary_model"], 3) for k in med if k.endswith(" lds") or k.startswith("k_wind_grid")},
           "lds_over_direct": {f"{src} {pname}": round(med[f"{src} {pname} lds"] / med[f"{src} {pname} direct"], 4)
                               for src in ("complex128", "codes") for pname in POLAR},
           "pixels_added_per_call": {**added, "grid 0.1": grid_added},
           "occupied_bins": {**occupied, **{k: int((results[f"complex128 {k} lds"][0] > 0).sum().item()) for k in CROSSED}},
           "paths_and_sources_give_equal_sums": same, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
