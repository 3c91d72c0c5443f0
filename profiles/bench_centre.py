"""Benchmark of xsarsea_amd.centre (k_wind_centre, csrc/xsw_cells.hip) on a 20000 x 20000 raster: the scene, the two sources
(co-pol grid codes and their complex128 expansion) and the tie grid of bench_polar.py, the first guess in the middle of the scene.
HIP events, median of warm repetitions, the variants taking turns inside every repetition.  Prints one JSON line and writes it to
profiles/centre_bench.json:

  - xsw_wind_centre on lattices of 9 x 9, 17 x 17 and 31 x 31 candidates, 0.25 km apart, for the annulus 1 .. 2.5 km, from
    complex128 winds and from codes, each staged (the default) and with XSW_CENTRE_PATH=direct
  - beside them, in the same run: k_wind_polar in rings of 2 km with 4 sectors from both sources: one pass of the kernel a search
    without this entry would run once per candidate
  - the share of the pixels that the staged path's cull lets through (counted on every 8th line and sample), the pairs of pixel
    and candidate per second that its sweep examines, the hits per second, and the candidates one wind_polar pass pays for

    python profiles/bench_centre.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/centre_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_ancillary_model import scene  # noqa: E402  (same folder)

LATTICES = (9, 17, 31)
STEP_KM, ANNULUS = 0.25, (1.0, 2.5)
POLAR = (2.0, 4)
R_KM, D2R = 6371.0088, 0.017453292519943295


def staged_share(tp, spec, wind, n, every=8):
    """The share of all pixels that are valid and lie inside the cull square of `spec`, counted on every `every`-th line and
    sample: the tie blend and the chart of include/xsw.h in numpy."""
    from xsarsea_amd import streaks as S
    line, sample = np.arange(0, n, every, dtype=np.float64), np.arange(0, n, every, dtype=np.float64)
    (lf, lt), (sf, st) = S.bracket(tp.line, line), S.bracket(tp.sample, sample)
    l1, s1 = np.minimum(lf + 1, len(tp.line) - 1), np.minimum(sf + 1, len(tp.sample) - 1)

    def tie(f):
        r0 = (1.0 - st) * f[lf][:, sf] + st * f[lf][:, s1]
        r1 = (1.0 - st) * f[l1][:, sf] + st * f[l1][:, s1]
        return (1.0 - lt)[:, None] * r0 + lt[:, None] * r1
    lon, lat = tie(tp.longitude), tie(tp.latitude)
    cos_g, sin_g = spec.tables()
    dl = lon - spec.lon_g
    dl = dl - 360.0 * np.rint(dl / 360.0)
    dy = (lat - spec.lat_g) * D2R
    h = 0.5 * dy
    x, y = (R_KM * D2R * dl) * ((cos_g - sin_g * h) - (0.5 * cos_g) * (h * h)), R_KM * dy
    bound = (spec.n - 1) // 2 * spec.step_km + spec.r_out_km
    valid = ~np.isnan(wind[::every, ::every].real.cpu().numpy())
    return float((valid & (np.abs(x) < bound) & (np.abs(y) < bound)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "centre_bench.json"))
    a = ap.parse_args()

    import torch
    import bench  # the scene generator of the flagship benchmark (repository root)
    from xsarsea_amd import TiePoints, _lib, streaks as S
    from xsarsea_amd.centre import CentreSpec
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

    tie_line, tie_sample, lon, lat, heading = scene(n)[:5]
    tp = TiePoints(tie_line, tie_sample, lon, lat, heading)
    put = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    lf, lt = S.bracket(tp.line, np.arange(n))
    sf, st = S.bracket(tp.sample, np.arange(n))
    tables = [put(x, np.float64) for x in (tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading)]
    tables += [put(lf, np.int32), put(lt, np.float64), put(sf, np.int32), put(st, np.float64)]
    guess = (float(0.5 * (tp.longitude.min() + tp.longitude.max())), float(0.5 * (tp.latitude.min() + tp.latitude.max())))

    variants, results, specs = {}, {}, {}

    def set_path(path):
        if path == "staged":
            os.environ.pop("XSW_CENTRE_PATH", None)
        else:
            os.environ["XSW_CENTRE_PATH"] = path

    def centre_call(kind, t, n_c, path):
        spec = CentreSpec(guess, STEP_KM, n_c, ANNULUS)
        cos_g, sin_g = spec.tables()
        sums = torch.zeros((5,) + spec.shape, dtype=torch.int64, device=dev)

        def run():
            set_path(path)
            ctx.wind_centre_raw(n, n, DEV, kind, p(t), None, len(tp.line), len(tp.sample), *(p(x) for x in tables), spec.lon_g, spec.lat_g, cos_g, sin_g,
                                spec.step_km, spec.n, spec.r_in_km, spec.r_out_km, p(sums))
        return run, sums, spec

    sources = (("complex128", _lib.CELLS_C128, wind), ("codes", _lib.CELLS_CODES, codes))
    for src, kind, t in sources:
        for n_c in LATTICES:
            for path in ("staged", "direct"):
                name = f"{src} n={n_c} {path}"
                variants[name], results[name], specs[n_c] = centre_call(kind, t, n_c, path)

    # beside them: one k_wind_polar pass around the first guess, rings out to the scene's farthest corner
    reach = 111.2 * float(np.hypot((tp.longitude.max() - tp.longitude.min()) * np.cos(np.deg2rad(guess[1])), tp.latitude.max() - tp.latitude.min())) / 2.0
    pspec = PolarSpec(guess, (POLAR[0], int(reach / POLAR[0]) + 2), POLAR[1])
    cos_c, sin_c, bsin, bcos = pspec.tables()
    bsin, bcos = put(bsin, np.float64), put(bcos, np.float64)
    for src, kind, t in sources:
        psums = torch.zeros((6,) + pspec.shape, dtype=torch.int64, device=dev)

        def run(kind=kind, t=t, psums=psums):
            os.environ.pop("XSW_GRID_PATH", None)
            ctx.wind_polar_raw(n, n, DEV, kind, p(t), None, len(tp.line), len(tp.sample), *(p(x) for x in tables), pspec.lon_c, pspec.lat_c, cos_c, sin_c,
                               pspec.dr_km, pspec.n_r, pspec.n_theta, p(bsin), p(bcos), p(psums))
        variants[f"k_wind_polar {src} 2km x 4"] = run

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
    os.environ.pop("XSW_CENTRE_PATH", None)
    med = {k: float(np.median(v)) for k, v in times.items()}

    # every variant of one lattice ran equally often: both paths and both sources hold the same sums
    reps = a.warmup + a.steps
    same, hits, share = {}, {}, {}
    for n_c in LATTICES:
        ref = results[f"complex128 n={n_c} staged"]
        same[str(n_c)] = bool(all(torch.equal(results[f"{src} n={n_c} {path}"], ref) for src in ("complex128", "codes") for path in ("staged", "direct")))
        hits[n_c] = int(ref[0].sum().item()) // reps
        share[n_c] = staged_share(tp, specs[n_c], wind, n)
    pairs = {n_c: share[n_c] * n * n * n_c * n_c for n_c in LATTICES}
    res = {"workload": "centre", "raster": [n, n], "tie_grid": [len(tp.line), len(tp.sample)], "steps": a.steps, "warmup": a.warmup,
           "first_guess": list(guess), "step_km": STEP_KM, "annulus_km": list(ANNULUS), "lattices": list(LATTICES), "polar_bins": [POLAR[0], pspec.n_r, POLAR[1]],
           "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "staged_over_direct": {f"{src} n={n_c}": round(med[f"{src} n={n_c} staged"] / med[f"{src} n={n_c} direct"], 5)
                                  for src in ("complex128", "codes") for n_c in LATTICES},
           "staged_over_one_polar_pass": {f"{src} n={n_c}": round(med[f"{src} n={n_c} staged"] / med[f"k_wind_polar {src} 2km x 4"], 3)
                                          for src in ("complex128", "codes") for n_c in LATTICES},
           "candidates_per_polar_pass": {f"{src} n={n_c}": round(n_c * n_c * med[f"k_wind_polar {src} 2km x 4"] / med[f"{src} n={n_c} staged"], 1)
                                         for src in ("complex128", "codes") for n_c in LATTICES},
           "share_of_pixels_staged": {str(k): round(v, 6) for k, v in share.items()},
           "pairs_examined_per_call": {str(k): int(v) for k, v in pairs.items()},
           "pairs_per_second_staged": {f"{src} n={n_c}": float(f"{pairs[n_c] / (med[f'{src} n={n_c} staged'] * 1e-3):.4g}")
                                       for src in ("complex128", "codes") for n_c in LATTICES},
           "hits_per_call": {str(k): v for k, v in hits.items()},
           "hits_per_second": {f"{src} n={n_c} {path}": float(f"{hits[n_c] / (med[f'{src} n={n_c} {path}'] * 1e-3):.4g}")
                               for src in ("complex128", "codes") for n_c in LATTICES for path in ("staged", "direct")},
           "paths_and_sources_give_equal_sums": same, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
