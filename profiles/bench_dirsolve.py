"""Benchmark of the wind direction at a known speed (k_dir_solve_co, include/xsw.h: xsw_dir_solve) on bench.py's `--config 3`
scene (20000 x 20000 float32 device rasters, the default CMOD5.N LUT), float64 outputs (the public call's default): the scene's
sigma0 in dB, the speed of its a-priori wind as the known speed and the direction of that wind (degrees(angle(anc)) as a float32
raster) as the reference direction.  Beside it, in the same run, the inverse along the speed axis and the forward operator as
yardsticks.  HIP events, median of warm repetitions, the variants alternating inside one loop so that clock and thermal drift hit
them alike.  Prints one JSON line and writes it to profiles/dirsolve_bench.json:

  eval_co        k_lut_eval_co writing sigma0_db alone (yardstick)          12 B read +  8 B written, eight LUT entries gathered
  solve_co       k_wspd_solve_co writing the speed alone (yardstick)        12 B read +  8 B written, four entries per bisection step
  dir_pair       k_dir_solve_co writing phi1 and phi2                       12 B read + 16 B written, four rows of n_phi entries walked
  dir_all        k_dir_solve_co writing all nine outputs                    16 B read + 58 B written

Reported per variant: milliseconds, the streamed bytes per pixel, their fraction of the 8 TB/s HBM peak, `vs_eval_co` and
`vs_solve_co` = its time over the yardsticks' in the same run; the shares of count 0 / 1 / 2 / more and of each flag.  No target is
set.

    python profiles/bench_dirsolve.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/dirsolve_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
BYTES = {"eval_co": 12 + 8, "solve_co": 12 + 8, "dir_pair": 12 + 16, "dir_all": 16 + 58}  # streamed bytes per pixel, float32 rasters, float64 outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dirsolve_bench.json"))
    a = ap.parse_args()

    import torch
    import bench  # the scene generator of the flagship benchmark (repository root)
    from xsarsea_amd import _lib

    n = a.size
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ctx.upload_luts(co=bench.build_product_lut()[1])
    inc, s_vv, anc = bench.make_scene(n, n, n, 0, 20260320 + 2, dev)
    s_db = (10 * torch.log10(s_vv + 1e-15)).to(torch.float32).contiguous()
    wspd = torch.abs(anc).to(torch.float32).contiguous()
    phi = torch.rad2deg(torch.angle(anc)).to(torch.float32).contiguous()
    del s_vv, anc
    outs = [torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(7)]
    count, flag = (torch.empty((n, n), dtype=torch.uint8, device=dev) for _ in range(2))
    p = lambda t: t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE
    torch.cuda.synchronize()

    def eval_co():
        ctx.lut_eval_raw(n, n, F32, F64, DEV, p(inc), p(wspd), p(phi), p(outs[0]))

    def solve_co():
        ctx.wspd_solve_raw(n, n, F32, F64, DEV, p(inc), p(s_db), p(phi), p(outs[0]))

    def dir_pair():
        ctx.dir_solve_raw(n, n, F32, F64, DEV, p(inc), p(s_db), p(wspd), None, p(outs[0]), p(outs[1]))

    def dir_all():
        ctx.dir_solve_raw(n, n, F32, F64, DEV, p(inc), p(s_db), p(wspd), p(phi), *(p(o) for o in outs), p(count), p(flag))

    variants = {"eval_co": eval_co, "solve_co": solve_co, "dir_pair": dir_pair, "dir_all": dir_all}
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
    med = {k: float(np.median(v)) for k, v in times.items()}

    # what was timed: the classes of the answer, and the selected direction against the a-priori one
    dir_all()
    ctx.synchronize()
    c, f = count[::4, ::4], flag[::4, ::4]
    share = lambda m: round(float(m.float().mean()), 5)
    classes = {"count_0": share(c == 0), "count_1": share(c == 1), "count_2": share(c == 2), "count_more": share(c > 2),
               "flag_nan": share(f == _lib.DIR_NAN), "flag_below": share(f == _lib.DIR_BELOW), "flag_above": share(f == _lib.DIR_ABOVE),
               "flag_more": share(f == _lib.DIR_MORE)}
    d = outs[4][::8, ::8] - phi[::8, ::8].double()
    d = torch.remainder(d + 180.0, 360.0) - 180.0
    d = d[torch.isfinite(d)]
    stats = {"median_abs_phi_near_minus_apriori_deg": round(float(d.abs().median()), 3),
             "median_abs_dphi_dsigma0_deg_per_db": round(float(outs[5][::8, ::8].abs().nanmedian()), 3)}

    res = {"workload": "dir_solve", "raster": [n, n], "scene": "bench.py --config 3: its sigma0, the speed and the direction of its a-priori wind",
           "out_dtype": "float64", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "variant": "plain (three float64 divisions per node; the screened variant was not built)", "classes": classes, "scene_stats": stats}
    for k in variants:
        res[k] = {"ms": round(med[k], 3), "ms_all": [round(t, 3) for t in times[k]], "vs_eval_co": round(med[k] / med["eval_co"], 3),
                  "vs_solve_co": round(med[k] / med["solve_co"], 3), "streamed_bytes_per_pixel": BYTES[k],
                  "fraction_of_hbm_peak": round(BYTES[k] * n * n / (med[k] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
