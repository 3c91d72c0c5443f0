"""Benchmark of the cost rasters from stored grid codes (k_cost_co / k_cost_cr, include/xsw.h: xsw_cost_from_codes,
xsw_cost_cr_from_codes) on bench.py's `--config 3` scene (20000 x 20000 float32 device rasters, the default CMOD5.N LUT + the
S1 VH GMF), float64 outputs (the public calls' default).  HIP events, median of warm repetitions, the variants alternating
inside one loop so that clock and thermal drift hit them alike.  Prints one JSON line and writes it to
profiles/cost_codes_bench.json:

  cost_J       `cost(parts=False)`: k_cost_co writing J alone           20 B read + 8 B written per pixel
  cost_parts   `cost(parts=True)`:  k_cost_co writing all four rasters  20 B read + 32 B written
  cost_dual    `cost_dual(parts=True)`, dsig_cr a raster: k_cost_cr     20 B read + 32 B written
  cross        k_cross_from_codes writing codes (the yardstick)         16 B read + 4 B written
  mono_codes   the co-pol search writing out_code_co (what a second search would cost)

Each cost pass also gathers ONE 8-byte LUT entry per pixel, which the byte counts above leave out: its effective traffic is
what this script is there to find out.  Reported per variant: milliseconds, the streamed bytes per pixel, their fraction of
the 8 TB/s HBM peak, and `vs_cross_scaled` = the time over the `cross` pass of the same run scaled by the ratio of bytes per
pixel (1.0: the streamed bytes explain the time; the excess is the gather and the float64 stores).  No threshold is set.

    python profiles/bench_cost_codes.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/cost_codes_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
BYTES = {"cost_J": 20 + 8, "cost_parts": 20 + 32, "cost_dual": 20 + 32, "cross": 16 + 4}  # streamed bytes per pixel, float32 rasters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cost_codes_bench.json"))
    a = ap.parse_args()

    import torch
    import bench  # the scene generator of the flagship benchmark (repository root)
    from xsarsea_amd import _lib
    from xsarsea_amd.windspeed import _engine, get_model

    n = a.size
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    ctx.upload_luts(co=bench.build_product_lut()[1], cr=_engine._cr_dict(get_model("gmf_s1_v2")._lut(units="dB")))
    inc, s_vv, anc = bench.make_scene(n, n, n, 0, 20260320 + 2, dev)
    s_vh, dsig = bench.make_crosspol(inc, anc, 777, dev)
    code_co = torch.empty((n, n), dtype=torch.int32, device=dev)
    code_cr = torch.empty((n, n), dtype=torch.int32, device=dev)
    outs = [torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE

    def mono_codes():
        ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code_co))

    def cross():
        ctx.cross_from_codes_raw(n, n, F32, F32, DEV, p(inc), p(code_co), p(s_vh), p(dsig), p(code_cr), None, dual_select=True)

    def cost_J():
        ctx.cost_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(s_vv), p(anc), p(outs[0]))

    def cost_parts():
        ctx.cost_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(s_vv), p(anc), *(p(o) for o in outs))

    def cost_dual():
        ctx.cost_cr_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(code_cr), p(s_vh), p(dsig), *(p(o) for o in outs))

    variants = {"mono_codes": mono_codes, "cross": cross, "cost_J": cost_J, "cost_parts": cost_parts, "cost_dual": cost_dual}
    mono_codes()  # (the codes the other passes read)
    cross()
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

    # what was timed is what the search minimised: J = Jwind + Jsig everywhere, finite wherever the code names a grid point
    cost_parts()
    ctx.synchronize()
    grid = code_co >= 0  # (int32 view: bit 31 clear)
    finite = bool(torch.isfinite(outs[0][grid]).all()) and bool(torch.isnan(outs[0][~grid]).all())
    additive = bool(torch.equal(outs[0][grid], outs[2][grid] + outs[1][grid]))
    searched = float(grid.float().mean())
    del grid

    res = {"workload": "cost_from_codes", "raster": [n, n], "scene": "bench.py --config 3", "out_dtype": "float64", "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "mono_codes_ms": round(med["mono_codes"], 3), "fraction_of_pixels_with_a_grid_code": round(searched, 4),
           "J_finite_exactly_on_grid_codes": finite, "J_equals_Jwind_plus_Jsig": additive}
    for k, b in BYTES.items():
        res[k] = {"ms": round(med[k], 3), "ms_all": [round(t, 3) for t in times[k]], "streamed_bytes_per_pixel": b,
                  "fraction_of_hbm_peak": round(b * n * n / (med[k] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
                  "vs_cross_scaled": round(med[k] / (med["cross"] * b / BYTES["cross"]), 3)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
