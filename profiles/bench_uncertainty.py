"""Benchmark of the wind-uncertainty rasters from stored grid codes (k_unc_co / k_unc_cr, include/xsw.h:
xsw_uncertainty_from_codes, xsw_uncertainty_cr_from_codes) on bench.py's `--config 3` scene (20000 x 20000 float32 device
rasters, the default CMOD5.N LUT + the S1 VH GMF), float64 outputs (the public calls' default), beside the cost pass they
share their J with.  HIP events, median of warm repetitions, the variants alternating inside one loop so that clock and
thermal drift hit them alike.  Prints one JSON line and writes it to profiles/uncertainty_bench.json:

  cost_parts  k_cost_co writing all four rasters (the yardstick)       20 B read + 32 B written, ONE 8-byte LUT entry gathered
  unc_co      k_unc_co writing wspd_std, dir_std, corr and the flag    20 B read + 25 B written, NINE entries gathered as three
              24-byte runs phi_pad * 8 = 1472 bytes apart in the default table
  unc_cr      k_unc_cr writing wspd_std and the flag, dsig_cr a raster 20 B read + 9 B written, one 24-byte run gathered

Reported per variant: milliseconds, the streamed bytes per pixel, their fraction of the 8 TB/s HBM peak, and
`vs_cost_parts` = its time over k_cost_co's in the same run: what nine gathers cost where one was measured.  No target is set.

    python profiles/bench_uncertainty.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/uncertainty_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
BYTES = {"cost_parts": 20 + 32, "unc_co": 20 + 25, "unc_cr": 20 + 9}  # streamed bytes per pixel, float32 rasters, float64 outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "uncertainty_bench.json"))
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
    flag = torch.empty((n, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE

    def cost_parts():
        ctx.cost_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(s_vv), p(anc), *(p(o) for o in outs))

    def unc_co():
        ctx.uncertainty_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(s_vv), p(anc), p(outs[0]), p(outs[1]), p(outs[2]), p(flag))

    def unc_cr():
        ctx.uncertainty_cr_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(code_cr), p(s_vh), p(dsig), p(outs[3]), p(flag))

    # the codes the passes read: the co-pol search, then the cross-pol step from its codes
    ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code_co))
    ctx.cross_from_codes_raw(n, n, F32, F32, DEV, p(inc), p(code_co), p(s_vh), p(dsig), p(code_cr), None, dual_select=True)
    variants = {"cost_parts": cost_parts, "unc_co": unc_co, "unc_cr": unc_cr}
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

    # what was timed gives estimates: the flag classes, and finite positive deviations exactly where the flag is 0
    unc_co()
    ctx.synchronize()
    classes = {str(v): round(float((flag == v).float().mean()), 5) for v in (0, 1, 2, 4, 6, 8)}
    ok = flag == 0
    consistent = bool((torch.isfinite(outs[0][ok]) & (outs[0][ok] > 0) & (outs[1][ok] > 0) & (outs[2][ok].abs() < 1)).all()) and bool(torch.isnan(outs[0][~ok]).all())
    medians = {"wspd_std_m_s": round(float(outs[0][ok].median()), 4), "dir_std_deg": round(float(outs[1][ok].median()), 3)}
    del ok
    unc_cr()
    ctx.synchronize()
    classes_cr = {str(v): round(float((flag == v).float().mean()), 5) for v in (0, 1, 2, 8)}

    res = {"workload": "uncertainty_from_codes", "raster": [n, n], "scene": "bench.py --config 3", "out_dtype": "float64", "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "flag_shares_co": classes, "flag_shares_cr": classes_cr, "medians_where_flag_0": medians,
           "finite_exactly_where_flag_0": consistent}
    for k, b in BYTES.items():
        res[k] = {"ms": round(med[k], 3), "ms_all": [round(t, 3) for t in times[k]], "streamed_bytes_per_pixel": b,
                  "fraction_of_hbm_peak": round(b * n * n / (med[k] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
                  "vs_cost_parts": round(med[k] / med["cost_parts"], 3)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
