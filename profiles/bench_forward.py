"""Benchmark of the forward operator on rasters (k_lut_eval_co / k_lut_eval_cr, include/xsw.h: xsw_lut_eval, xsw_lut_eval_cr) on
bench.py's `--config 3` scene (20000 x 20000 float32 device rasters, the default CMOD5.N LUT + the S1 VH GMF), float64 outputs
(the public call's default), evaluated at the scene's a-priori wind (|anc| and degrees(angle(anc)) as float32 rasters), beside
the cost pass of DESIGN section 13 as the yardstick.  HIP events, median of warm repetitions, the variants alternating inside one
loop so that clock and thermal drift hit them alike.  Prints one JSON line and writes it to profiles/forward_bench.json:

  cost_parts   k_cost_co writing all four rasters (the yardstick)     20 B read + 32 B written, ONE 8-byte LUT entry gathered
  eval_co      k_lut_eval_co writing sigma0_db alone                  12 B read +  8 B written, EIGHT entries gathered as four
               adjacent pairs in two incidence planes, seven IEEE divisions
  eval_co_jac  k_lut_eval_co writing sigma0_db, dwspd and dphi        12 B read + 24 B written, eight divisions
  eval_cr      k_lut_eval_cr writing sigma0_db                         8 B read +  8 B written, four entries, three divisions

Reported per variant: milliseconds, the streamed bytes per pixel, their fraction of the 8 TB/s HBM peak, and `vs_cost_parts` =
its time over k_cost_co's in the same run.  No target is set.

    python profiles/bench_forward.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/forward_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
BYTES = {"cost_parts": 20 + 32, "eval_co": 12 + 8, "eval_co_jac": 12 + 24, "eval_cr": 8 + 8}  # streamed bytes per pixel, float32 rasters, float64 outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forward_bench.json"))
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
    wspd = torch.abs(anc).to(torch.float32).contiguous()
    phi = torch.rad2deg(torch.angle(anc)).to(torch.float32).contiguous()
    code_co = torch.empty((n, n), dtype=torch.int32, device=dev)
    outs = [torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE

    def cost_parts():
        ctx.cost_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code_co), p(s_vv), p(anc), *(p(o) for o in outs))

    def eval_co():
        ctx.lut_eval_raw(n, n, F32, F64, DEV, p(inc), p(wspd), p(phi), p(outs[0]))

    def eval_co_jac():
        ctx.lut_eval_raw(n, n, F32, F64, DEV, p(inc), p(wspd), p(phi), p(outs[0]), p(outs[1]), p(outs[2]))

    def eval_cr():
        ctx.lut_eval_cr_raw(n, n, F32, F64, DEV, p(inc), p(wspd), p(outs[3]))

    # the codes the yardstick reads: the co-pol search
    ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code_co))
    variants = {"cost_parts": cost_parts, "eval_co": eval_co, "eval_co_jac": eval_co_jac, "eval_cr": eval_cr}
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

    # what was timed is a simulation: the finite shares, and sigma0 at the a-priori wind against the observation
    eval_co_jac()
    eval_cr()
    ctx.synchronize()
    finite = {"co": round(float(torch.isfinite(outs[0]).float().mean()), 5), "cr": round(float(torch.isfinite(outs[3]).float().mean()), 5)}
    consistent = bool((torch.isfinite(outs[0]) == torch.isfinite(outs[1])).all()) and bool((torch.isfinite(outs[0]) == torch.isfinite(outs[2])).all())
    obs_db = 10 * torch.log10(s_vv[::8, ::8].double() + 1e-15)
    d = (obs_db - outs[0][::8, ::8])
    d = d[torch.isfinite(d)]
    stats = {"median_obs_minus_sim_db": round(float(d.median()), 4), "median_abs_dwspd_db_per_m_s": round(float(outs[1][::8, ::8].abs().nanmedian()), 4),
             "median_abs_dphi_db_per_deg": round(float(outs[2][::8, ::8].abs().nanmedian()), 5)}

    res = {"workload": "lut_eval", "raster": [n, n], "scene": "bench.py --config 3, evaluated at its a-priori wind", "out_dtype": "float64",
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "finite_shares": finite, "jacobian_finite_exactly_where_sigma0_is": consistent, "scene_stats": stats}
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
