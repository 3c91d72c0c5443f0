"""Benchmark of the wind speed at a known direction (k_wspd_solve_co / k_wspd_solve_cr, include/xsw.h: xsw_wspd_solve,
xsw_wspd_solve_cr) on bench.py's `--config 3` scene (20000 x 20000 float32 device rasters, the default CMOD5.N LUT + the S1 VH
GMF), float64 outputs (the public call's default): the scene's sigma0 in dB and the direction of its a-priori wind
(degrees(angle(anc)) as a float32 raster); the cross-pol kernel reads the VH table's own sigma0 at the a-priori speed
(k_lut_eval_cr, rounded to float32), since the scene has no cross-pol channel.  Beside them, in the same run, the forward operator
and the co-pol search as yardsticks.  HIP events, median of warm repetitions, the variants alternating inside one loop so that
clock and thermal drift hit them alike.  Prints one JSON line and writes it to profiles/solve_bench.json:

  eval_co        k_lut_eval_co writing sigma0_db alone (the yardstick)    12 B read +  8 B written, eight LUT entries gathered
  solve_co       k_wspd_solve_co writing the speed alone                  12 B read +  8 B written, four entries per bisection step
  solve_co_all   k_wspd_solve_co writing speed, sensitivity and flag      12 B read + 17 B written
  solve_cr       k_wspd_solve_cr writing speed, sensitivity and flag       8 B read + 17 B written, two entries per step
  search_co      the co-pol Bayesian search (xsw_invert, pruned, codes out): what produced a speed before this call existed

Reported per variant: milliseconds, and for the raster passes the streamed bytes per pixel, their fraction of the 8 TB/s HBM peak
and `vs_eval_co` = its time over k_lut_eval_co's in the same run; the shares of TAIL and no-solution pixels.  No target is set.

    python profiles/bench_solve.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/solve_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
BYTES = {"eval_co": 12 + 8, "solve_co": 12 + 8, "solve_co_all": 12 + 17, "solve_cr": 8 + 17}  # streamed bytes per pixel, float32 rasters, float64 outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "solve_bench.json"))
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
    s_db = (10 * torch.log10(s_vv + 1e-15)).to(torch.float32).contiguous()
    wspd = torch.abs(anc).to(torch.float32).contiguous()
    phi = torch.rad2deg(torch.angle(anc)).to(torch.float32).contiguous()
    code_co = torch.empty((n, n), dtype=torch.int32, device=dev)
    outs = [torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(3)]
    flag = torch.empty((n, n), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE
    s_cr_db = torch.empty((n, n), dtype=torch.float32, device=dev)
    ctx.lut_eval_cr_raw(n, n, F32, F32, DEV, p(inc), p(wspd), p(s_cr_db))
    ctx.synchronize()
    torch.cuda.synchronize()

    def eval_co():
        ctx.lut_eval_raw(n, n, F32, F64, DEV, p(inc), p(wspd), p(phi), p(outs[2]))

    def solve_co():
        ctx.wspd_solve_raw(n, n, F32, F64, DEV, p(inc), p(s_db), p(phi), p(outs[0]))

    def solve_co_all():
        ctx.wspd_solve_raw(n, n, F32, F64, DEV, p(inc), p(s_db), p(phi), p(outs[0]), p(outs[1]), p(flag))

    def solve_cr():
        ctx.wspd_solve_cr_raw(n, n, F32, F64, DEV, p(inc), p(s_cr_db), p(outs[0]), p(outs[1]), p(flag))

    def search_co():
        ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code_co))

    variants = {"eval_co": eval_co, "solve_co": solve_co, "solve_co_all": solve_co_all, "solve_cr": solve_cr, "search_co": search_co}
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

    # what was timed: the classes of the answer, and the retrieved speed against the a-priori one
    def shares():
        ctx.synchronize()
        f = flag[::4, ::4]
        return {"solved_leading_rows": round(float((f == 0).float().mean()), 5), "tail": round(float((f == _lib.SOLVE_TAIL).float().mean()), 5),
                "below": round(float((f == _lib.SOLVE_BELOW).float().mean()), 5), "above": round(float((f == _lib.SOLVE_ABOVE).float().mean()), 5),
                "nan": round(float((f == _lib.SOLVE_NAN).float().mean()), 5)}

    solve_cr()
    classes = {"cr": shares()}
    solve_co_all()
    classes["co"] = shares()
    d = (outs[0][::8, ::8] - wspd[::8, ::8].double())
    d = d[torch.isfinite(d)]
    stats = {"median_wspd_minus_apriori_m_s": round(float(d.median()), 4), "median_abs_wspd_minus_apriori_m_s": round(float(d.abs().median()), 4),
             "median_abs_dwspd_dsigma0_m_s_per_db": round(float(outs[1][::8, ::8].abs().nanmedian()), 4)}

    res = {"workload": "wspd_solve", "raster": [n, n], "scene": "bench.py --config 3: its sigma0 and the direction of its a-priori wind",
           "out_dtype": "float64", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "classes": classes, "scene_stats": stats}
    for k in variants:
        res[k] = {"ms": round(med[k], 3), "ms_all": [round(t, 3) for t in times[k]], "vs_eval_co": round(med[k] / med["eval_co"], 3)}
        if k in BYTES:
            res[k].update(streamed_bytes_per_pixel=BYTES[k], fraction_of_hbm_peak=round(BYTES[k] * n * n / (med[k] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4))
    res["solve_co_vs_search_co"] = round(med["solve_co"] / med["search_co"], 3)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
