"""Benchmark of the error bars of the joint dual-pol solution from stored grid codes (k_unc_joint, include/xsw.h:
xsw_uncertainty_joint_from_codes) on bench.py's `--config 3` scene (20000 x 20000 float32 device rasters, the
default CMOD5.N LUT + the S1 VH GMF, dsig_cr a raster), float64 outputs (the public call's default), beside k_unc_co, the co-pol
pass whose stencil it extends.  HIP events, median of warm repetitions, every call of k_unc_joint alternating with k_unc_co inside
one loop so that clock and thermal drift hit them alike.  Prints one JSON line and writes it to
profiles/uncertainty_joint_bench.json:

  unc_co       k_unc_co writing wspd_std, dir_std, corr and the flag (the yardstick)   20 B read + 25 B written
  joint_polar  k_unc_joint writing the same four outputs                               28 B read + 25 B written
  joint_all    k_unc_joint writing all six real outputs and the flag                   28 B read + 49 B written
  joint_flag   k_unc_joint writing the flag alone                                      28 B read +  1 B written

The input codes are the co-pol search's: the pass does the same work for any grid code, and a joint search of this raster would
take a quarter of a minute.  Reported per variant: milliseconds, its time over k_unc_co's of the same run, the streamed bytes
per pixel (a reading of the code, as is the gather count) and their fraction of the 8 TB/s HBM peak; and from the outputs the
share of pixels with an estimate and the median joint and co-pol wspd_std.  No target is set.

    python profiles/bench_uncertainty_joint.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/uncertainty_joint_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
BYTES = {"unc_co": 20 + 25, "joint_polar": 28 + 25, "joint_all": 28 + 49, "joint_flag": 28 + 1}  # streamed per pixel: float32 rasters, float64 outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "uncertainty_joint_bench.json"))
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
    code = torch.empty((n, n), dtype=torch.int32, device=dev)
    outs = [torch.empty((n, n), dtype=torch.float64, device=dev) for _ in range(6)]
    flag = torch.empty((n, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE

    def unc_co():
        ctx.uncertainty_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code), p(s_vv), p(anc), p(outs[0]), p(outs[1]), p(outs[2]), p(flag))

    def joint(polar, uv):
        o = [p(t) if on else None for t, on in zip(outs, [polar] * 3 + [uv] * 3)]
        ctx.uncertainty_joint_from_codes_raw(n, n, F32, F64, DEV, p(inc), p(code), p(s_vv), p(anc), p(s_vh), p(dsig), *o, p(flag))

    ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code))
    variants = {"joint_polar": lambda: joint(True, False), "joint_all": lambda: joint(True, True), "joint_flag": lambda: joint(False, False)}
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
            unc_co()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {k: [] for k in BYTES}
    for _ in range(a.steps):  # alternating: every call of k_unc_joint is followed by one of k_unc_co
        for k, fn in variants.items():
            times[k].append(timed(fn))
            times["unc_co"].append(timed(unc_co))
    med = {k: float(np.median(v)) for k, v in times.items()}

    # what was timed gives estimates: the flag classes, finite positive deviations exactly where no NaN bit is set, and the medians
    unc_co()
    ctx.synchronize()
    ok_co = flag == 0
    share_co, med_co = float(ok_co.float().mean()), float(outs[0][ok_co].median())
    del ok_co
    joint(True, True)
    ctx.synchronize()
    classes = {str(v): round(float((flag == v).float().mean()), 5) for v in (0, 1, 2, 4, 6, 8, 16, 17, 18, 20, 22, 24)}
    ok = (flag & 15) == 0
    consistent = bool((torch.isfinite(outs[0][ok]) & (outs[0][ok] > 0) & (outs[1][ok] > 0) & (outs[2][ok].abs() < 1)).all()) \
        and bool((torch.isfinite(outs[3][ok]) & torch.isfinite(outs[4][ok]) & (outs[5][ok].abs() <= 1)).all()) and bool(torch.isnan(outs[3][~ok]).all())
    medians = {"wspd_std_m_s": round(float(outs[0][ok].median()), 4), "dir_std_deg": round(float(outs[1][ok].median()), 3),
               "u_std_m_s": round(float(outs[3][ok].median()), 4), "v_std_m_s": round(float(outs[4][ok].median()), 4)}
    share = float(ok.float().mean())
    del ok

    res = {"workload": "uncertainty_joint_from_codes", "raster": [n, n], "scene": "bench.py --config 3", "input_codes": "co-pol search (xsw_invert)",
           "out_dtype": "float64", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_gb_s": HBM_PEAK_GBS,
           "flag_shares_joint": classes, "share_with_an_estimate": {"joint": round(share, 5), "co_pol": round(share_co, 5)},
           "medians_where_estimated_joint": medians, "median_wspd_std_co_pol_m_s": round(med_co, 4),
           "finite_exactly_where_estimated": consistent,
           "measured": ["ms", "ms_all", "vs_unc_co", "fraction_of_hbm_peak (from ms)", "shares", "medians"],
           "read_from_the_code": ["streamed_bytes_per_pixel"]}
    for k, b in BYTES.items():
        res[k] = {"ms": round(med[k], 3), "ms_all": [round(t, 3) for t in times[k]], "streamed_bytes_per_pixel": b,
                  "fraction_of_hbm_peak": round(b * n * n / (med[k] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
                  "vs_unc_co": round(med[k] / med["unc_co"], 3)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
