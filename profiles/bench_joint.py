"""Benchmark of the joint dual-pol inversion from stored co-pol codes (k_joint_from_codes, include/xsw.h: xsw_joint_from_codes;
DESIGN.md section 19) on bench.py's `--config 3` scene (float32 device rasters, CMOD5.N + S1 VH GMF).  HIP events, median of warm
repetitions, the three passes alternating inside one loop so that clock and thermal drift hit them alike.  Prints one JSON line
and writes it to profiles/joint_bench.json:

  mono_codes   the co-pol search that produces the codes (the mono xsw_invert chain writing out_code_co)
  cross        k_cross_from_codes on those codes (the two-step scheme's second step)
  joint        k_joint_from_codes on those codes, writing the joint codes

and, from one more joint pass with the statistics counters on (xsw_stats_enable), the mean number of candidates scored per
searched pixel, and the share of searched pixels whose joint grid point differs from the co-pol one.  --size is the side of the
square raster: the default is the largest at which one repetition of the joint pass stays under about two seconds on an MI355X.
The script sets no threshold.

    python profiles/bench_joint.py [--size 7000] [--steps 7] [--warmup 2] [--out profiles/joint_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=7000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "joint_bench.json"))
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
    code_joint = torch.empty((n, n), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    F32, DEV = _lib.XSW_F32, _lib.MEM_DEVICE

    def mono_codes():
        ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code_co))

    def cross():
        ctx.cross_from_codes_raw(n, n, F32, F32, DEV, p(inc), p(code_co), p(s_vh), p(dsig), p(code_cr), None, dual_select=True)

    def joint():
        ctx.joint_from_codes_raw(n, n, F32, F32, DEV, p(inc), p(code_co), p(s_vv), p(anc), p(s_vh), p(dsig), p(code_joint))

    variants = {"mono_codes": mono_codes, "cross": cross, "joint": joint}
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.steps):  # alternating: one repetition of every pass per round
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}

    ctx.stats_enable(True)  # one more joint pass, counting (the counters are vector atomics, one pair per wave)
    joint()
    st = ctx.stats()
    ctx.stats_enable(False)
    searched = (code_joint >= 0) & (code_co >= 0)  # bit 31 clear in both
    moved = searched & (((code_joint ^ code_co) & 0x3FFFFFFF) != 0)
    n_searched = int(searched.sum().item())

    res = {"workload": "joint_from_codes", "raster": [n, n], "scene": "bench.py --config 3", "steps": a.steps, "warmup": a.warmup,
           "k_joint_from_codes_ms": round(med["joint"], 3), "k_joint_from_codes_ms_all": [round(t, 3) for t in times["joint"]],
           "k_joint_from_codes_mpx_s": round(n * n / med["joint"] / 1e3, 3),
           "mono_codes_ms": round(med["mono_codes"], 3), "mono_codes_mpx_s": round(n * n / med["mono_codes"] / 1e3, 3),
           "k_cross_from_codes_ms": round(med["cross"], 3), "k_cross_from_codes_mpx_s": round(n * n / med["cross"] / 1e3, 3),
           "pixels_searched": st["pixels_co"], "candidates_scored": st["cand_co"],
           "candidates_per_searched_pixel": round(st["cand_co"] / max(st["pixels_co"], 1), 1),
           "candidates_per_second": round(st["cand_co"] / (med["joint"] * 1e-3), 0),
           "share_joint_point_differs_from_copol": round(int(moved.sum().item()) / max(n_searched, 1), 4),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
