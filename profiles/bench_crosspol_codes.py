"""Benchmark of the cross-pol step from stored co-pol codes (k_cross_from_codes, include/xsw.h: xsw_cross_from_codes) against the
fused dual-pol launch, on bench.py's `--config 3` scene (20000 x 20000 float32, CMOD5.N + S1 VH GMF, dual select on).  HIP events,
median of warm repetitions, the variants alternating inside one loop so that clock and thermal drift hit them alike.  Prints one
JSON line and writes it to profiles/crosspol_codes_bench.json:

  (a) fused        one dual-pol xsw_invert writing the two complex64 rasters (what bench.py --config 3 times)
  (b) split        the mono co-pol chain writing out_code_co, then k_cross_from_codes writing out_code_cr
  (c) cross alone  k_cross_from_codes writing codes, against its 20 B per pixel (16 read, 4 written) and the 8 TB/s HBM peak

(a) as a yardstick for a tree under test is taken AT THE PARENT COMMIT with this script's `--fused-only`; the figure of (a)
printed by a full run is the tree's own.  The script sets no threshold.

    python profiles/bench_crosspol_codes.py [--size 20000] [--steps 7] [--warmup 2] [--fused-only] [--out profiles/crosspol_codes_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fused-only", action="store_true", help="variant (a) alone: what a parent commit without the new entry can run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crosspol_codes_bench.json"))
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
    out_co = torch.empty((n, n), dtype=torch.complex64, device=dev)
    out_dual = torch.empty((n, n), dtype=torch.complex64, device=dev)
    code_co = torch.empty((n, n), dtype=torch.int32, device=dev)
    code_cr = torch.empty((n, n), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()
    F32, DEV = _lib.XSW_F32, _lib.MEM_DEVICE

    def fused():
        ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), p(s_vh), p(dsig), p(anc), p(out_co), p(out_dual), algo=_lib.ALGO_PRUNED, dual_select=True)

    def mono_codes():
        ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(code_co))

    def cross():
        ctx.cross_from_codes_raw(n, n, F32, F32, DEV, p(inc), p(code_co), p(s_vh), p(dsig), p(code_cr), None, dual_select=True)

    def split():
        mono_codes()
        cross()

    variants = {"fused": fused} if a.fused_only else {"fused": fused, "split": split, "mono_codes": mono_codes, "cross": cross}
    if not a.fused_only:
        mono_codes()  # (the codes `cross` alone reads)
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

    res = {"workload": "crosspol_from_codes", "raster": [n, n], "scene": "bench.py --config 3", "steps": a.steps, "warmup": a.warmup,
           "fused_dual_ms": round(med["fused"], 3), "fused_dual_ms_all": [round(t, 3) for t in times["fused"]],
           "fused_dual_gpx_s": round(n * n / med["fused"] / 1e6, 3), "device": torch.cuda.get_device_name(0)}
    if not a.fused_only:
        # the split answer is the fused one: every cross-pol code expands to the fused launch's wind_dual
        fused()
        split()
        chk = torch.empty((n, n), dtype=torch.complex64, device=dev)
        ctx.expand_codes_raw(n * n, DEV, F32, p(code_co), p(code_cr), None, p(chk))
        ctx.synchronize()
        same = bool(torch.equal(torch.view_as_real(chk).view(torch.int32), torch.view_as_real(out_dual).view(torch.int32)))
        res.update({
            "split_ms": round(med["split"], 3), "split_ms_all": [round(t, 3) for t in times["split"]],
            "split_gpx_s": round(n * n / med["split"] / 1e6, 3),
            "mono_codes_ms": round(med["mono_codes"], 3), "k_cross_from_codes_ms": round(med["cross"], 3),
            "k_cross_from_codes_ms_all": [round(t, 3) for t in times["cross"]], "k_cross_from_codes_bytes": 20 * n * n,
            "k_cross_from_codes_fraction_of_hbm_peak": round(20 * n * n / (med["cross"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
            "split_equals_fused_bit_for_bit": same})
    line = json.dumps(res)
    if a.out and not a.fused_only:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
