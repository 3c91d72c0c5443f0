"""Benchmark of xsarsea_amd.cells (k_cells, csrc/xsw_cells.hip) on a 20000 x 20000 raster: the flagship scene inverted to co-pol
grid codes, their complex128 expansion and its float32 speed as the three sources.  HIP events, median of warm repetitions, the
variants taking turns inside every repetition.  Prints one JSON line and writes it to profiles/cells_bench.json:

  - xsw_wind_cells from complex128 winds (16 B read per pixel) and from codes (4 B), xsw_raster_cells from float32 (4 B), at
    cells of 100 x 100, 10 x 10 and 1000 x 1000 pixels, each in both forced mappings (XSW_CELLS_MAPPING = wave / workgroup), and
    complex128 with a keep mask (+ 1 B) at 100 x 100; a sweep of cell sizes between 16 x 16 and 300 x 300 for the threshold
    XSW_CELLS_WG_AREA; each as a fraction of the 8 TB/s HBM peak from the bytes read
  - what the pass replaces, in the same run: k_expand (codes -> complex128 raster) plus the download of that raster into
    page-locked host memory
  - k_detrend (float32 in, float32 out: 8 B per pixel) as the bandwidth yardstick of the run

    python profiles/bench_cells.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/cells_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0
CELLS = [(100, 100), (10, 10), (1000, 1000)]
SWEEP = [(16, 16), (20, 20), (32, 32), (50, 50), (70, 70), (300, 300)]  # where the two mappings cross


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cells_bench.json"))
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
    codes = torch.empty((n, n), dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    F32, F64, DEV = _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE
    ctx.invert_raw(n, n, F32, F32, DEV, p(inc), p(s_vv), None, None, p(anc), None, None, algo=_lib.ALGO_PRUNED, out_code_co=p(codes))
    del anc
    wind = torch.empty((n, n), dtype=torch.complex128, device=dev)
    ctx.expand_codes_raw(n * n, DEV, F64, p(codes), None, p(wind), None)
    ctx.synchronize()
    speed = wind.abs().float()
    keep = (inc < 40.0).to(torch.uint8).contiguous()
    detrended = torch.empty((n, n), dtype=torch.float32, device=dev)
    ratio = np.linspace(0.5, 2.0, n)
    pinned = torch.empty((n, n), dtype=torch.complex128, pin_memory=True)
    torch.cuda.synchronize()

    def outputs(cell):
        shape = (-(-n // cell[0]), -(-n // cell[1]))
        return [torch.empty(shape, dtype=dt, device=dev) for dt in (torch.int32, torch.complex128, torch.float64, torch.float64, torch.float64)]

    def cells_call(src, cell, mapping, with_keep=False):
        o = outputs(cell)
        k = keep if with_keep else None

        def run():
            os.environ["XSW_CELLS_MAPPING"] = mapping
            if src == "float32":
                ctx.raster_cells_raw(n, n, DEV, F32, p(speed), p(k), cell[0], cell[1], p(o[0]), p(o[2]), p(o[3]))
            else:
                kind, t = (_lib.CELLS_C128, wind) if src == "complex128" else (_lib.CELLS_CODES, codes)
                ctx.wind_cells_raw(n, n, DEV, kind, p(t), p(k), cell[0], cell[1], 0, 0, *[None] * 8, *(p(x) for x in o), None, None, None, None)
        return run, o

    per_px = {"complex128": 16, "codes": 4, "float32": 4}
    variants, nbytes, results = {}, {}, {}
    for src in per_px:
        for cell in CELLS + SWEEP:
            for mapping in ("wave", "workgroup"):
                name = f"{src} {cell[0]}x{cell[1]} {mapping}"
                variants[name], results[name] = cells_call(src, cell, mapping)
                nbytes[name] = per_px[src] * n * n
    for mapping in ("wave", "workgroup"):
        name = f"complex128+keep 100x100 {mapping}"
        variants[name], results[name] = cells_call("complex128", (100, 100), mapping, with_keep=True)
        nbytes[name] = 17 * n * n

    def expand_and_download():
        ctx.expand_codes_raw(n * n, DEV, F64, p(codes), None, p(wind), None)
        pinned.copy_(wind, non_blocking=True)
    variants["k_expand + pinned download"] = expand_and_download
    variants["k_expand"] = lambda: ctx.expand_codes_raw(n * n, DEV, F64, p(codes), None, p(wind), None)
    nbytes["k_expand"] = 20 * n * n
    variants["k_detrend"] = lambda: ctx.detrend_raw(n, n, F32, F32, DEV, p(s_vv), ratio, p(detrended))
    nbytes["k_detrend"] = 8 * n * n

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
    os.environ.pop("XSW_CELLS_MAPPING", None)
    med = {k: float(np.median(v)) for k, v in times.items()}

    # the two mappings and the two wind sources give the same bits
    same = {}
    for cell in CELLS:
        ref = results[f"complex128 {cell[0]}x{cell[1]} wave"]
        eq = lambda o: all(torch.equal(torch.nan_to_num(torch.view_as_real(x) if x.is_complex() else x.double()),
                                       torch.nan_to_num(torch.view_as_real(y) if y.is_complex() else y.double())) for x, y in zip(o, ref))
        same[f"{cell[0]}x{cell[1]}"] = bool(eq(results[f"complex128 {cell[0]}x{cell[1]} workgroup"]) and eq(results[f"codes {cell[0]}x{cell[1]} wave"])
                                            and eq(results[f"codes {cell[0]}x{cell[1]} workgroup"]))
    valid = float((results["complex128 100x100 wave"][0].double().sum() / (n * n)).item())

    frac = lambda name: round(nbytes[name] / (med[name] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
    res = {"workload": "cells", "raster": [n, n], "steps": a.steps, "warmup": a.warmup, "valid_pixels": round(valid, 4),
           "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "fraction_of_hbm_peak": {k: frac(k) for k in nbytes}, "bytes_read_per_pixel": {**per_px, "complex128+keep": 17},
           "mappings_and_sources_give_equal_bits": same, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
