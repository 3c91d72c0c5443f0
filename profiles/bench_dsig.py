"""Benchmark of dsig_cr from the unflattened noise on device rasters (20000 x 20000 float32 by default), per get_dsig rule:

  fused       windspeed.dsig_from_nesz: the flattening's fit, then k_dsig_flat (the flattened noise stays in a register)
  unfused     windspeed.nesz_flattening (fit + k_nesz_eval) followed by the device get_dsig (k_dsig)
  torch_ops   cmodms1ahw only: nesz_flattening followed by the reference's expression on torch's own operators, which is what
              get_dsig did with device tensors before k_dsig existed

HIP events, median of warm repetitions, the variants of one rule alternating inside one loop.  Every variant comes with the
bytes per pixel it has to move by its algorithm (the fit's two read passes, 8 + 4 B, are in all of them) and the rate achieved
against them.  Writes profiles/dsig_bench.json and prints the same JSON line.

    python profiles/bench_dsig.py [--size 20000] [--steps 7] [--warmup 2] [--out profiles/dsig_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "profiles"))

from bench_gradients_masked import HBM_PEAK_GBS, alternating  # noqa: E402

FIT_BYTES = 12  # k_nesz_colsum reads noise and inc (8 B), k_nesz_fit reads noise again (4 B); float32 rasters
RULES = {"gmf_s1_v2": 4, "gmf_rs2_v2": 0, "sarwing_lut_cmodms1ahw": 0}  # name -> incidence bytes the rule reads per pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dsig_bench.json"))
    a = ap.parse_args()

    import torch
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig, nesz_flattening

    n = a.size
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    inc = (20.0 + 25.0 * torch.arange(n, device=dev, dtype=torch.float32) / n).expand(n, n).contiguous()
    noise = 10.0 ** (-2.2 - 0.02 * (inc - 20.0)) * (0.9 + 0.2 * torch.rand((n, n), device=dev, generator=gen))
    sigma0 = noise * (0.05 + 20.0 * torch.rand((n, n), device=dev, generator=gen)) - 0.5 * noise  # a few per cent negative
    torch.cuda.synchronize()
    px = float(n) * n

    def entry(ms, raw, bytes_px):
        return {"ms": round(ms, 3), "bytes_per_pixel": bytes_px, "gb_per_s": round(bytes_px * px / ms / 1e6, 1),
                "fraction_of_hbm_peak": round(bytes_px * px / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4), "all_ms": raw}

    rules = {}
    for name, inc_b in RULES.items():
        fns = [lambda: dsig_from_nesz(name, inc, sigma0, noise), lambda: get_dsig(name, inc, sigma0, nesz_flattening(noise, inc))]
        labels = [("fused", FIT_BYTES + 4 + inc_b + 8), ("unfused", FIT_BYTES + 8 + 8 + 4 + inc_b + 8)]
        if name == "sarwing_lut_cmodms1ahw":
            fns.append(lambda: (1.25 / (sigma0 / nesz_flattening(noise, inc))) ** 4.0)
            labels.append(("torch_ops", FIT_BYTES + 8 + 8 + 4 + 8))  # the bytes of a single pass; the operators make three
        ms, raw = alternating(torch, fns, a.steps, a.warmup)
        rules[name] = {lab: entry(m, r, b) for (lab, b), m, r in zip(labels, ms, raw)}
        rules[name]["fused_over_unfused"] = round(ms[0] / ms[1], 4)
    (flat_ms,), raw = alternating(torch, [lambda: nesz_flattening(noise, inc)], a.steps, a.warmup)
    res = {"workload": "dsig_from_nesz", "raster": [n, n], "dtype": "float32", "out_dtype": "float64", "steps": a.steps, "warmup": a.warmup,
           "rules": rules, "nesz_flattening_alone": entry(flat_ms, raw[0], FIT_BYTES + 8), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
