#!/usr/bin/env python3
"""Detours of k_invert_band's waves on the headline scene (CMOD5.N mono, 20000 x 20000 float32), counted by a counter build of
the library (-DXSW_BAND_DETOUR_STATS, xsw_band.hpp / xsw_device.hpp) on the production chain (xsw_stats_enable(ctx, 2)):

    XSW_LIB=$PWD/build/libxsw_detours.so XSW_EXTRA_FLAGS=-DXSW_BAND_DETOUR_STATS python -m xsarsea_amd._build
    XSW_LIB=$PWD/build/libxsw_detours.so python profiles/band_detours.py out.json

Per wave of k_invert_band: the library-log10 detour (some lane's sigma0 is NaN, 0, inf or negative after the dB offset: what
to_db(float) took through ocml's log10 while that sat behind a branch), store_pixel's near-tie path (two emulated divisions, two
float64 atan2), the tail-cut branch of stage 1, and the trips of the first ray's loop.  In a library built without the flag the
same slots hold the chain's usual counters and the figures mean nothing: the script refuses to report them."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from xsarsea_amd import _lib  # noqa: E402

lines = samples = int(os.environ.get("XSW_TRAFFIC_N", "20000"))
dev = torch.device("cuda", 0)
lut, co = bench.build_product_lut()
ctx = _lib.Context(0)
ctx.upload_luts(co=co)
inc, s_vv, anc = bench.make_scene(lines, samples, lines, 0, 20260322, dev)
out = torch.empty((lines, samples), dtype=torch.complex64, device=dev)
torch.cuda.synchronize()
ctx.stats_enable(2)
ctx.invert_raw(lines, samples, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE, inc.data_ptr(), s_vv.data_ptr(), None, None,
               anc.data_ptr(), out.data_ptr(), None, algo=_lib.ALGO_PRUNED)
st, ch = ctx.stats(), ctx.stats_chain()
ctx.stats_enable(False)
all_waves = lines * ((samples + 63) // 64)
waves = st["pixels_co"]
if not 0 < waves <= all_waves:
    sys.exit("not a -DXSW_BAND_DETOUR_STATS build: slot 0 holds %d, the raster has %d waves" % (waves, all_waves))
res = {
    "what": "k_invert_band detour counters (-DXSW_BAND_DETOUR_STATS, production chain, headline scene %d^2 CMOD5.N mono float32); per wave" % lines,
    "waves": all_waves,
    "waves_with_co_search": waves,
    "nan_sigma0_share": float(torch.isnan(s_vv).float().mean()),
    "log10_detour_waves": st["cand_co"], "log10_detour_share": st["cand_co"] / all_waves,
    "store_near_tie_waves": st["pixels_exact"], "store_near_tie_share": st["pixels_exact"] / all_waves,
    "tail_cut_branch_waves": st["pixels_cr"], "tail_cut_branch_share": st["pixels_cr"] / all_waves,
    "first_ray_trips": ch["cand_band2"], "first_ray_trips_per_wave": ch["cand_band2"] / waves,
}
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
