"""Every forced route of the inversion chain on LUT shapes other than the default one, against the CPU oracle.

The routing switches (RouteKnobs, csrc/xsw_plan.hpp) are read once per process, so each route is one child process.  The
child installs the seven tables of tests/route_geometry.py one after the other on one context and inverts each table's scene
(13 x 333 pixels, float32 and float64, mono and dual-pol) twice: through invert_host (the workers' lists) and on device rasters
through invert_raw (the context's lists: the only ones XSW_LIST_CAP_TEST shrinks).  The parent process builds tables, scenes
and the oracle's answer once, without a GPU, and hands them over in one .npz.  A child process takes 3.1 .. 3.8 s on an MI355X (LABBOOK section 20 has the counters seen).

Reference: oracle.cport / oracle.invert (the numpy restatement of the reference), never another GPU kernel.  Grid indices must
equal the oracle's on every pixel; the winds go through assert_complex_close with test_random_configurations's tolerances (1e-12
co-pol, 1e-9 cross-pol).  algo="exhaustive_f64" must give the oracle's co-pol indices on every table as well, so that a failure
of a route can be told from a failure of a table.

That a forced route really ran is read from timing() (the counters of the context's lists: device-raster calls only) and
stats_chain() (what each kernel of the production chain scored), per geometry (the second half of the test).  What no counter shows:
  * the stage-1 live arc of k_invert_band (window_arc) has no counter, and the kernel sits on a register-allocation edge that a
    counter would move.  That it runs under `arc-always` rests on the thresholds in KArgs: XSW_ARC_MIN=8 directions and
    XSW_ARC_CROWD=1 pixel per wave, against scenes whose waves hold 48 or more windows of 8 directions or more in three lines
    of four (one line of four on the two coarse tables): tests/test_route_geometry_cpu.py checks exactly that.
  * the tail sweep of k_invert_band2 has no counter of its own either.  It is seen by what it takes off the general kernels: on
    `tail`, k_invert_list and k_invert_blocks are left fewer pixels with it (`default`) than without (`tail-sweep-0`).
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import route_geometry as rg
from conftest import REPO

pytestmark = pytest.mark.gpu

DTYPES = {"f64": np.float64, "f32": np.float32}
SCENE_KEYS = ("inc", "sco", "scr", "dsig", "anc")
BLOCKS_OFF = ("narrow", "coarse_full")  # blk_span_ok == 0 (tests/test_host_lutplan.py pins it): no k_invert_blocks on these tables
LIST_CAP = 64

ROUTES = {
    "default": {},
    "long-run-1": {"XSW_LONG_RUN": "1"},
    "long-run-0": {"XSW_LONG_RUN": "0"},
    "arc-always": {"XSW_ARC_MIN": "8", "XSW_ARC_CROWD": "1"},
    "arc-never": {"XSW_ARC_MIN": "0"},
    "refine-always": {"XSW_B2_REFINE_MIN": "0"},
    "refine-never": {"XSW_B2_REFINE_MIN": "65", "XSW_B2_CROWD": "65"},
    "rows8-refine-always": {"XSW_B2_ROWS_MAX": "8", "XSW_B2_REFINE_MIN": "0"},
    "wide16": {"XSW_B2_WIDE": "16"},
    "crowd1": {"XSW_B2_CROWD": "1"},
    "no-records": {"XSW_NO_RECORDS": "1"},
    "cap64": {"XSW_LIST_CAP_TEST": str(LIST_CAP)},
    "cap64-nomask": {"XSW_LIST_CAP_TEST": str(LIST_CAP), "XSW_NO_STRIP_MASKS": "1"},
    "cap64-norecords": {"XSW_LIST_CAP_TEST": str(LIST_CAP), "XSW_NO_RECORDS": "1"},
    "all-blocks": {"XSW_BLOCK_MIN": "0"},
    "no-blk4": {"XSW_NO_BLK4": "1"},
    "no-blocks-kernel": {"XSW_NO_BLOCKS_KERNEL": "1"},
    "no-band": {"XSW_NO_BAND": "1"},
    "tail-sweep-0": {"XSW_TAIL_SWEEP": "0"},
    "no-tail-cut": {"XSW_TAIL_SWEEP": "0", "XSW_NO_TAIL_CUT": "1"},  # (as test_tail_cut_keeps_saturating_windows_in_the_band_kernels: neither)
}


@pytest.fixture(scope="module")
def problem(tmp_path_factory):
    """Tables, scenes and the oracle's answers of every geometry in one .npz (no GPU in here)."""
    d = {}
    for g in rg.GEOMETRIES:
        lco, lcr = rg.build_luts(g)
        d.update({f"{g}/co": lco.values, f"{g}/inc_ax": lco.incidence, f"{g}/w_ax": lco.wspd, f"{g}/phi_ax": lco.phi,
                  f"{g}/cr": lcr.values, f"{g}/wcr_ax": lcr.wspd})
        for tag, dt in DTYPES.items():
            sc = rg.build_scene(g, dt)
            o_co, o_cr, o_idx = rg.oracle_answer(lco, lcr, sc)
            # the scene must hold what the comparison is about: pixels with an answer, and pixels without
            assert (o_idx[..., 0] >= 0).sum() > 0.85 * o_idx[..., 0].size and (o_idx[..., 0] < 0).any() and (o_idx[..., 2] >= 0).any()
            d.update({f"{g}/{tag}/{k}": sc[k] for k in SCENE_KEYS})
            d.update({f"{g}/{tag}/o_co": o_co, f"{g}/{tag}/o_cr": o_cr, f"{g}/{tag}/o_idx": o_idx.astype(np.int32)})
    path = tmp_path_factory.mktemp("route_geometry") / "problem.npz"
    np.savez(path, **d)
    return str(path)


_CHILD = r"""
import sys, time
t0 = time.perf_counter()
import numpy as np
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
import torch
from oracle import lut as olut
from util import lut_dicts, assert_complex_close
import route_geometry as rg
from xsarsea_amd import _lib
d = np.load({npz!r})
ctx = _lib.Context(0)
dev = torch.device("cuda", 0)

def close(got, ref, rtol):
    try:
        assert_complex_close(got, ref, rtol=rtol)
        return "ok"
    except AssertionError as e:
        return "FAIL:" + str(e).replace(" ", "_")

for g in rg.GEOMETRIES:
    lco = olut.Lut(d[g + "/co"], d[g + "/inc_ax"], d[g + "/w_ax"], d[g + "/phi_ax"], "dB", "x", "co", "VV")
    lcr = olut.Lut(d[g + "/cr"], d[g + "/inc_ax"], d[g + "/wcr_ax"], None, "dB", "x", "cr", "VH")
    co, cr = lut_dicts(lco, lcr)
    ctx.upload_luts(co=co, cr=cr)
    for tag in ("f64", "f32"):
        inc, sco, scr, dsig, anc = (d[g + "/" + tag + "/" + k] for k in ("inc", "sco", "scr", "dsig", "anc"))
        o_co, o_cr, o_idx = (d[g + "/" + tag + "/" + k] for k in ("o_co", "o_cr", "o_idx"))
        ex = ctx.invert_host(inc, sigma0_co=sco, anc=anc, dsig_co=rg.DSIG_CO, sigma0_is_db=True, algo="exhaustive_f64", want_idx=True)
        print("EXHAUSTIVE", g, tag, int(np.sum(np.any(ex[2][..., :2] != o_idx[..., :2], axis=-1))))
        t_in = [torch.from_numpy(a).to(dev) for a in (inc, sco, scr, dsig, anc)]
        xdt = _lib.XSW_F32 if tag == "f32" else _lib.XSW_F64
        for mode in ("mono", "dual"):
            dual = mode == "dual"
            want_idx = o_idx.copy()
            if not dual:
                want_idx[..., 2] = -1  # (the mono call runs no cross-pol search)
            for path in ("host", "device"):
                ctx.timing_enable(True)
                ctx.stats_enable(2)
                if path == "host":
                    got_co, got_cr, idx = ctx.invert_host(inc, sigma0_co=sco, sigma0_cr=scr if dual else None, dsig_cr=dsig if dual else None, anc=anc,
                                                          dsig_co=rg.DSIG_CO, sigma0_is_db=True, algo="pruned", want_idx=True)
                    tm = dict(last_band2_pixels=-1, last_list_pixels=-1, last_blocks_pixels=-1)
                else:
                    out_co = torch.full(inc.shape, float("nan"), dtype=torch.complex128, device=dev)
                    out_cr = torch.full(inc.shape, float("nan"), dtype=torch.complex128, device=dev) if dual else None
                    t_idx = torch.full(inc.shape + (3,), -7, dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()
                    ctx.invert_raw(inc.shape[0], inc.shape[1], xdt, _lib.XSW_F64, _lib.MEM_DEVICE, t_in[0].data_ptr(), t_in[1].data_ptr(),
                                   t_in[2].data_ptr() if dual else None, t_in[3].data_ptr() if dual else None, t_in[4].data_ptr(), out_co.data_ptr(),
                                   out_cr.data_ptr() if dual else None, out_idx=t_idx.data_ptr(), dsig_co=rg.DSIG_CO, sigma0_is_db=True,
                                   algo=_lib.ALGO_PRUNED)
                    tm = ctx.timing()
                    got_co, got_cr, idx = out_co.cpu().numpy(), (out_cr.cpu().numpy() if dual else None), t_idx.cpu().numpy()
                ch = ctx.stats_chain()
                ctx.stats_enable(False)
                ctx.timing_enable(False)
                print("RESULT", g, tag, mode, path, int(np.sum(np.any(idx != want_idx, axis=-1))), close(got_co, o_co, 1e-12),
                      close(got_cr, o_cr, 1e-9) if dual else "ok", tm["last_band2_pixels"], tm["last_list_pixels"], tm["last_blocks_pixels"],
                      ch["cand_band2"], ch["cand_blocks"], ch["cand_list"], ch["pixels_refined"])
ctx.close()
print("SECONDS %.2f" % (time.perf_counter() - t0))
"""

FIELDS = ("idx_mismatch", "co", "cr", "band2_px", "list_px", "blocks_px", "cand_band2", "cand_blocks", "cand_list", "refined")
_runs = {}


def run_route(route, npz):
    """One child process per route and pytest session: {(geometry, dtype, mode, path): dict of FIELDS}, {(geometry, dtype):
    mismatches of the exhaustive sweep}."""
    if route in _runs:
        if isinstance(_runs[route], BaseException):  # (a route that failed is not started again for another route's comparison)
            raise _runs[route]
        return _runs[route]
    try:
        _runs[route] = _start_route(route, npz)
    except BaseException as e:
        _runs[route] = e
        raise
    return _runs[route]


def _start_route(route, npz):
    env = {k: v for k, v in os.environ.items() if not k.startswith("XSW_") or k == "XSW_LIB"}
    env.update(ROUTES[route])
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, npz=npz)], env=env, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    rows, exh = {}, {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[:1] == ["RESULT"]:
            rows[tuple(t[1:5])] = {k: (v if k in ("co", "cr") else int(v)) for k, v in zip(FIELDS, t[5:])}
        elif t[:1] == ["EXHAUSTIVE"]:
            exh[tuple(t[1:3])] = int(t[3])
    print(f"route {route}: process {wall:.1f} s" + "".join("\n  " + ln for ln in r.stdout.splitlines() if not ln.startswith("EXHAUSTIVE")))
    assert len(rows) == len(rg.GEOMETRIES) * 8 and len(exh) == len(rg.GEOMETRIES) * 2, r.stdout[-2000:]
    return rows, exh


def device_rows(rows, g):
    return [(k, v) for k, v in rows.items() if k[0] == g and k[3] == "device"]


def left_to_general_kernels(rows, g):
    """Pixels of geometry g's device-raster calls that k_invert_band and k_invert_band2 left to k_invert_blocks and k_invert_list."""
    return sum(v["list_px"] + v["blocks_px"] for _, v in device_rows(rows, g))


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_on_every_geometry(route, problem):
    rows, exh = run_route(route, problem)
    for key, n in exh.items():
        assert n == 0, f"{key}: {n} pixels of the exhaustive float64 sweep differ from the oracle: the table, not the route"
    for key, v in rows.items():
        assert v["idx_mismatch"] == 0, f"{route} {key}: grid indices differ from the oracle on {v['idx_mismatch']} pixels"
        assert v["co"] == "ok", f"{route} {key}: co-pol wind {v['co']}"
        assert v["cr"] == "ok", f"{route} {key}: cross-pol wind {v['cr']}"
    # ---- the forced route was reached, geometry by geometry
    for g in rg.GEOMETRIES:
        dev = device_rows(rows, g)
        every = [(k, v) for k, v in rows.items() if k[0] == g]
        assert len(dev) == 4 and len(every) == 8
        for k, v in every:
            if g in BLOCKS_OFF or route in ("no-blocks-kernel", "no-band"):
                assert v["cand_blocks"] == 0, (route, k, "k_invert_blocks scored candidates")
        if route == "no-band":  # the one-kernel path: no list is written
            assert all(v["cand_band2"] == 0 for _, v in every), (route, g)
            continue
        for k, v in dev:
            if route == "long-run-0":
                assert v["band2_px"] == 0, (route, k, v)
            else:
                assert v["band2_px"] > 0, (route, k, "no pixel was handed to k_invert_band2", v)
            if route.startswith("cap64"):
                # list G overflowed: the pixels with a non-finite co-pol problem alone (some 85 per raster: route_geometry.build_scene) are
                # more than its 64 entries, on every table and in both modes
                assert v["list_px"] > LIST_CAP, (route, k, "list G did not overflow", v)
        for k, v in every:
            if route == "long-run-0":
                assert v["cand_band2"] == 0 and v["refined"] == 0, (route, k, v)
            elif route == "rows8-refine-always":
                # a live arc of more than 8 rows is passed on: k_invert_band2 itself may score nothing, the general kernels take its pixels
                assert (v["cand_list"] if g in BLOCKS_OFF else v["cand_blocks"]) > 0, (route, k, v)
            else:
                assert v["cand_band2"] > 0, (route, k, "k_invert_band2 scored nothing", v)
            if route in ("refine-always", "crowd1"):
                assert v["refined"] > 0, (route, k, "no record went through the refinement", v)
            if route == "refine-never":
                assert v["refined"] == 0, (route, k, v)
            if route == "all-blocks":
                if g in BLOCKS_OFF:
                    assert v["cand_list"] > 0, (route, k, "list C's pixels did not reach k_invert_list", v)
                else:
                    assert v["cand_blocks"] > 0, (route, k, "k_invert_blocks scored nothing", v)
    if route in ("default", "tail-sweep-0", "no-tail-cut"):
        with_sweep = left_to_general_kernels(run_route("default", problem)[0], "tail")
        without = left_to_general_kernels(run_route("tail-sweep-0", problem)[0], "tail")
        assert with_sweep < without, ("tail sweep", with_sweep, without)
        if route == "no-tail-cut":
            assert without <= left_to_general_kernels(rows, "tail"), ("tail cut", without, left_to_general_kernels(rows, "tail"))
