"""k_invert_band with the window-class queues of a workgroup's four waves pooled (XSW_BAND_POOL, xsw_band.hpp: band_wave):
every pixel is still settled by one segment with the same arithmetic, only the wave that runs the pass changes, so the fast
path must equal the exhaustive sweep bit for bit -- also where a workgroup has fewer than four live waves, where whole waves
hold no eligible pixel, and where its waves hold different window classes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from test_gpu_kernel import synthetic_scene
from util import bits_equal, lut_dicts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx_default(gpu_ctx, default_luts):
    lco, lcr = default_luts
    co, cr = lut_dicts(lco, lcr)
    gpu_ctx.upload_luts(co=co, cr=cr)
    return gpu_ctx


def _mono_equal(ctx, inc, s_vv, anc, what):
    got = ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
    ex = ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    assert bits_equal(got[0], ex[0]), what
    assert np.array_equal(got[2], ex[2]), what


def _classes_scene(lines, samples, seed):
    """A scene whose lines (= the waves of a workgroup) differ in how far the a-priori wind is from the truth: line % 4 == 0
    close (narrow windows), 1 and 2 further off, 3 far off (wide windows) -- a workgroup's waves then hold different classes."""
    inc, s_vv, _, _, anc = synthetic_scene(lines, samples, np.float64, seed)
    rng = np.random.default_rng(seed)
    scale = np.array([1.0, 1.3, 0.7, 0.35])[np.arange(lines) % 4][:, None]
    noise = np.array([0.2, 1.0, 2.0, 6.0])[np.arange(lines) % 4][:, None]
    anc = anc * scale + noise * (rng.standard_normal(anc.shape) + 1j * rng.standard_normal(anc.shape))
    return inc, s_vv, anc


@pytest.mark.parametrize("lines", [1, 2, 3, 5, 6, 7, 39])
@pytest.mark.parametrize("samples", [64, 200, 333])
def test_partial_workgroups(ctx_default, lines, samples):
    """Raster heights that leave the last workgroup 1-3 live waves (the others run through without pixels), widths that are
    and are not a multiple of 64."""
    inc, s_vv, anc = _classes_scene(lines, samples, 100 + lines)
    _mono_equal(ctx_default, inc, s_vv, anc, (lines, samples))


def test_whole_waves_without_eligible_pixels(ctx_default):
    """Lines with no pixel for the band rule: sigma0 NaN, incidence NaN, ancillary NaN, sigma0 infinite -- next to ordinary lines
    in the same workgroups (every pattern of dead waves 0..3 out of 4)."""
    lines, samples = 64, 250
    inc, s_vv, anc = _classes_scene(lines, samples, 7)
    for ln in range(lines):
        g, w = divmod(ln, 4)
        if (g >> w) & 1 == 0:
            continue
        kind = (g + w) % 4
        if kind == 0:
            s_vv[ln] = np.nan
        elif kind == 1:
            inc[ln] = np.nan
        elif kind == 2:
            anc[ln] = np.nan
        else:
            s_vv[ln] = np.inf
    _mono_equal(ctx_default, inc, s_vv, anc, "dead waves")


def test_disjoint_classes_per_wave(ctx_default):
    """The four lines of every workgroup far apart in window width (narrow, wider, wider, wide): the pooled queues of the workgroup
    take each class from mostly one wave, and passes run in waves that own none of their pixels."""
    lines, samples = 48, 640
    inc, s_vv, anc = _classes_scene(lines, samples, 11)
    _mono_equal(ctx_default, inc, s_vv, anc, "classes per wave")


def test_dual_pol_instantiation(ctx_default):
    """The dual-pol instantiation of k_invert_band pools as well: co-pol and cross-pol equal the general kernel's full search
    (the exhaustive sweep is mono co-pol only)."""
    lines, samples = 23, 333
    inc, s_vv, s_vh, dsig, anc = synthetic_scene(lines, samples, np.float64, 21)
    got = ctx_default.invert_host(inc, sigma0_co=s_vv, sigma0_cr=s_vh, dsig_cr=dsig, anc=anc, algo="pruned", want_idx=True)
    ex = ctx_default.invert_host(inc, sigma0_co=s_vv, sigma0_cr=s_vh, dsig_cr=dsig, anc=anc, algo="exact", want_idx=True)
    assert bits_equal(got[0], ex[0]) and bits_equal(got[1], ex[1])
    assert np.array_equal(got[2], ex[2])


def test_statistics_instantiation_counts_per_pixel(ctx_default):
    """The statistics instantiation counts candidates per pixel: a raster's count is the sum of its lines' counts inverted one
    line at a time (one live wave per workgroup: nothing to pool)."""
    lines, samples = 7, 333
    inc, s_vv, anc = _classes_scene(lines, samples, 5)
    ctx_default.stats_enable(True)
    try:
        ctx_default.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned")
        whole = ctx_default.stats()
        per_line = {}
        for ln in range(lines):
            ctx_default.invert_host(inc[ln:ln + 1], sigma0_co=s_vv[ln:ln + 1], anc=anc[ln:ln + 1], algo="pruned")
            for k, v in ctx_default.stats().items():
                per_line[k] = per_line.get(k, 0) + v
    finally:
        ctx_default.stats_enable(False)
    assert whole["cand_co"] > 0
    assert whole == per_line


_ROUTE_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
if {device!r}:
    import torch  # (before libxsw.so is loaded: seconds faster than after it)
from oracle import lut as olut
from util import lut_dicts, bits_equal
from test_gpu_band_pool import _classes_scene
from xsarsea_amd import _lib
co, _ = lut_dicts(olut.to_lut("gmf_cmod5n"), None)
ctx = _lib.Context(0)
ctx.upload_luts(co=co)
# (the overflow routes: rasters of some 40 000 pixels -- a tenth of such a scene is k_invert_band2's, and list B holds 1200)
for lines, samples, seed in (((119, 333, 3), (14, 2500, 4)) if {device!r} else ((39, 333, 3), (6, 900, 4))):
    inc, s_vv, anc = _classes_scene(lines, samples, seed)
    if {device!r}:  # device rasters: the context's own work lists, the only ones XSW_LIST_CAP_TEST shrinks (host rasters go through the workers' lists)
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(a).to(dev) for a in (inc, s_vv, anc)]
        out = torch.empty(inc.shape, dtype=torch.complex128, device=dev)
        idx = torch.empty(inc.shape + (3,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.timing_enable(True)
        ctx.invert_raw(lines, samples, _lib.XSW_F64, _lib.XSW_F64, _lib.MEM_DEVICE, t[0].data_ptr(), t[1].data_ptr(), None, None, t[2].data_ptr(),
                       out.data_ptr(), None, out_idx=idx.data_ptr(), algo=_lib.ALGO_PRUNED)
        tm = ctx.timing()
        ctx.timing_enable(False)
        got = (out.cpu().numpy(), None, idx.cpu().numpy())
        handed = (tm["last_list_pixels"], tm["last_band2_pixels"], tm["last_blocks_pixels"])
    else:
        got = ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
        handed = (-1, -1, -1)
    ex = ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    print("RESULT", lines, samples, int(bits_equal(got[0], ex[0]) and np.array_equal(got[2], ex[2])), *handed)
"""


@pytest.mark.parametrize("route", ["long-run-1", "long-run-0", "list-300", "arc-always", "arc-never", "no-records", "no-masks-300"])
def test_hand_over_routes(route):
    """The hand-over routes of k_invert_band forced, in a fresh process (the switches are read once): every eligible pixel to
    k_invert_band2 / none, overflowing lists (strip masks, and without them), the stage-1 live arc always / never, list B as
    indices -- on heights that leave partial workgroups.  The two overflow routes invert device rasters (the context's lists are
    the ones XSW_LIST_CAP_TEST shrinks to 300 entries for list G and 4 x 300 each for lists B and C; on host rasters the workers'
    lists of 16384 entries or more never overflowed, whatever the variable said) and show from the lists' counters that list B
    overflowed.  With 300 entries the 39 x 333 scene of the other routes hands 1007 pixels to k_invert_band2, 100 to k_invert_blocks
    and none to k_invert_list: nothing overflows there either, hence the larger rasters (heights 119 and 14: partial workgroups
    all the same).  An overflowing list G: tests/test_gpu_route_geometry.py, cap64."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("XSW_")}
    env.update({"long-run-1": {"XSW_LONG_RUN": "1"}, "long-run-0": {"XSW_LONG_RUN": "0"}, "list-300": {"XSW_LIST_CAP_TEST": "300"},
                "arc-always": {"XSW_ARC_MIN": "8", "XSW_ARC_CROWD": "1"}, "arc-never": {"XSW_ARC_MIN": "0"},
                "no-records": {"XSW_NO_RECORDS": "1"},
                "no-masks-300": {"XSW_LIST_CAP_TEST": "300", "XSW_NO_STRIP_MASKS": "1"}}[route])
    if "XSW_LIB" in os.environ:
        env["XSW_LIB"] = os.environ["XSW_LIB"]
    overflow = route in ("list-300", "no-masks-300")
    r = subprocess.run([sys.executable, "-c", _ROUTE_SCRIPT.format(repo=REPO, device=overflow)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert len(rows) == 2
    for _, lines, samples, ok, n_g, n_b, n_c in rows:
        assert ok == "1", (route, lines, samples)
        print(route, lines, samples, "handed to k_invert_list / k_invert_band2 / k_invert_blocks:", n_g, n_b, n_c)
        if overflow:
            assert int(n_b) > 4 * 300, (route, lines, samples, "list B did not overflow", n_g, n_b, n_c)
