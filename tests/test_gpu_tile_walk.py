"""The tile walk (csrc/xsw_tilewalk.hpp) at its six sites, on rasters whose strips leave 0, 1 or 2 tile columns over and whose
line groups are 1, 2, 8, 9 and 17, ragged last strips and last groups included.

Every route that restates the walk inverts the same friendly scene (NaN holes as in the other route tests) into buffers
pre-filled with a sentinel bit pattern:
  * the production chain (k_invert_band and its followers);
  * the chain with the statistics instantiation of k_invert_band;
  * the forced one-kernel pruned route (k_invert, XSW_NO_BAND=1);
  * algo="exhaustive" (k_invert_exhaustive32);
  * the two overflow walks of k_invert_list (XSW_LIST_CAP_TEST, with and without the strip masks), at 64 * 9 + 1 samples x 33 lines.
No sentinel may be left (a tile nobody took), the output must equal algo="exact" on the same raster bit for bit, and with the
statistics on pixels_co must equal the number of searchable pixels (a tile taken twice counts twice).

The routing switches are read once per process, so the routes behind a switch run in one child process each, over all shapes;
the scenes and the exact answers are made once, here, and handed over in one .npz."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from util import lut_dicts

pytestmark = pytest.mark.gpu

SAMPLES = (40, 64 * 7 + 3, 64 * 8, 64 * 9 + 1, 64 * 15 + 63, 64 * 17)  # strips 1, 8, 8, 10, 16, 17
LINES = (1, 5, 29, 33, 67)                                            # line groups 1, 2, 8, 9, 17
SHAPES = [(s, l) for s in SAMPLES for l in LINES]
OVERFLOW_SHAPE = (64 * 9 + 1, 33)
OVERFLOW_CAP = 16  # the smallest the switch takes
SENTINEL = 0x5EA15EA1  # as float32 about 5.8e18: no wind component, and not the NaN the kernels store
CHILD_ROUTES = {
    "one-kernel": ({"XSW_NO_BAND": "1"}, SHAPES),
    "overflow-masks": ({"XSW_LIST_CAP_TEST": str(OVERFLOW_CAP)}, [OVERFLOW_SHAPE]),
    "overflow-nomask": ({"XSW_LIST_CAP_TEST": str(OVERFLOW_CAP), "XSW_NO_STRIP_MASKS": "1"}, [OVERFLOW_SHAPE]),
}


def scene(samples, lines):
    from test_gpu_kernel import synthetic_scene
    inc, s_vv, _, _, anc = synthetic_scene(lines, samples, np.float32, 1000 + samples + lines)
    # infinite sigma0 here and there: searchable pixels with a non-finite co-pol problem, which are list G's whatever the route
    # (as in tests/route_geometry.py; some 95 on the overflow shape, against the 16 entries the list has there)
    s_vv[np.random.default_rng(samples * 100 + lines).random(s_vv.shape) < 0.005] = np.inf
    return inc, s_vv, anc


def searchable(inc, s_vv, anc):
    """Pixels with a co-pol search: incidence and sigma0 not NaN (inf counts), |a-priori wind| not NaN."""
    with np.errstate(all="ignore"):
        return int(np.sum(~np.isnan(inc) & ~np.isnan(s_vv) & ~np.isnan(np.abs(anc))))


def invert(ctx, inc, s_vv, anc, algo, stats=False):
    """One mono float32 -> complex64 inversion on device rasters into a sentinel-filled buffer: (output bits as int32
    [lines, samples, 2], timing(), stats() or None)."""
    import torch
    from xsarsea_amd import _lib
    dev = torch.device("cuda", 0)
    lines, samples = inc.shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (inc, s_vv, anc)]
    out = torch.full((lines, samples, 2), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.timing_enable(True)
    if stats:
        ctx.stats_enable(True)
    try:
        ctx.invert_raw(lines, samples, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE, t[0].data_ptr(), t[1].data_ptr(), None, None,
                       t[2].data_ptr(), out.data_ptr(), None, algo=_lib.ALGOS[algo])
        ctx.synchronize()
        tm, st = ctx.timing(), (ctx.stats() if stats else None)
    finally:
        ctx.timing_enable(False)
        if stats:
            ctx.stats_enable(False)
    return out.cpu().numpy(), tm, st


def verdict(got, want, tm, st, inc, s_vv, anc):
    return dict(sentinel_left=int(np.sum(got == SENTINEL)), differ=int(np.sum(got != want)), launches=int(tm["launches"]),
                list_px=int(tm["last_list_pixels"]), pixels_co=None if st is None else int(st["pixels_co"]), searchable=searchable(inc, s_vv, anc))


def check(v, chain):
    assert v["sentinel_left"] == 0, f"{v['sentinel_left']} output words still hold the sentinel: a tile nobody took"
    assert v["differ"] == 0, f"{v['differ']} output words differ from algo=exact"
    assert v["launches"] == (1 if chain else 0), ("the route that ran is not the one asked for", v)
    if v["pixels_co"] is not None:
        assert v["pixels_co"] == v["searchable"], ("searched pixels against searchable pixels: a tile taken twice, or not at all", v)


@pytest.fixture(scope="module")
def ctx(gpu_ctx, default_luts):
    co, _ = lut_dicts(default_luts[0], None)
    gpu_ctx.upload_luts(co=co)
    return gpu_ctx


@pytest.fixture(scope="module")
def exact(ctx):
    """{(samples, lines): (inc, s_vv, anc, output bits of algo="exact")}, made once."""
    out = {}
    for s, l in SHAPES:
        inc, s_vv, anc = scene(s, l)
        want, _, _ = invert(ctx, inc, s_vv, anc, "exact")
        assert not np.any(want == SENTINEL)
        assert 0 < searchable(inc, s_vv, anc) < inc.size  # pixels with an answer, and pixels without
        out[(s, l)] = (inc, s_vv, anc, want)
    return out


@pytest.fixture(scope="module")
def problem_npz(exact, tmp_path_factory):
    path = tmp_path_factory.mktemp("tile_walk") / "problem.npz"
    d = {}
    for (s, l), (inc, s_vv, anc, want) in exact.items():
        d.update({f"{s}x{l}/inc": inc, f"{s}x{l}/sco": s_vv, f"{s}x{l}/anc": anc, f"{s}x{l}/want": want})
    np.savez(path, **d)
    return str(path)


@pytest.mark.parametrize("samples,lines", SHAPES)
@pytest.mark.parametrize("route", ["chain", "chain-stats", "exhaustive"])
def test_route_takes_every_tile_once(ctx, exact, route, samples, lines):
    inc, s_vv, anc, want = exact[(samples, lines)]
    got, tm, st = invert(ctx, inc, s_vv, anc, "exhaustive" if route == "exhaustive" else "pruned", stats=route == "chain-stats")
    check(verdict(got, want, tm, st, inc, s_vv, anc), chain=route != "exhaustive")


def child_main(npz, shapes):
    """In a child process, under the parent's routing switches: algo="pruned" with the statistics on, every shape asked for."""
    from oracle import lut as olut
    from xsarsea_amd import _lib
    d = np.load(npz)
    c = _lib.Context(0)
    co, _ = lut_dicts(olut.to_lut("gmf_cmod5n"), None)
    c.upload_luts(co=co)
    res = {}
    for key in shapes:
        inc, s_vv, anc, want = (d[f"{key}/{k}"] for k in ("inc", "sco", "anc", "want"))
        got, tm, st = invert(c, inc, s_vv, anc, "pruned", stats=os.environ.get("XSW_NO_BAND") == "1")
        res[key] = verdict(got, want, tm, st, inc, s_vv, anc)
    c.close()
    print("RESULTS " + json.dumps(res))


_children = {}


def child_results(route, npz):
    """One child process per route and pytest session; a route whose process failed is not started again."""
    if route not in _children:
        env_add, shapes = CHILD_ROUTES[route]
        env = {k: v for k, v in os.environ.items() if not k.startswith("XSW_") or k == "XSW_LIB"}
        env.update(env_add)
        code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_tile_walk as t; t.child_main(sys.argv[1], sys.argv[2:])"
                % (REPO, os.path.join(REPO, "tests")))
        try:
            r = subprocess.run([sys.executable, "-c", code, npz] + [f"{s}x{l}" for s, l in shapes], env=env, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            _children[route] = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULTS "))[8:])
        except BaseException as e:
            _children[route] = e
    if isinstance(_children[route], BaseException):
        raise _children[route]
    return _children[route]


@pytest.mark.parametrize("samples,lines", SHAPES)
def test_one_kernel_route_takes_every_tile_once(problem_npz, samples, lines):
    v = child_results("one-kernel", problem_npz)[f"{samples}x{lines}"]
    assert v["pixels_co"] is not None
    check(v, chain=False)


@pytest.mark.parametrize("route", ["overflow-masks", "overflow-nomask"])
def test_overflow_walks_take_every_tile_once(problem_npz, route):
    """List G holds 16 pixels: k_invert_list walks the marked strips (strip masks) or every tile (no masks) of the raster."""
    v = child_results(route, problem_npz)["%dx%d" % OVERFLOW_SHAPE]
    assert v["list_px"] > OVERFLOW_CAP, ("list G did not overflow: the walk did not run", v)
    check(v, chain=True)
