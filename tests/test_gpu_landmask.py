"""xsarsea_amd.landmask on the MI355X against its CPU restatement (tests/landmask_ref.py): every case of tests/landmask_cases.py,
through numpy arrays and through device tensors, on the banded kernel (at its own band count and at forced ones) and on the
direct kernel, byte for byte.  The statement has no division and no library call, and the kernels and the restatement round the
same operations in the same order."""
import numpy as np
import pytest

import landmask_cases as lc
import landmask_ref as lref
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from util import bits_equal
from xsarsea_amd import TiePoints, _lib, land_mask, landmask, wind_cells, wind_grid

pytestmark = pytest.mark.gpu

# (XSW_LAND_PATH, XSW_LAND_BANDS): both kernels at the plan's own band count, the banded one at three forced counts
CONFIGS = [("bands", None), ("direct", None), ("bands", "1"), ("bands", "7"), ("bands", "1000")]


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def set_knobs(monkeypatch, path, bands):
    monkeypatch.setenv("XSW_LAND_PATH", path)
    if bands is None:
        monkeypatch.delenv("XSW_LAND_BANDS", raising=False)
    else:
        monkeypatch.setenv("XSW_LAND_BANDS", bands)


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv("XSW_LAND_PATH", raising=False)
    monkeypatch.delenv("XSW_LAND_BANDS", raising=False)


def both_routes(case, torch, **kw):
    """The numpy route and the `device=` route of one call; both are returned as host arrays."""
    coast, tp = case.coastline(), case.tie_points()
    a = land_mask(coast, tp, **case.raster(), **kw)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8
    b = land_mask(coast, tp, device="cuda:0", **case.raster(), **kw)
    assert isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.uint8
    return a, host(b)


@pytest.mark.parametrize("path,bands", CONFIGS)
def test_every_small_case(torch, monkeypatch, path, bands):
    chunk = _lib.land_chunk_edges()
    set_knobs(monkeypatch, path, bands)
    for name, case in lc.small_cases(chunk).items():
        want = case.want()
        for got in both_routes(case, torch):
            assert lref.same_bytes(got, want), (name, path, bands, int((got != want).sum()) if got.shape == want.shape else got.shape)


@pytest.mark.parametrize("path", ["bands", "direct"])
def test_strip_raster(torch, monkeypatch, path):
    """8197 x 1030: two workgroup columns, five lines per workgroup (a line group of four and one more line), a last workgroup of
    two; 1030 samples: bytes stored one by one."""
    case = lc.strip_case()
    lc.check_strip_geometry(case)
    want = case.want()
    land = want == 0
    assert 0.1 < land[lc.strip_rows(1)].mean() < 0.9 and 0.1 < land[lc.strip_rows(-1)].mean() < 0.9
    set_knobs(monkeypatch, path, None)
    got = land_mask(case.coastline(), case.tie_points(), shape=case.shape, device="cuda:0")
    assert lref.same_bytes(host(got), want)


def test_and_with_and_invert(torch, monkeypatch):
    case = lc.small_cases(_lib.land_chunk_edges())["archipelago"]
    coast, tp, want = case.coastline(), case.tie_points(), case.want()
    rng = np.random.default_rng(3)
    valid = rng.uniform(size=want.shape) < 0.7
    assert (valid & (want == 0)).any() and (~valid & (want == 1)).any()
    for path in ("bands", "direct"):
        monkeypatch.setenv("XSW_LAND_PATH", path)
        inverted = land_mask(coast, tp, shape=want.shape, invert=True)
        assert lref.same_bytes(inverted, 1 - want)
        got = land_mask(coast, tp, shape=want.shape, and_with=valid)  # numpy bool
        assert isinstance(got, np.ndarray) and lref.same_bytes(got, want & valid)
        sevens = torch.from_numpy(valid.astype(np.uint8) * 7).to("cuda:0")  # device uint8: non-zero counts as 1
        got = land_mask(coast, tp, shape=want.shape, and_with=sevens)
        assert isinstance(got, torch.Tensor) and got.is_cuda and lref.same_bytes(host(got), want & valid)
        got = land_mask(coast, tp, shape=want.shape, and_with=torch.from_numpy(valid).to("cuda:0"), invert=True)
        assert lref.same_bytes(host(got), (1 - want) & valid)  # AND-ed in after the inversion
        got = land_mask(coast, tp, shape=want.shape, and_with=valid, invert=True, device="cuda:0")
        assert got.is_cuda and lref.same_bytes(host(got), (1 - want) & valid)
    # an odd sample count: bytes one by one
    odd = lc.small_case("odd", case.rings, sample=np.arange(297.0))
    valid = rng.uniform(size=odd.shape) < 0.7
    assert lref.same_bytes(land_mask(odd.coastline(), odd.tie_points(), **odd.raster(), and_with=valid),
                           lref.land_mask(odd.rings, odd.tie_line, odd.tie_sample, odd.tie_lon, odd.tie_lat, odd.line, odd.sample, and_with=valid))


def raw_args(case, plan, out, n_bands=None, and_with=None, mem=None, band_start=None, band_edges=None):
    """The arguments of land_mask_raw on host buffers; the arrays are returned too, so that they outlive the call."""
    tp = case.tie_points()
    lf, lt = lref.bracket(case.tie_line, case.line)
    sf, st = lref.bracket(case.tie_sample, case.sample)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (tp.longitude, tp.latitude, lt, st, plan.edges)]
    keep += [lf.astype(np.int32), sf.astype(np.int32), plan.band_start if band_start is None else band_start,
             plan.band_edges if band_edges is None else band_edges]
    lon, lat, lt, st, edges, lf, sf, bstart, bedges = keep
    nb = plan.n_bands if n_bands is None else n_bands
    ptr = lambda a: a.ctypes.data
    args = (case.shape[0], case.shape[1], _lib.MEM_HOST if mem is None else mem, len(case.tie_line), len(case.tie_sample), ptr(lon), ptr(lat), ptr(lf),
            ptr(lt), ptr(sf), ptr(st), len(edges), ptr(edges), nb, ptr(bstart) if nb else None, len(bedges) if nb else 0, ptr(bedges) if nb else None,
            plan.lat0, plan.h, None if and_with is None else ptr(and_with), 0, ptr(out))
    return args, keep


def test_raw_entry_on_host_buffers():
    """xsw_land_mask itself: n_bands = 0 with NULL band arrays (the direct kernel), and with a plan; no edges at all."""
    ctx = _lib.default_context(0)
    case = lc.small_cases(_lib.land_chunk_edges())["archipelago"]
    want = case.want()
    plan = landmask.plan(case.coastline(), case.tie_points(), n_bands=64)
    for nb in (0, None):
        got = np.full(want.shape, 7, np.uint8)
        args, keep = raw_args(case, plan, got, n_bands=nb)
        ctx.land_mask_raw(*args)
        assert lref.same_bytes(got, want), nb
    got = np.full(want.shape, 7, np.uint8)
    args, keep = raw_args(case, plan, got, n_bands=0)
    args = args[:11] + (0, None) + args[13:]
    ctx.land_mask_raw(*args)
    assert (got == 1).all()  # no edges: all water


def test_raw_entry_refusals(monkeypatch):
    ctx = _lib.default_context(0)
    case = lc.small_cases(_lib.land_chunk_edges())["archipelago"]
    plan = landmask.plan(case.coastline(), case.tie_points(), n_bands=64)
    got = np.full(case.shape, 7, np.uint8)
    outside = plan.band_edges.copy()
    outside[len(outside) // 2] = len(plan.edges)
    negative = plan.band_edges.copy()
    negative[0] = -1
    descending = plan.band_start.copy()
    descending[10] = descending[9] - 1
    beyond = plan.band_start.copy()
    beyond[-1] += 1
    for what, kw in (("band_edges", dict(band_edges=outside)), ("band_edges", dict(band_edges=negative)), ("band_start", dict(band_start=descending)),
                     ("band_start", dict(band_start=beyond)), ("mem", dict(mem=7)), ("n_bands", dict(n_bands=65537))):
        args, keep = raw_args(case, plan, got, **kw)
        with pytest.raises(_lib.XswError, match=what):
            ctx.land_mask_raw(*args)
    args, keep = raw_args(case, plan, got)
    with pytest.raises(_lib.XswError, match="n_edges"):
        ctx.land_mask_raw(*(args[:11] + (-1,) + args[12:]))
    with pytest.raises(_lib.XswError, match="invert"):
        ctx.land_mask_raw(*(args[:20] + (2,) + args[21:]))
    monkeypatch.setenv("XSW_LAND_PATH", "lanes")  # read by the library at every call
    with pytest.raises(_lib.XswError, match="XSW_LAND_PATH"):
        ctx.land_mask_raw(*args)
    monkeypatch.delenv("XSW_LAND_PATH")
    assert (got == 7).all()  # a refused call writes nothing
    ctx.land_mask_raw(*args)
    assert lref.same_bytes(got, case.want())


def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):
    """A device `and_with` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns
    while the producer is still in flight and its result is that of the filled values."""
    dev = torch.device("cuda", 0)
    case = lc.small_cases(_lib.land_chunk_edges())["archipelago"]
    coast, tp, want = case.coastline(), case.tie_points(), case.want()
    rng = np.random.default_rng(8)
    valid = (rng.uniform(size=want.shape) < 0.6).astype(np.uint8)
    decoy = 1 - valid
    assert not lref.same_bytes(want & decoy, want & valid)
    buf, src = (torch.from_numpy(a.copy()).to(dev) for a in (decoy, valid))
    land_mask(coast, tp, shape=want.shape, and_with=src)  # once on landed values: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = land_mask(coast, tp, shape=want.shape, and_with=buf)
        _in_flight(done)
        got, = _read_back(torch, P, out)
    assert lref.same_bytes(got, want & valid)


def test_mask_feeds_the_cells_and_the_grid(torch):
    """The device mask as `keep=` of wind_cells and wind_grid on a 64 x 64 scene: every output equals, bit for bit, what the same
    call gives with the restatement's mask."""
    dev = torch.device("cuda", 0)
    n = 64
    tie_line, tie_sample = np.array([0.0, 20.0, 63.0]), np.array([0.0, 40.5, 63.0])
    glon = 11.0 + 1.0 * tie_sample[None, :] / 63.0 + 0.1 * tie_line[:, None] / 63.0
    glat = 2.5 - 0.8 * tie_line[:, None] / 63.0 + 0.1 * tie_sample[None, :] / 63.0
    rng = np.random.default_rng(13)
    heading = -168.0 + rng.uniform(-1, 1, (3, 3))
    rings = [lc.star(11.5, 2.1, 0.3, 80, 5), lc.box(10.0, 0.0, 13.0, 1.9)]
    case = lc.Case("integration", rings, tie_line, tie_sample, glon, glat, np.arange(n), np.arange(n))
    want = case.want()
    assert 0.2 < (want == 0).mean() < 0.8
    tp = TiePoints(tie_line, tie_sample, glon, glat, heading)
    got = land_mask(case.coastline(), tp, shape=(n, n), device=dev)
    assert lref.same_bytes(host(got), want)
    ref = torch.from_numpy(want.copy()).to(dev)
    wind = torch.from_numpy(rng.normal(0, 7, (n, n)) + 1j * rng.normal(0, 7, (n, n))).to(dev)
    a, b = wind_cells(wind, (8, 8), tie_points=tp, keep=got), wind_cells(wind, (8, 8), tie_points=tp, keep=ref)
    assert 0 < host(a.count).sum() < n * n and host(a.count).sum() == int(want.sum())
    for name in ("count", "wind", "wspd", "wspd_std", "steadiness", "u", "v"):
        assert bits_equal(host(a[name]), host(b[name])), name
    spec = dict(lon=(11.0, 0.125, 10), lat=(1.5, 0.125, 10))
    a, b = wind_grid(wind, tp, keep=got, **spec), wind_grid(wind, tp, keep=ref, **spec)
    assert 0 < int(host(a.sums)[0].sum()) <= int(want.sum()) and np.array_equal(host(a.sums), host(b.sums))
    free = wind_grid(wind, tp, **spec)
    assert int(host(free.sums)[0].sum()) > int(host(a.sums)[0].sum())  # the mask took land out
