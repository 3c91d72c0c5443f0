"""xsarsea_amd.ancillary on the MI355X against its CPU restatement (tests/ancillary_model_ref.py).  Every comparison is bit for
bit (`same_bits`: NaN where and only where the restatement has NaN, payloads aside, every other part equal as uint64): the kernel
and the restatement round the same operations in the same order, and neither calls a trigonometric function on the device."""
import warnings

import numpy as np
import pytest

import ancillary_model_ref as aref
import strip_shapes
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from util import bits_equal
from xsarsea_amd import TiePoints, _lib, ancillary_from_model, streaks

pytestmark = pytest.mark.gpu

L, S = 37, 300  # one full 256-column block and a 44-lane one; 37 lines: the line loop ends inside a group of four
TIE_LINE = np.array([0.0, 4.0, 36.0])          # non-uniform, dyadic weights; raster line 4 is a tie line
TIE_SAMPLE = np.array([0.0, 70.0, 256.0, 299.0])  # raster column 256 is a tie column


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def model_fields(shape, dtype, seed, nan_at=None):
    rng = np.random.default_rng(seed)
    u, v = rng.normal(0, 12, shape).astype(dtype), rng.normal(0, 12, shape).astype(dtype)
    if nan_at is not None:
        u[nan_at] = np.nan
    return u, v


def regional_scene():
    """Over the regional grid lon 10 .. 18, lat -3 .. 3 (7 x 9 nodes): the scene leaves it to the west (lon < 10), to the east
    (lon > 18), to the north (lat > 3) and to the south (lat < -3), and column 256 lies exactly on the last longitude node (its
    tie longitudes are 18 on every tie line and the line weights are dyadic, so the blend is exact)."""
    lon = np.array([9.25, 11.5, 18.0, 19.5])[None, :] + np.array([0.0, 0.125, 0.5])[:, None] * np.array([1.0, 1.0, 0.0, 1.0])[None, :]
    lat = np.array([4.0, 2.9, -3.6])[:, None] + 0.2 * TIE_SAMPLE[None, :] / 299.0
    heading = -168.0 + np.array([0.0, 0.4, 2.5])[:, None] + 1.5 * TIE_SAMPLE[None, :] / 299.0
    return lon, lat, heading


def both_routes(u, v, lon, lat, tp, torch, **raster):
    """The numpy route and the `device=` route of one call; both are returned as host arrays."""
    a = ancillary_from_model(u, v, lon, lat, tp, **raster)
    assert isinstance(a, np.ndarray) and a.dtype == np.complex128
    b = ancillary_from_model(u, v, lon, lat, tp, device="cuda:0", **raster)
    assert isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.complex128
    return a, host(b)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_raster_over_a_regional_grid(torch, dtype, descending):
    glon, glat, heading = regional_scene()
    u, v = model_fields((7, 9), dtype, 1, nan_at=(2, 4))
    mlon, mlat = 10.0 + np.arange(9), -3.0 + np.arange(7)
    if descending:
        u, v, mlat = u[::-1].copy(), v[::-1].copy(), mlat[::-1].copy()
    want = aref.ancillary_from_model(u, v, mlon, mlat, TIE_LINE, TIE_SAMPLE, glon, glat, heading, np.arange(L), np.arange(S))
    nan = np.isnan(want.real)
    assert nan[:, 0].all() and nan[:, -1].all() and nan[0].all() and nan[-1].all()     # west, east, north, south
    assert not nan[5:30, 256].any() and nan[5:30, 257].all()                           # the last longitude node, and just beyond it
    assert 0.2 < nan.mean() < 0.8 and nan[8:30, 100:200].any() and not nan[8:30, 100:200].all()  # the NaN node's four cells
    tp = TiePoints(TIE_LINE, TIE_SAMPLE, glon, glat, heading)
    for got in both_routes(u, v, mlon, mlat, tp, torch, shape=(L, S)):
        assert aref.same_bits(got, want)
    if descending:  # what the flipped grid gives, bit for bit
        assert aref.same_bits(ancillary_from_model(u[::-1].copy(), v[::-1].copy(), mlon, mlat[::-1].copy(), tp, shape=(L, S)), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_raster_over_the_periodic_grid(torch, dtype):
    """Nodes 0 .. 315 step 45: the tie longitudes run 150 -> 380, across the antimeridian (given wrapped) and across the grid's
    own seam between node 7 (315) and node 0."""
    wrapped = np.array([150.0, -160.0, -30.0, 20.0])[None, :] + np.array([0.0, 1.5, 9.0])[:, None]
    glat = np.array([8.0, 5.5, -8.0])[:, None] - 0.7 * TIE_SAMPLE[None, :] / 299.0
    heading = 11.0 + np.array([0.0, -0.4, -2.5])[:, None] + 1.5 * TIE_SAMPLE[None, :] / 299.0
    u, v = model_fields((3, 8), dtype, 2)
    mlon, mlat = 45.0 * np.arange(8), np.array([-10.0, 0.0, 10.0])
    tp = TiePoints(TIE_LINE, TIE_SAMPLE, wrapped, glat, heading)
    np.testing.assert_array_equal(tp.longitude[0], [150.0, 200.0, 330.0, 380.0])
    want = aref.ancillary_from_model(u, v, mlon, mlat, TIE_LINE, TIE_SAMPLE, wrapped, glat, heading, np.arange(L), np.arange(S))
    assert not np.isnan(want.real).any()
    for got in both_routes(u, v, mlon, mlat, tp, torch, line=np.arange(L), sample=np.arange(S)):
        assert aref.same_bits(got, want)


def test_degenerate_axes(torch):
    glon, glat, heading = regional_scene()
    u, v = model_fields((7, 9), np.float64, 3)
    mlon, mlat = 10.0 + np.arange(9), -3.0 + np.arange(7)
    tp = TiePoints(TIE_LINE, TIE_SAMPLE, glon, glat, heading)
    cases = [(np.array([7.0]), np.arange(float(S))), (np.arange(float(L)), np.array([131.5])), (np.array([36.0]), np.array([299.0]))]
    for line, sample in cases:  # L = 1, S = 1, one pixel
        want = aref.ancillary_from_model(u, v, mlon, mlat, TIE_LINE, TIE_SAMPLE, glon, glat, heading, line, sample)
        assert not np.isnan(want.real).all() or len(line) * len(sample) == 1
        for got in both_routes(u, v, mlon, mlat, tp, torch, line=line, sample=sample):
            assert got.shape == (len(line), len(sample)) and aref.same_bits(got, want)
    # a single tie line under a one-line raster
    one = TiePoints([5.0], TIE_SAMPLE, glon[1:2], glat[1:2], heading[1:2])
    want = aref.ancillary_from_model(u, v, mlon, mlat, [5.0], TIE_SAMPLE, glon[1:2], glat[1:2], heading[1:2], [5.0], np.arange(float(S)))
    assert not np.isnan(want.real).all()
    for got in both_routes(u, v, mlon, mlat, one, torch, line=[5.0], sample=np.arange(float(S))):
        assert aref.same_bits(got, want)
    # a 2 x 2 model grid: one cell
    u2, v2 = model_fields((2, 2), np.float32, 4)
    want = aref.ancillary_from_model(u2, v2, [9.0, 20.0], [5.0, -4.0], TIE_LINE, TIE_SAMPLE, glon, glat, heading, np.arange(L), np.arange(S))
    assert not np.isnan(want.real).any()
    for got in both_routes(u2, v2, [9.0, 20.0], [5.0, -4.0], tp, torch, shape=(L, S)):
        assert aref.same_bits(got, want)
    empty = ancillary_from_model(u, v, mlon, mlat, tp, line=np.empty(0), sample=np.arange(float(S)))
    assert empty.shape == (0, S) and empty.dtype == np.complex128


def test_raw_entry_with_a_descending_axis_and_cancelling_headings():
    """xsw_ancillary_model itself on host buffers: dlat < 0 (the public call never passes one: it reads a descending axis
    backwards), and tie tables whose blended heading vector is exactly 0 half-way (the pixel is NaN)."""
    ctx = _lib.default_context(0)
    glon, glat, heading = regional_scene()
    u, v = model_fields((7, 9), np.float64, 5, nan_at=(4, 7))
    h = np.deg2rad(heading)
    tcos, tsin = np.cos(h), np.sin(h)
    tcos[:, 1], tsin[:, 1] = -tcos[:, 0], -tsin[:, 0]  # opposite headings at tie columns 0 and 70: they cancel at column 35
    lf, lt = aref.bracket(TIE_LINE, np.arange(L))
    sf, st = aref.bracket(TIE_SAMPLE, np.arange(S))
    want = aref.core(u, v, 10.0, 1.0, False, 3.0, -1.0, glon, glat, tcos, tsin, lf, lt, sf, st)
    assert np.isnan(want[:, 35].real).all() and not np.isnan(want[5:30, 34].real).any() and not np.isnan(want[5:30, 36].real).any()
    got = np.full((L, S), 7.0 + 7.0j)
    tables = [np.ascontiguousarray(a, dtype=np.float64) for a in (glon, glat, tcos, tsin, lt, st)]
    lf, sf = lf.astype(np.int32), sf.astype(np.int32)
    ctx.ancillary_model_raw(L, S, _lib.MEM_HOST, _lib.XSW_F64, u.ctypes.data, v.ctypes.data, 7, 9, 10.0, 1.0, 0, 3.0, -1.0, 3, 4,
                            tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, tables[3].ctypes.data, lf.ctypes.data,
                            tables[4].ctypes.data, sf.ctypes.data, tables[5].ctypes.data, got.ctypes.data)
    assert aref.same_bits(got, want)
    for bad in (dict(n_lat=1), dict(dlon=0.0), dict(dlat=float("nan")), dict(periodic=2), dict(dtype=5), dict(mem=7)):
        a = dict(mem=_lib.MEM_HOST, dtype=_lib.XSW_F64, n_lat=7, n_lon=9, dlon=1.0, periodic=0, dlat=-1.0)
        a.update(bad)
        with pytest.raises(_lib.XswError):
            ctx.ancillary_model_raw(L, S, a["mem"], a["dtype"], u.ctypes.data, v.ctypes.data, a["n_lat"], a["n_lon"], 10.0, a["dlon"], a["periodic"], 3.0,
                                    a["dlat"], 3, 4, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, tables[3].ctypes.data,
                                    lf.ctypes.data, tables[4].ctypes.data, sf.ctypes.data, tables[5].ctypes.data, got.ctypes.data)


def strip_grid(rows, cols, wg_per_cu=16):
    """csrc/xsw_plan.hpp: strip_grid, restated."""
    gx = (cols + 255) // 256
    gy = (256 * wg_per_cu + gx - 1) // gx
    gy = max(1, min(gy, rows, 65535))
    rpb = (rows + gy - 1) // gy
    gy = (rows + rpb - 1) // rpb
    return gx, gy, rpb


def test_multi_line_raster(torch):
    """4097 x 2048: nine lines per workgroup (two unrolled groups of four and one more line), a last workgroup of two.  Tie lines
    are placed so that the line bracket changes at each position 0 .. 3 of an unrolled group inside the second workgroup row, and
    inside the last one."""
    Lb, Sb = strip_shapes.shape("streaks")
    gx, gy, rpb = strip_grid(Lb, Sb)
    last = Lb - (gy - 1) * rpb
    assert (Lb, Sb) == (4097, 2048) and (gx, gy, rpb, last) == strip_shapes.SHAPES["streaks"].grid
    assert rpb > 4 and 0 < last < rpb
    tie_line = np.array([0.0, 10.0, 11.5, 13.0, 15.0, 2000.0, 4095.5, 4096.0])
    tie_sample = np.array([0.0, 700.25, 2047.0])
    first, _ = aref.bracket(tie_line, np.arange(Lb))
    changes = {int(l) for l in np.nonzero(np.diff(first))[0] + 1}
    second = strip_shapes.block_lines("streaks", 1)
    assert {(l - second[0]) % 4 for l in changes if l in second and l != second[0]} == {0, 1, 2, 3}
    assert any(l in changes for l in strip_shapes.block_lines("streaks", -1)[1:])
    rng = np.random.default_rng(6)
    glon = 9.0 + 10.5 * tie_sample[None, :] / 2047.0 + 0.6 * tie_line[:, None] / 4096.0 + rng.uniform(-0.02, 0.02, (8, 3))
    glat = 2.9 - 6.0 * tie_line[:, None] / 4096.0 + 0.3 * tie_sample[None, :] / 2047.0 + rng.uniform(-0.02, 0.02, (8, 3))
    heading = -167.0 + rng.uniform(-1.5, 1.5, (8, 3))
    u, v = model_fields((7, 9), np.float32, 7, nan_at=(1, 6))
    mlon, mlat = 10.0 + np.arange(9), 3.0 - np.arange(7)
    want = aref.ancillary_from_model(u, v, mlon, mlat, tie_line, tie_sample, glon, glat, heading, np.arange(Lb), np.arange(Sb))
    nan = np.isnan(want.real)
    assert 0.05 < nan.mean() < 0.6 and 0.1 < nan[second].mean() < 0.9 and 0.1 < nan[-2:].mean() < 0.9
    got = ancillary_from_model(u, v, mlon, mlat, TiePoints(tie_line, tie_sample, glon, glat, heading), shape=(Lb, Sb), device="cuda:0")
    assert aref.same_bits(host(got), want)


def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):
    """`model_u` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns while the
    producer is still in flight and its result is that of the filled values."""
    dev = torch.device("cuda", 0)
    glon, glat, heading = regional_scene()
    tp = TiePoints(TIE_LINE, TIE_SAMPLE, glon, glat, heading)
    (u, v), (decoy, _) = model_fields((7, 9), np.float64, 8), model_fields((7, 9), np.float64, 9)
    mlon, mlat = 10.0 + np.arange(9), -3.0 + np.arange(7)
    want = aref.ancillary_from_model(u, v, mlon, mlat, TIE_LINE, TIE_SAMPLE, glon, glat, heading, np.arange(L), np.arange(S))
    assert not aref.same_bits(aref.ancillary_from_model(decoy, v, mlon, mlat, TIE_LINE, TIE_SAMPLE, glon, glat, heading, np.arange(L), np.arange(S)), want)
    buf, src, tv = (torch.from_numpy(a.copy()).to(dev) for a in (decoy, u, v))
    ancillary_from_model(src, tv, mlon, mlat, tp, shape=(L, S))  # once on landed fields: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = ancillary_from_model(buf, tv, mlon, mlat, tp, shape=(L, S))
        _in_flight(done)
        got, = _read_back(torch, P, out)
    assert aref.same_bits(got, want)


def test_result_feeds_the_streaks_and_the_inversion(torch):
    """The device raster as `ancillary_wind` of Streaks.resolve, ancillary_from_streaks and invert_from_model on a 64 x 64 scene:
    each output equals, bit for bit, what the same call gives on the restatement's raster."""
    from xsarsea_amd import windspeed
    dev = torch.device("cuda", 0)
    n = 64
    inc, s_vv, _, _, _ = synthetic_scene(n, n, np.float64, 12)
    tie_line, tie_sample = np.array([0.0, 20.0, 63.0]), np.array([0.0, 40.5, 63.0])
    rng = np.random.default_rng(13)
    glon = 11.0 + 5.0 * tie_sample[None, :] / 63.0 + 0.5 * tie_line[:, None] / 63.0
    glat = 2.5 - 4.0 * tie_line[:, None] / 63.0 + 0.2 * tie_sample[None, :] / 63.0
    heading = -168.0 + rng.uniform(-1, 1, (3, 3))
    u, v = rng.normal(0, 7, (7, 9)), rng.normal(0, 7, (7, 9))
    mlon, mlat = 10.0 + np.arange(9), 3.0 - np.arange(7)
    want = aref.ancillary_from_model(u, v, mlon, mlat, tie_line, tie_sample, glon, glat, heading, np.arange(n), np.arange(n))
    assert not np.isnan(want.real).any()
    got = ancillary_from_model(u, v, mlon, mlat, TiePoints(tie_line, tie_sample, glon, glat, heading), shape=(n, n), device=dev)
    ref = torch.from_numpy(want).to(dev)
    assert aref.same_bits(host(got), want)
    W = torch.from_numpy(rng.uniform(0, 1, (2, 3, 4, 72))).to(dev)
    bins = np.linspace(-np.pi / 2, np.pi / 2, 72, endpoint=False)
    s = streaks.streaks_direction(W, angles=bins, line=np.array([8.0, 30.0, 55.0]), sample=np.array([5.0, 22.0, 40.0, 60.0]))
    a, b = s.resolve(got), s.resolve(ref)
    assert not np.isnan(host(a).real).any() and bits_equal(host(a), host(b))
    a, b = streaks.ancillary_from_streaks(s, got), streaks.ancillary_from_streaks(s, ref)
    assert not np.isnan(host(a).real).any() and bits_equal(host(a), host(b))
    ti, ts0 = torch.from_numpy(inc).to(dev), torch.from_numpy(s_vv).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = windspeed.invert_from_model(ti, ts0, ancillary_wind=got, model="gmf_cmod5n", resolution="low")
        b = windspeed.invert_from_model(ti, ts0, ancillary_wind=ref, model="gmf_cmod5n", resolution="low")
    assert (~np.isnan(host(a).real)).mean() > 0.9 and bits_equal(host(a), host(b))
