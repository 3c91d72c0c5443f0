"""xsarsea_amd.cells on the MI355X against its CPU restatement (tests/cells_ref.py).  Every comparison is bit for bit
(`cells_ref.same_bits`: NaN where and only where the restatement has NaN, payloads aside, every other value equal as uint64,
`count` equal), over every cell, in both forced mappings (XSW_CELLS_MAPPING = wave / workgroup, read at every call) and in the
default one.  k_cells owns a cell with one wave or one workgroup and does not loop over cells, so there is no grid cap to
read: the 600 x 700 raster of (1, 1) cells sends 105 000 workgroups (wave mapping) and 420 000 (workgroup mapping) through it.
The one bound in this file is the round trip's, a constant of tests/test_cells_cpu.py."""
import functools
import warnings

import numpy as np
import pytest

import ancillary_model_ref as aref
import cells_ref as cref
from test_cells_cpu import ROUND_TRIP_BOUND, round_trip, round_trip_scene
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from xsarsea_amd import TiePoints, _lib, ancillary_from_model, raster_cells, wind_cells, windspeed
from xsarsea_amd.windspeed.crosspol import CopolCodes

pytestmark = pytest.mark.gpu

L, S = 83, 150
CELLS = [(3, 3),       # N = 9, below one wave
         (10, 13),     # 130: between 64 and 256
         (17, 31),     # 527: two or three pixels per accumulator; clipped last row and column, so w changes
         (40, 37),     # 1480: more than one trip of a lane's four accumulators, with a tail
         (1, 1),       # std NaN, count 0 / 1
         (200, 200)]   # one clipped cell holds the whole raster
WIND_NAMES = ("count", "wind", "wspd", "wspd_std", "steadiness")
REAL_NAMES = ("count", "mean", "std")
GEO_NAMES = ("longitude", "latitude", "u", "v")


@pytest.fixture(params=["default", "wave", "workgroup"])
def mapping(request, monkeypatch):
    if request.param == "default":
        monkeypatch.delenv("XSW_CELLS_MAPPING", raising=False)
    else:
        monkeypatch.setenv("XSW_CELLS_MAPPING", request.param)
    return request.param


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def up(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))  # a copy: the cached cases are read-only


def assert_same(got, want, names, what=""):
    for name in names:
        g = host(got[name])
        assert cref.same_bits(g, want[name]), f"{what} {name}: {int((g != want[name]).sum())} cells differ (NaN counted)"


def special_cells(cell):
    """Pixel slices of three cells of the grid (None for a grid of fewer than four cells): one to fill with NaN, the clipped
    last one to leave with exactly one valid pixel, one to empty with `keep` alone."""
    cl, cs = cell
    nl, ns = -(-L // cl), -(-S // cs)
    if nl * ns < 4:
        return None
    box = lambda i, j: (slice(i * cl, min((i + 1) * cl, L)), slice(j * cs, min((j + 1) * cs, S)))
    return box(0, 0), box(nl - 1, ns - 1), box(0, 1)


@functools.lru_cache(maxsize=None)
def wind_case(cell, dtype):
    """(wind, keep, restatement) for one cell shape: winds of 8 +- 3 m/s, the three kinds of invalid pixel sprinkled, a keep
    mask with a tenth of zeros, and the three special cells."""
    rng = np.random.default_rng(100 + cell[0])
    w = rng.normal(8.0, 3.0, (L, S)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (L, S)))
    kind = rng.uniform(size=(L, S))
    w[kind < 0.02] = complex(np.nan, 0.0)
    w[(kind >= 0.02) & (kind < 0.04)] = complex(np.nan, np.nan)
    w.imag[(kind >= 0.04) & (kind < 0.06)] = np.nan        # finite + NaN j
    keep = rng.uniform(size=(L, S)) < 0.9
    boxes = special_cells(cell)
    if boxes:
        w[boxes[0]] = complex(np.nan, np.nan)
        one = w[boxes[1]].copy()
        one[:] = complex(np.nan, 0.0)
        one[-1, -1] = 3.0 - 4.0j
        w[boxes[1]] = one
        keep[boxes[1]] = True
        keep[boxes[2]] = False
        w[boxes[2]][0, 0] = 5.0 + 5.0j   # the source itself is valid there: `keep` alone empties the cell
    w = w.astype(dtype)
    w.setflags(write=False)
    keep.setflags(write=False)
    want = cref.wind(w, cell, keep)
    if boxes:
        nl, ns = want["count"].shape
        assert want["count"][0, 0] == 0 and want["count"][-1, -1] == 1 and want["count"][0, 1] == 0
        assert np.isnan(want["wspd_std"][-1, -1]) and want["wind"][-1, -1] == 3.0 - 4.0j
    return w, keep, want


@functools.lru_cache(maxsize=None)
def real_case(cell, dtype):
    rng = np.random.default_rng(200 + cell[0])
    x = rng.uniform(0.01, 0.3, (L, S)).astype(dtype)
    x[rng.uniform(size=(L, S)) < 0.05] = np.nan
    keep = (rng.uniform(size=(L, S)) < 0.9).astype(np.uint8) * 3   # any non-zero byte keeps
    boxes = special_cells(cell)
    if boxes:
        x[boxes[0]] = np.nan
        keep[boxes[2]] = 0
    x.setflags(write=False)
    keep.setflags(write=False)
    return x, keep, cref.real(x, cell, keep)


# ------------------------------------------------------------------------------------------------------------------ wind_cells
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("cell", CELLS)
def test_wind_cells(torch, mapping, cell, dtype):
    w, keep, want = wind_case(cell, dtype)
    got = wind_cells(up(torch, w), cell, keep=up(torch, keep))
    assert isinstance(got.wind, torch.Tensor) and got.wind.is_cuda and got.wind.dtype == torch.complex128 and got.count.dtype == torch.int32
    assert got.longitude is None and got.u is None and got.direction is None
    assert_same(got, want, WIND_NAMES, f"{cell} {mapping}")
    np.testing.assert_array_equal(got.line, cref.centres(np.arange(L), cell[0]))
    np.testing.assert_array_equal(got.sample, cref.centres(np.arange(S), cell[1]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cell", CELLS)
def test_raster_cells(torch, mapping, cell, dtype):
    x, keep, want = real_case(cell, dtype)
    got = raster_cells(up(torch, x), cell, keep=up(torch, keep))
    assert got.mean.is_cuda and got.mean.dtype == torch.float64 and got.count.dtype == torch.int32
    assert_same(got, want, REAL_NAMES, f"{cell} {mapping}")
    if cell == (17, 31):  # no keep: the NULL pointer's path
        assert_same(raster_cells(up(torch, x), cell), cref.real(x, cell), REAL_NAMES, "no keep")


@pytest.mark.parametrize("cell", [(3, 3), (17, 31), (200, 200)])
def test_numpy_route_and_device_route_give_the_same_bits(torch, mapping, cell):
    w, keep, want = wind_case(cell, np.complex128)
    a = wind_cells(w, cell, keep=keep)
    assert isinstance(a.wind, np.ndarray) and a.wind.dtype == np.complex128 and a.count.dtype == np.int32
    assert_same(a, want, WIND_NAMES, "numpy")
    b = wind_cells(up(torch, w), cell)                  # no keep
    c = wind_cells(w, cell)
    assert_same(b, cref.wind(w, cell), WIND_NAMES, "device, no keep")
    for name in WIND_NAMES:
        assert cref.same_bits(c[name], host(b[name]))
    x, kx, wantx = real_case(cell, np.float32)
    r = raster_cells(x, cell, keep=kx)
    assert isinstance(r.mean, np.ndarray)
    assert_same(r, wantx, REAL_NAMES, "numpy")


def test_outputs_left_out_are_never_written(torch):
    """The raw entry on host buffers with only `count` and `wspd_std` asked for; bad arguments are refused with XSW_EINVAL."""
    ctx = _lib.default_context(0)
    w, keep, want = wind_case((10, 13), np.complex128)
    nl, ns = want["count"].shape
    count, std = np.full((nl, ns), -7, np.int32), np.full((nl, ns), -7.0)
    k8 = np.ascontiguousarray(keep).view(np.uint8)
    args = lambda **o: (L, S, _lib.MEM_HOST, o.get("kind", _lib.CELLS_C128), w.ctypes.data, k8.ctypes.data, o.get("cl", 10), o.get("cs", 13), 0, 0,
                        *[None] * 8, count.ctypes.data, None, None, std.ctypes.data, None, None, None, o.get("u"), None)
    ctx.wind_cells_raw(*args())
    assert cref.same_bits(count, want["count"]) and cref.same_bits(std, want["wspd_std"])
    for bad in (dict(cl=0), dict(cs=-2), dict(kind=3), dict(u=std.ctypes.data)):  # u without tie points
        with pytest.raises(_lib.XswError):
            ctx.wind_cells_raw(*args(**bad))
    with pytest.raises(_lib.XswError):
        ctx.raster_cells_raw(L, S, _lib.MEM_HOST, 7, w.ctypes.data, None, 3, 3, count.ctypes.data, None, None)
    with pytest.raises(ValueError, match="container kind"):
        wind_cells(up(torch, w), (3, 3), keep=keep)


def test_forced_mapping_must_be_one_of_the_two(monkeypatch):
    monkeypatch.setenv("XSW_CELLS_MAPPING", "lanes")
    with pytest.raises(_lib.XswError, match="XSW_CELLS_MAPPING"):
        raster_cells(np.ones((4, 4)), (2, 2))


# ---------------------------------------------------------------------------------------------------------------------- codes
@functools.lru_cache(maxsize=None)
def codes_scene():
    n = 64
    inc, s_vv, _, _, anc = synthetic_scene(n, n, np.float64, 31)   # its first three columns have a NaN incidence
    anc[5, 10:20] = np.nan
    anc[42:49, 27:36] = complex(np.nan, np.nan)                     # a whole (7, 9) cell without an a-priori wind
    return inc, s_vv, anc


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("cell", [(7, 9), (1, 1), (64, 64)])
def test_cells_from_codes(torch, mapping, cell, where):
    inc, s_vv, anc = codes_scene()
    on = (lambda a: up(torch, a)) if where == "device" else (lambda a: a)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(on(inc), on(s_vv), ancillary_wind=on(anc), model="gmf_cmod5n", resolution="low")
    raw = host(cc.codes).view(np.uint32).copy()
    assert ((raw & 0x80000000) != 0).sum() > 64 * 3   # NaN incidence / a-priori pixels are there
    raw[20, 30] = 0x80000005          # a code of no LUT: bit 31
    raw[21, 31] = 0x3FFFFFFF          # and one whose index lies beyond this LUT's plane
    codes = CopolCodes(on(inc), on(raw.view(np.int32)) if where == "device" else raw, cc.lut_co)
    expanded = codes.wind()
    wh = host(expanded)
    assert wh.dtype == np.complex128 and np.isnan(wh[20, 30].real) and np.isnan(wh[21, 31].real) and (~np.isnan(wh.real)).mean() > 0.8
    keep = np.random.default_rng(5).uniform(size=wh.shape) < 0.9
    for k in (None, keep):
        got = codes.cells(cell, keep=None if k is None else on(k))
        assert (hasattr(got.wind, "is_cuda") and got.wind.is_cuda) == (where == "device")
        other = wind_cells(expanded, cell, keep=None if k is None else on(k))
        want = cref.wind(wh, cell, k)
        assert_same(got, want, WIND_NAMES, "codes vs restatement")
        for name in WIND_NAMES:
            assert cref.same_bits(host(got[name]), host(other[name])), name
    if cell == (7, 9):
        assert want["count"].min() == 0 and want["count"].max() > 40


# ----------------------------------------------------------------------------------------------------------------- tie points
def antimeridian_ties():
    """A 3 x 4 tie grid over the 83 x 150 raster, longitudes given wrapped across the antimeridian, varying headings."""
    tl, ts = np.array([0.0, 30.0, 82.0]), np.array([0.0, 40.5, 100.0, 149.0])
    lon = np.array([178.2, 179.4, -179.1, -177.9])[None, :] + np.array([0.0, 0.3, 0.8])[:, None]
    lat = np.array([12.0, 11.2, 9.9])[:, None] + 0.25 * ts[None, :] / 149.0
    heading = -168.0 + np.array([0.0, 0.7, 2.2])[:, None] + 1.5 * ts[None, :] / 149.0
    return tl, ts, lon, lat, heading


@pytest.mark.parametrize("cell", [(17, 31), (3, 3), (200, 200)])
def test_tie_points_across_the_antimeridian(torch, mapping, cell):
    tl, ts, lon, lat, heading = antimeridian_ties()
    w, keep, want = wind_case(cell, np.complex128)
    tp = TiePoints(tl, ts, lon, lat, heading)
    assert tp.longitude.max() > 180.0
    cline, csample = cref.centres(np.arange(L), cell[0]), cref.centres(np.arange(S), cell[1])
    geo = cref.geo(want["wind"], tl, ts, lon, lat, heading, cline, csample)
    assert geo["longitude"].max() > 180.0 or cell == (200, 200)
    for got in (wind_cells(up(torch, w), cell, keep=up(torch, keep), tie_points=tp), wind_cells(w, cell, keep=keep, tie_points=tp)):
        assert_same(got, want, WIND_NAMES)
        assert_same(got, geo, GEO_NAMES, "geo")
        d = host(got.direction)
        ok = ~np.isnan(geo["u"])
        off = (d - (270.0 - np.degrees(np.arctan2(geo["v"], geo["u"]))) + 180.0) % 360.0 - 180.0
        assert np.isnan(d[~ok]).all() and np.abs(off[ok]).max() < 1e-9  # the one value not pinned to the bit


def test_single_tie_line_and_cancelling_headings(torch, mapping):
    rng = np.random.default_rng(9)
    w = (rng.normal(8.0, 3.0, (1, S)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (1, S))))
    ts = np.array([0.0, 70.0, 149.0])
    lon, lat = np.array([[10.0, 10.6, 11.3]]), np.array([[4.0, 4.1, 4.3]])
    heading = np.array([[-170.0, 10.0, 12.0]])    # opposite at tie columns 0 and 70: they cancel half-way, at sample 35
    tp = TiePoints([5.0], ts, lon, lat, heading)
    tp.cos_heading[0, 1], tp.sin_heading[0, 1] = -tp.cos_heading[0, 0], -tp.sin_heading[0, 0]  # exactly opposite tables
    cell = (1, 71)                                 # centres at samples 35, 106, 145.5
    want = cref.wind(w, cell)
    lf, lt = aref.bracket([5.0], [5.0])
    sf, st = aref.bracket(ts, cref.centres(np.arange(S), 71))
    geo = cref.geo_core(want["wind"], tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading, lf, lt, sf, st)
    assert np.isnan(geo["u"][0, 0]) and np.isnan(geo["v"][0, 0]) and not np.isnan(want["wind"][0, 0]) and not np.isnan(geo["u"][0, 1:]).any()
    for got in (wind_cells(up(torch, w), cell, tie_points=tp, line=[5.0]), wind_cells(w, cell, tie_points=tp, line=[5.0])):
        assert_same(got, want, WIND_NAMES)
        assert_same(got, geo, GEO_NAMES, "geo")
        assert np.isfinite(host(got.longitude)).all()


# ------------------------------------------------------------------------------------------------------- many cells, one launch
@pytest.mark.parametrize("cell", [(1, 1), (2, 3)])
def test_many_cells(torch, mapping, cell):
    rng = np.random.default_rng(17)
    Lb, Sb = 600, 700
    w = rng.normal(8.0, 3.0, (Lb, Sb)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (Lb, Sb)))
    w[rng.uniform(size=w.shape) < 0.05] = np.nan
    w[100:104, 300:306] = np.nan
    want = cref.wind(w, cell)
    assert want["count"].shape == (Lb // cell[0], -(-Sb // cell[1])) and want["count"].min() == 0
    assert_same(wind_cells(up(torch, w), cell), want, WIND_NAMES)
    x = w.real.astype(np.float32)
    assert_same(raster_cells(up(torch, x), cell), cref.real(x, cell), REAL_NAMES)


# ------------------------------------------------------------------------------------------------------------------- streams
def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):
    """`wind` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns while the
    producer is still in flight and its result is that of the filled values."""
    dev = torch.device("cuda", 0)
    cell = (17, 31)
    w, keep, want = wind_case(cell, np.complex128)
    decoy = np.where(np.isnan(w.real), w, w * 0.5)
    assert not cref.same_bits(cref.wind(decoy, cell, keep)["wspd"], want["wspd"])
    tl, ts, lon, lat, heading = antimeridian_ties()
    tp = TiePoints(tl, ts, lon, lat, heading)
    geo = cref.geo(want["wind"], tl, ts, lon, lat, heading, cref.centres(np.arange(L), 17), cref.centres(np.arange(S), 31))
    buf, src, tk = up(torch, decoy), up(torch, w), up(torch, keep)
    wind_cells(src, cell, keep=tk, tie_points=tp)   # once on landed values: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = wind_cells(buf, cell, keep=tk, tie_points=tp)
        _in_flight(done)
        got = _read_back(torch, P, out.count, out.wind, out.wspd, out.wspd_std, out.steadiness, out.u, out.v)
    for name, g in zip(WIND_NAMES + ("u", "v"), got):
        assert cref.same_bits(g, {**want, **geo}[name]), name


# ---------------------------------------------------------------------------------------------------------------- round trip
def test_round_trip_on_the_device(torch):
    """device ancillary_from_model -> wind_cells with the same tie points returns the model's (u, v), within the bound of
    tests/test_cells_cpu.py; the device chain equals the restatements' chain bit for bit."""
    sc = round_trip_scene()
    tp = TiePoints(sc["tl"], sc["ts"], sc["glon"], sc["glat"], sc["heading"])
    raster = ancillary_from_model(sc["u"], sc["v"], sc["mlon"], sc["mlat"], tp, shape=(sc["L"], sc["S"]), device="cuda:0")
    got = wind_cells(raster, sc["cell"], tie_points=tp)
    u, v = host(got.u), host(got.v)
    print(f"largest |u - model u| = {np.abs(u - sc['u0']).max():.3g}, |v - model v| = {np.abs(v - sc['v0']).max():.3g} (bound {ROUND_TRIP_BOUND:g})")
    assert np.abs(u - sc["u0"]).max() <= ROUND_TRIP_BOUND and np.abs(v - sc["v0"]).max() <= ROUND_TRIP_BOUND
    ru, rv = round_trip(sc)
    assert cref.same_bits(u, ru) and cref.same_bits(v, rv)
    assert int(host(got.count).sum()) == sc["L"] * sc["S"]
