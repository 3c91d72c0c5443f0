"""CPU: the restatement of xsarsea_amd.grid (tests/grid_ref.py) -- its freedom from any order, what the fixed point costs against
extended precision, which side an edge belongs to on hand-checkable scenes, the finish -- and the public calls' host checks,
which all precede the first device call."""
import os
import re

import numpy as np
import pytest

import ancillary_model_ref as aref
import grid_cases as gc
import grid_ref as gref
from conftest import REPO
from test_cells_cpu import round_trip_scene
from xsarsea_amd import TiePoints, _lib, grid
from xsarsea_amd.windspeed.crosspol import CopolCodes

# A mean of n fixed-point terms: each term is within half a unit (2**-25 for Q24) of its pixel's value, the int64 sum is exact,
# and (float64(S) / n) * 2**-24 rounds twice, each time within 2**-53 of a value below 2**9: far below 2**-40.
MEAN_BOUND = 2.0 ** -25 + 2.0 ** -40


# ------------------------------------------------------------------------------------------------------------ order freedom
def test_permuted_pixels_give_equal_sums():
    p = gc.pixels()
    grid_ = gc.GRIDS["desc"]
    want, _ = gc.case("desc")
    inside, i, j = gref.bins(p["lon"], p["lat"], grid_)
    ok = p["ok"] & inside
    vec = [a[ok] for a in (j, i, p["u"], p["v"], p["sp"], p["q"])]
    rng = np.random.default_rng(4)
    for order in (np.arange(len(vec[0])), rng.permutation(len(vec[0])), np.arange(len(vec[0]))[::-1]):
        got = gref.accumulate(np.zeros_like(want), *[a[order] for a in vec])
        assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["coarse", "desc", "periodic"])
def test_row_tiles_add_up_to_the_scene(name):
    w, keep = gc.scene()
    want, _ = gc.case(name)
    total = np.zeros_like(want)
    for a, b in ((0, 1), (1, 40), (40, 41), (41, gc.L)):     # a tile of one line, tiles that end on and start at a tie line
        total += gref.sums(w[a:b], *gc.ties(), gc.GRIDS[name], line=np.arange(a, b), keep=keep[a:b])
    assert np.array_equal(total, want)


def second_scene():
    """Another scene over the same sea: other tie points (a descending pass), other winds."""
    rng = np.random.default_rng(77)
    tl, ts = np.array([0.0, 59.0]), np.array([0.0, 80.0, 199.0])
    lon = gc.wrap(179.6 + 0.003 * ts[None, :] - 0.0005 * tl[:, None])
    lat = 10.3 - 0.004 * tl[:, None] - 0.0004 * ts[None, :]
    heading = -168.0 + 0.01 * tl[:, None] + 0.0 * ts[None, :]
    w = rng.normal(0.0, 9.0, (60, 200)) + 1j * rng.normal(0.0, 9.0, (60, 200))
    w[rng.uniform(size=w.shape) < 0.05] = np.nan
    return w, (tl, ts, lon, lat, heading)


def test_scene_order_does_not_matter():
    a, keep = gc.scene()
    b, ties_b = second_scene()
    for name in ("coarse", "desc"):
        g = gc.GRIDS[name]
        ab = gref.sums(b, *ties_b, g, into=gref.sums(a, *gc.ties(), g, keep=keep))
        ba = gref.sums(a, *gc.ties(), g, keep=keep, into=gref.sums(b, *ties_b, g))
        alone = gref.sums(b, *ties_b, g)
        assert alone[0].sum() > 5000 and np.array_equal(ab, ba) and np.array_equal(ab, gc.case(name)[0] + alone)


# ------------------------------------------------------------------------------------------------------------- quantisation
@pytest.mark.parametrize("name", sorted(gc.GRIDS))
def test_means_are_within_half_a_unit_of_the_exact_means(name):
    """Per occupied bin, u, v and wspd against the exact mean of the same per-pixel float64 values, summed in longdouble."""
    p = gc.pixels()
    s, f = gc.case(name)
    inside, i, j = gref.bins(p["lon"], p["lat"], gc.GRIDS[name])
    ok = p["ok"] & inside
    occupied = s[0] > 0
    worst = 0.0
    for key, field in (("u", "u"), ("v", "v"), ("sp", "wspd")):
        exact = np.zeros(s[0].shape, np.longdouble)
        np.add.at(exact, (j[ok], i[ok]), p[key][ok].astype(np.longdouble))
        err = np.abs(f[field][occupied].astype(np.longdouble) - exact[occupied] / s[0][occupied])
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= MEAN_BOUND, (field, float(err.max()))
    print(f"{name}: largest |mean - exact mean| = {worst:.3g} (bound {MEAN_BOUND:.3g})")


# --------------------------------------------------------------------------------------------------------- which side an edge is on
def edge_scene():
    """9 lines x 65 samples whose pixels lie at longitude 10 + 0.25 s and latitude 40 + 0.5 l exactly (every weight is a dyadic
    fraction), heading 0, one wind everywhere."""
    tl, ts = np.array([0.0, 8.0]), np.array([0.0, 64.0])
    lon = np.array([[10.0, 26.0], [10.0, 26.0]])
    lat = np.array([[40.0, 40.0], [44.0, 44.0]])
    return np.full((9, 65), -3.0 - 4.0j), (tl, ts, lon, lat, np.zeros((2, 2)))


@pytest.mark.parametrize("lat", [(40.0, 1.0, 4), (44.0, -1.0, 4)])
def test_a_pixel_on_an_edge_belongs_to_the_bin_above_it(lat):
    """lon0 = 10, dlon = 1: the pixel at s = 4 k lies on the edge between bins k - 1 and k and belongs to bin k; s = 64 gives
    x == n_lon, outside.  Ascending latitudes: l = 2 k on the edge of bin k, l = 8 outside.  Descending from 44: y = 4 - l / 2,
    l = 8 - 2 k on the edge of bin k, l = 0 (y == n_lat) outside.  Either way every bin holds 2 lines x 4 samples."""
    w, ties = edge_scene()
    tl, ts, tlon, tlat, heading = ties
    lf, lt = gref.bracket(tl, np.arange(9.0))
    sf, st = gref.bracket(ts, np.arange(65.0))
    plon, plat, ch, sh = gref.geolocate(tlon, tlat, np.ones((2, 2)), np.zeros((2, 2)), lf, lt, sf, st)
    assert np.array_equal(plon, np.broadcast_to(10.0 + 0.25 * np.arange(65.0), (9, 65))) and np.array_equal(plat[:, 0], 40.0 + 0.5 * np.arange(9.0))
    g = (10.0, 1.0, 16) + lat
    inside, i, j = gref.bins(plon, plat, g)
    assert np.array_equal(i[4, :64], np.arange(64) // 4) and not inside[:, 64].any()
    if lat[1] > 0:
        assert np.array_equal(j[:8, 0], np.arange(8) // 2) and not inside[8].any() and inside[:8, :64].all()
    else:
        assert np.array_equal(j[1:, 0], (8 - np.arange(1, 9)) // 2) and not inside[0].any() and inside[1:, :64].all()
    s = gref.sums(w, *ties, g)
    assert np.array_equal(s[0], np.full((4, 16), 8))
    f = gref.finish(s)
    assert (f["u"] == 3.0).all() and (f["v"] == 4.0).all() and (f["wspd"] == 5.0).all() and (f["wspd_std"] == 0.0).all() and (f["steadiness"] == 1.0).all()
    assert (s[1] == 8 * 3 * 2 ** 24).all() and (s[4] == 8 * 25 * 2 ** 16).all()
    wide = gref.sums(w, *ties, (9.0, 1.0, 18) + lat)           # a grid that reaches beyond the scene: the pixels at s = 64 count
    assert wide[0][:, 0].sum() == 0 and np.array_equal(wide[0][:, 17], np.full(4, 2)) and wide[0].sum() == 8 * 65


# ---------------------------------------------------------------------------------------------------------------------- finish
def test_finish_of_empty_and_single_pixel_bins():
    s = np.zeros((5, 1, 3), np.int64)
    s[:, 0, 1] = [1, -3 * 2 ** 24, 4 * 2 ** 24, 5 * 2 ** 24, 25 * 2 ** 16]
    s[:, 0, 2] = [2, 0, 0, 10 * 2 ** 24, 52 * 2 ** 16]       # speeds 4 and 6 in opposite directions
    for f in (gref.finish(s), grid.WindGrid(s, grid.GridSpec((0.0, 1.0, 3), (0.0, 1.0, 1)))):
        assert np.array_equal(f["count"], [[0, 1, 2]])
        for name in ("u", "v", "wspd", "wspd_std", "steadiness"):
            assert np.isnan(f[name][0, 0]), name
        assert (f["u"][0, 1], f["v"][0, 1], f["wspd"][0, 1], f["steadiness"][0, 1]) == (-3.0, 4.0, 5.0, 1.0) and np.isnan(f["wspd_std"][0, 1])
        assert (f["u"][0, 2], f["wspd"][0, 2], f["wspd_std"][0, 2], f["steadiness"][0, 2]) == (0.0, 5.0, np.sqrt(2.0), 0.0)


@pytest.mark.parametrize("name", sorted(gc.GRIDS))
def test_the_package_finishes_as_the_restatement_does(name):
    s, want = gc.case(name)
    g = gc.GRIDS[name]
    got = grid.WindGrid(s.copy(), grid.GridSpec(g[:3], g[3:]))
    for field in gref.NAMES:
        assert gref.same_bits(got[field], want[field]), field
    assert got.spec.periodic == (name == "periodic")
    np.testing.assert_array_equal(got.longitude, g[0] + (np.arange(g[2]) + 0.5) * g[1])
    np.testing.assert_array_equal(got.latitude, g[3] + (np.arange(g[5]) + 0.5) * g[4])
    ok = s[0] > 0
    off = (got.direction[ok] - (270.0 - np.degrees(np.arctan2(want["v"][ok], want["u"][ok]))) + 180.0) % 360.0 - 180.0
    assert np.isnan(got.direction[~ok]).all() and np.abs(off).max() < 1e-9


def test_a_constant_wind_comes_back_within_half_a_unit():
    """model (u, v) -> the a-priori raster of ancillary_model_ref -> grid_ref on the same tie points: u, v undo the rotation."""
    sc = round_trip_scene()
    line, sample = np.arange(float(sc["L"])), np.arange(float(sc["S"]))
    raster = aref.ancillary_from_model(sc["u"], sc["v"], sc["mlon"], sc["mlat"], sc["tl"], sc["ts"], sc["glon"], sc["glat"], sc["heading"], line, sample)
    s = gref.sums(raster, sc["tl"], sc["ts"], sc["glon"], sc["glat"], sc["heading"], (11.0, 0.5, 12, 3.0, -0.5, 10))
    f = gref.finish(s)
    ok = s[0] > 0
    assert s[0].sum() == sc["L"] * sc["S"] and ok.sum() > 40
    dev = max(float(np.abs(f["u"][ok] - sc["u0"]).max()), float(np.abs(f["v"][ok] - sc["v0"]).max()))
    print(f"largest |u - model u|, |v - model v| = {dev:.3g} (bound {2.0 ** -25:.3g})")
    assert dev <= 2.0 ** -25


def test_merge_adds_sums_and_refuses_another_grid():
    s, _ = gc.case("coarse")
    g = gc.GRIDS["coarse"]
    a, b = (grid.WindGrid(s.copy(), grid.GridSpec(g[:3], g[3:])) for _ in range(2))
    before = a.u.copy()
    a += b
    assert np.array_equal(a.sums, 2 * s) and gref.same_bits(a.u, gref.finish(2 * s)["u"]) and a.merge(b) is a and np.array_equal(a.sums, 3 * s)
    assert gref.same_bits(before, b.u)
    other = grid.WindGrid(np.zeros((5, 6, 9), np.int64), grid.GridSpec((179.0, 0.25, 9), g[3:]))
    with pytest.raises(ValueError, match="different grids"):
        a.merge(other)
    with pytest.raises(TypeError):
        a.merge(s)
    with pytest.raises(ValueError, match="int64"):
        grid.WindGrid(s.astype(np.int32), grid.GridSpec(g[:3], g[3:]))


# ---------------------------------------------------------------------------------------------- the public calls' host checks
@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the checks must have refused the call before."""
    def touched(*a, **k):
        raise AssertionError("a device call was reached before the host checks refused the arguments")
    monkeypatch.setattr(grid, "_Call", touched)
    monkeypatch.setattr(_lib, "default_context", touched)
    monkeypatch.delenv("XSW_GRID_PATH", raising=False)


def tie_points():
    tl, ts = np.array([0.0, 7.0, 22.0]), np.array([0.0, 4.0, 19.0, 30.0])
    return TiePoints(tl, ts, 10.0 + 0.1 * ts[None, :] + 0 * tl[:, None], 3.0 - 0.1 * tl[:, None] + 0 * ts[None, :], np.full((3, 4), 12.0))


LON, LAT = (10.0, 0.5, 8), (3.0, -0.5, 6)


def calls():
    """The three public forms on a 23 x 31 raster, as functions of the keyword arguments."""
    w = np.ones((23, 31), np.complex128)
    codes = CopolCodes(w.real, np.zeros((23, 31), np.uint32), None)
    return (lambda tp=None, **k: grid.wind_grid(w, tp or tie_points(), **{"lon": LON, "lat": LAT, **k}),
            lambda tp=None, **k: grid.wind_grid(w.astype(np.complex64), tp or tie_points(), **{"lon": LON, "lat": LAT, **k}),
            lambda tp=None, **k: codes.grid(tp or tie_points(), **{"lon": LON, "lat": LAT, **k}))


def test_rank_dtype_and_keep_are_checked(no_device):
    w = np.ones((23, 31), np.complex128)
    for bad in (w[0], w[None]):
        with pytest.raises(ValueError, match="2-D"):
            grid.wind_grid(bad, tie_points(), lon=LON, lat=LAT)
    for bad in (w.real, np.ones((23, 31), np.int32)):
        with pytest.raises(TypeError, match="complex128 or complex64"):
            grid.wind_grid(bad, tie_points(), lon=LON, lat=LAT)
    with pytest.raises(TypeError, match="uint32 or int32"):
        CopolCodes(w.real, np.zeros((23, 31), np.int64), None).grid(tie_points(), lon=LON, lat=LAT)
    with pytest.raises(ValueError, match="2-D"):
        CopolCodes(w.real[0], np.zeros(31, np.uint32), None).grid(tie_points(), lon=LON, lat=LAT)
    for call in calls():
        with pytest.raises(ValueError, match="shape"):
            call(keep=np.ones((23, 30), bool))
        for bad in (np.ones((23, 31)), np.ones((23, 31), np.int32)):
            with pytest.raises(TypeError, match="bool or uint8"):
                call(keep=bad)


def test_tie_points_and_coordinates_are_checked(no_device):
    tp = tie_points()
    for call in calls():
        with pytest.raises(TypeError, match="TiePoints"):
            call(tp=(tp.line, tp.sample))
        for key, bad in (("line", np.arange(23.0) + 1.0), ("sample", np.arange(31.0) - 2.0)):
            with pytest.raises(ValueError, match="extrapolated"):
                call(**{key: bad})
        for key, bad in (("line", np.arange(22.0)), ("sample", np.arange(32.0)), ("line", np.arange(23.0)[None])):
            with pytest.raises(ValueError, match="do not match"):
                call(**{key: bad})
        with pytest.raises(ValueError, match="NaN"):
            call(line=np.where(np.arange(23) == 4, np.nan, np.arange(23.0)))
    with pytest.raises(ValueError, match="extrapolated"):   # every PIXEL must lie inside the tie span, not the centres of some cells
        grid.wind_grid(np.ones((25, 31), np.complex128), tp, lon=LON, lat=LAT)
    with pytest.raises(TypeError):                           # tie points are required
        grid.wind_grid(np.ones((23, 31), np.complex128), None, lon=LON, lat=LAT)


def test_grid_entries_are_checked(no_device):
    for call in calls():
        for bad in ((10.0, 0.0, 8), (10.0, -0.5, 8), (np.nan, 0.5, 8), (10.0, np.inf, 8), (10.0, 0.5, 0), (10.0, 0.5, -3), (10.0, 0.5), (10.0, 0.5, 8, 1), 5,
                    (10.0, 0.5, 2 ** 31)):
            with pytest.raises(ValueError):
                call(lon=bad)
        for bad in ((3.0, 0.0, 6), (3.0, np.nan, 6), (np.inf, 0.5, 6), (3.0, 0.5, 0), (3.0, 0.5)):
            with pytest.raises(ValueError):
                call(lat=bad)
        for bad in ((10.0, 0.5, 8.0), (10.0, 0.5, "a"), ("a", 0.5, 8)):
            with pytest.raises(TypeError):
                call(lon=bad)
        with pytest.raises(ValueError, match="int32"):
            call(lon=(10.0, 0.001, 70000), lat=(3.0, 0.001, 70000))
    assert grid.GridSpec((-180.0, 0.5, 720), LAT).periodic and not grid.GridSpec((-180.0, 0.5, 719), LAT).periodic
    assert grid.GridSpec((0.0, 360.0 / 1441, 1441), LAT).periodic and grid.GridSpec(LON, (3.0, -0.5, 6)).shape == (6, 8)


def test_path_switch_and_into_are_checked(no_device, monkeypatch):
    other = grid.WindGrid(np.zeros((5, 6, 9), np.int64), grid.GridSpec((10.0, 0.5, 9), LAT))
    shifted = grid.WindGrid(np.zeros((5, 6, 8), np.int64), grid.GridSpec((10.0, 0.5, 8), (3.0, 0.5, 6)))
    for call in calls():
        for bad in (other, shifted):
            with pytest.raises(ValueError, match="into lies on"):
                call(into=bad)
        with pytest.raises(TypeError, match="WindGrid"):
            call(into=np.zeros((5, 6, 8), np.int64))
    for bad in ("lanes", "", "LDS", "direct "):
        monkeypatch.setenv("XSW_GRID_PATH", bad)
        for call in calls():
            with pytest.raises(ValueError, match="XSW_GRID_PATH"):
                call()


def test_good_arguments_reach_the_device(monkeypatch):
    reached = []

    def device(*arrays):
        reached.append(arrays)
        raise RuntimeError("the device")
    monkeypatch.setattr(grid, "_Call", device)
    for path in ("direct", "lds", None):
        if path is None:
            monkeypatch.delenv("XSW_GRID_PATH", raising=False)
        else:
            monkeypatch.setenv("XSW_GRID_PATH", path)
        for call in calls():
            with pytest.raises(RuntimeError, match="the device"):
                call(keep=np.ones((23, 31), bool), into=grid.WindGrid(np.zeros((5, 6, 8), np.int64), grid.GridSpec(LON, LAT)))
    assert len(reached) == 9


# --------------------------------------------------------------------------------------------------------------- declarations
def test_public_names():
    import xsarsea_amd
    assert xsarsea_amd.wind_grid is grid.wind_grid and xsarsea_amd.WindGrid is grid.WindGrid and xsarsea_amd.grid is grid
    assert {"grid", "wind_grid", "WindGrid"} <= set(xsarsea_amd.__all__) and {"WindGrid", "wind_grid", "codes_grid"} <= set(grid.__all__)
    assert callable(CopolCodes.grid) and callable(grid.WindGrid.merge) and grid.WindGrid.__iadd__ is grid.WindGrid.merge
    from xsarsea_amd import _raster
    assert _raster._TORCH_DTYPE[np.int64] == "int64"


def test_header_declares_the_entry_and_the_binding_has_one_letter_per_argument():
    entry = "xsw_wind_grid"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"include/xsw.h does not declare {entry}"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[0].startswith("xsw_ctx") and params[-1].startswith("int64_t *")
    sig = _lib.RASTER_ENTRIES[entry]
    assert len(sig) == len(params) - 1 == 24
    for letter, p in zip(sig, params[1:]):
        want = "p" if "*" in p else {"int64_t": "l", "int32_t": "i", "double": "d"}[p.split()[0]]
        assert letter == want, p
    assert entry in _lib.EXPORTS and hasattr(_lib.Context, "wind_grid_raw")
    assert hasattr(_lib.load(), entry)
    assert int(re.search(r"#\s*define\s+XSW_VERSION\s+(\d+)", txt).group(1)) == 4 == _lib.ABI_VERSION
