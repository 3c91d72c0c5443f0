"""CPU: the restatement of xsarsea_amd.polar (tests/polar_ref.py) against a per-pixel loop with atan2 sectors, what its chart
costs against the sphere, a modified Rankine vortex through the storm-centred helpers, the merge, the finish -- and the public
calls' host checks, which all precede the first device call."""
import math
import os
import re

import numpy as np
import pytest

import polar_cases as pc
import polar_ref as pref
from conftest import REPO
from xsarsea_amd import TiePoints, _lib, polar
from xsarsea_amd.windspeed.crosspol import CopolCodes


def container(sums, kw):
    return polar.WindPolar(np.array(sums), polar.PolarSpec(kw["centre"], kw["radius"], kw["sectors"]))


# --------------------------------------------------------------------------------------------------- an independent brute force
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_restatement_equals_a_per_pixel_loop_with_atan2_sectors(name):
    """Scalar Python arithmetic per pixel, the sector from math.atan2, Python integers as sums.  A pixel nearer than 1e-9 rad to a
    sector border is left to the sign rules and the table (and taken from the restatement): none outside `axes`."""
    kw = pc.spec(name)
    want, _ = pc.case(name)
    lon, lat, ch, sh = pc.geolocation(name)
    w, keep = pc.scene()
    ok, u, v, sp, q = pref.gref.pixel_terms(w, keep, ch, sh)
    (lon_c, lat_c), (dr, n_r), n_theta = kw["centre"], kw["radius"], kw["sectors"]
    lon_c = lon_c - 360.0 * round(lon_c / 360.0)
    c, s = math.cos(math.radians(lat_c)), math.sin(math.radians(lat_c))
    assert (c, s) == pref.tables(lat_c, n_theta)[:2]
    width = 2.0 * math.pi / n_theta
    got = np.zeros(want.shape, object)
    got[...] = 0
    excluded, p = 0, pc.pixels(name)
    for i, j in zip(*np.nonzero(ok)):
        dl = float(lon[i, j]) - lon_c
        dl = dl - 360.0 * round(dl / 360.0)
        dy = (float(lat[i, j]) - lat_c) * pref.D2R
        h = 0.5 * dy
        x, y = (pref.KX * dl) * ((c - s * h) - (0.5 * c) * (h * h)), pref.R_KM * dy
        r = math.sqrt(x * x + y * y)
        kr = math.floor(r / dr)
        if not kr < n_r:
            continue
        theta = math.atan2(x, y) % (2.0 * math.pi)
        near = abs(theta / width - round(theta / width)) * width
        if near < 1e-9:
            excluded += 1
            sector = int(p["sector"][i, j])
        else:
            sector = int(theta // width)
        uu, vv = float(u[i, j]), float(v[i, j])
        vr, vt = (0.0, 0.0) if r == 0.0 else ((uu * x + vv * y) / r, (vv * x - uu * y) / r)
        s24 = round(float(sp[i, j]) * 2.0 ** 24)
        for plane, a in enumerate((1, s24, round(float(q[i, j]) * 2.0 ** 16), round(vr * 2.0 ** 24), round(vt * 2.0 ** 24))):
            got[plane, kr, sector] += a
        got[5, kr, sector] = max(got[5, kr, sector], s24)
    assert np.array_equal(got.astype(np.int64), want)
    if name == "axes":
        i, j = pc.AXES_PIXEL
        assert excluded == int(p["ok"][i].sum() + p["ok"][:, j].sum()) - 1 > 40    # the centre's row and column, the centre once
    else:
        assert excluded == 0


# ------------------------------------------------------------------------------------------------------ the chart against the sphere
def sphere(lon_c, lat_c, bearing, dist_km):
    """(lon, lat) in degrees of the points at `dist_km` along the great circles leaving the centre at `bearing` (radians)."""
    d, p1 = dist_km / pref.R_KM, math.radians(lat_c)
    p2 = np.arcsin(np.sin(p1) * np.cos(d) + np.cos(p1) * np.sin(d) * np.cos(bearing))
    dlam = np.arctan2(np.sin(bearing) * np.sin(d) * np.cos(p1), np.cos(d) - np.sin(p1) * np.sin(p2))
    return lon_c + np.degrees(dlam), np.degrees(p2)


def haversine_and_bearing(lon_c, lat_c, lon, lat):
    p1, p2, dlam = math.radians(lat_c), np.radians(lat), np.radians(lon - lon_c)
    a = np.sin((p2 - p1) / 2.0) ** 2 + math.cos(p1) * np.cos(p2) * np.sin(dlam / 2.0) ** 2
    dist = 2.0 * pref.R_KM * np.arcsin(np.sqrt(a))
    return dist, np.arctan2(np.sin(dlam) * np.cos(p2), math.cos(p1) * np.sin(p2) - math.sin(p1) * np.cos(p2) * np.cos(dlam))


CHART = {}


@pytest.mark.parametrize("lat_c", [5.0, -15.0, 25.0, -35.0, 35.0])
def test_chart_error_against_haversine_distance_and_initial_bearing(lat_c):
    """Random points out to 300 km.  The issue's own measurement: 7.4e-5 relative in distance and 0.95 degrees of bearing at 35
    degrees, 4.5e-5 and 0.63 at 25.  Asserted: 2e-4 and 1.5 degrees."""
    rng = np.random.default_rng(int(abs(lat_c)))
    lon_c = 130.0
    lon, lat = sphere(lon_c, lat_c, rng.uniform(0.0, 2.0 * np.pi, 20000), rng.uniform(1.0, 300.0, 20000))
    dist, bearing = haversine_and_bearing(lon_c, lat_c, lon, lat)
    x, y = pref.chart(lon, lat, lon_c, lat_c, *pref.tables(lat_c, 4)[:2])
    rel = np.abs(np.sqrt(x * x + y * y) - dist) / dist
    off = np.degrees(np.abs((np.arctan2(x, y) - bearing + np.pi) % (2.0 * np.pi) - np.pi))
    CHART[lat_c] = (float(rel.max()), float(off.max()))
    print(f"lat_c = {lat_c}: largest relative distance error {rel.max():.3g}, largest bearing error {off.max():.3g} degrees")
    assert rel.max() <= 2e-4 and off.max() <= 1.5


# ------------------------------------------------------------------------------------------------- a modified Rankine vortex
VM, RM, DR, N_R = 50.0, 30.0, 5.0, 58
CENTRE = (130.0, 20.0)


def rankine(half):
    """A counter-clockwise vortex of Vm = 50 m/s at Rm = 30 km, V ~ r**-0.5 outside, on 2 * half x 2 * half pixels of 2 km laid out
    in the chart's own coordinates (a tie point per pixel, heading 0): (wind, tie arguments)."""
    n = 2 * half
    k = np.arange(n) - (half - 0.5)
    x, y = np.meshgrid(2.0 * k, -2.0 * k)                    # east, north in km; line 0 is the northernmost
    lon_c, lat_c = CENTRE
    cos_c, sin_c = pref.tables(lat_c, 4)[:2]
    dy = y / pref.R_KM
    h = 0.5 * dy
    lat = lat_c + dy / pref.D2R
    lon = lon_c + x / (pref.KX * ((cos_c - sin_c * h) - (0.5 * cos_c) * (h * h)))
    r = np.hypot(x, y)
    speed = np.where(r < RM, VM * r / RM, VM * np.sqrt(RM / r))
    u, v = -speed * y / r, speed * x / r
    return -u - 1j * v, (np.arange(float(n)), np.arange(float(n)), lon, lat, np.zeros((n, n)))


def test_rankine_vortex_profile_rmax_and_wind_radii():
    kw = dict(centre=CENTRE, radius=(DR, N_R), sectors=8)
    w, ties = rankine(150)
    assert w.shape == (300, 300)
    p = container(pref.sums(w, *ties, **kw), kw)
    prof = p.ring_profile()
    assert (prof["coverage"] == 1.0).all() and prof["count"].sum() > 60000
    pixel_max, ring_max, rmax = p.vmax_rmax()
    assert abs(rmax - RM) <= DR and ring_max <= pixel_max <= VM and pixel_max > 0.97 * VM and ring_max > 0.9 * VM
    radii = p.wind_radii()
    assert radii.shape == (3, 4)
    for row, T in zip(radii, (17.4911, 25.7222, 32.9244)):
        want = RM * (VM / T) ** 2
        print(f"T = {T}: {want:.2f} km expected, quadrants {np.round(row, 2)}")
        assert want < N_R * DR - DR and (np.abs(row - want) <= DR).all()
    beyond = prof["radius"] > RM + DR
    assert np.abs(prof["vt"][beyond] - prof["wspd"][beyond]).max() <= 2.0 ** -20 and np.abs(prof["vr"]).max() < 2.0 ** -20
    assert np.abs(p.inflow_angle[p.count > 0]).max() < 1e-4
    assert np.array_equal(p.radius, (np.arange(N_R) + 0.5) * DR) and np.array_equal(p.bearing, (np.arange(8) + 0.5) * 45.0)
    # the first ring wins a tie
    tied = np.array(p.sums)
    tied[1:, 9] = tied[1:, 6]
    tied[0, 9] = tied[0, 6]
    flat = container(tied, kw).ring_profile()["wspd"]
    assert flat[9] == flat[6] == flat.max() and container(tied, kw).vmax_rmax()[2] == (6 + 0.5) * DR


def test_wind_radii_are_nan_where_the_raster_ends_inside_the_radius():
    """300 km x 300 km: the corners lie at 212 km, inside the 34 kt radius of 245 km."""
    kw = dict(centre=CENTRE, radius=(DR, N_R), sectors=8)
    w, ties = rankine(75)
    p = container(pref.sums(w, *ties, **kw), kw)
    radii = p.wind_radii()
    assert np.isnan(radii[0]).all() and (np.abs(radii[1] - RM * (VM / 25.7222) ** 2) <= DR).all() and (np.abs(radii[2] - RM * (VM / 32.9244) ** 2) <= DR).all()
    assert np.isnan(p.wind_radii(thresholds=(60.0,))).all()                       # no ring reaches it
    assert np.isnan(p.wind_radii(min_count=10 ** 6)).all()                        # no ring has that many pixels
    prof = p.ring_profile()
    assert np.isnan(prof["wspd"][prof["coverage"] < 0.5]).all() and (prof["coverage"] < 0.5).any() and not np.isnan(prof["wspd"][:20]).any()
    assert not np.isnan(p.ring_profile(min_coverage=0.0)["wspd"][prof["count"] > 0]).any()
    empty = container(np.zeros((6, N_R, 8), np.int64), kw)
    assert all(np.isnan(v) for v in empty.vmax_rmax()) and np.isnan(empty.wind_radii()).all()


# ----------------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("name", ["quadrants", "antimeridian", "axes"])
def test_merge_of_row_halves_equals_the_whole(name):
    w, keep = pc.scene()
    kw = pc.spec(name)
    whole, fields = pc.case(name)
    top = pref.sums(w[:48], *pc.ties(name), **kw, line=np.arange(48), keep=keep[:48])
    bottom = pref.sums(w[48:], *pc.ties(name), **kw, line=np.arange(48, pc.L), keep=keep[48:])
    assert top[5].max() != bottom[5].max() and np.array_equal(pref.merge(top, bottom), whole) and np.array_equal(pref.merge(bottom, top), whole)
    for a, b in ((top, bottom), (bottom, top)):
        got = container(a, kw)
        assert got.merge(container(b, kw)) is got and np.array_equal(got.sums, whole)
        for field in pref.NAMES:
            assert pref.same_bits(got[field], fields[field]), field
    got = container(top, kw)
    before = got.wspd.copy()
    got += container(bottom, kw)
    assert np.array_equal(got.sums, whole) and not pref.same_bits(before, got.wspd)
    into = pref.sums(w[48:], *pc.ties(name), **kw, line=np.arange(48, pc.L), keep=keep[48:], into=top.copy())
    assert np.array_equal(into, whole)
    other = polar.WindPolar(np.zeros((6, kw["radius"][1], kw["sectors"] + 4), np.int64), polar.PolarSpec(kw["centre"], kw["radius"], kw["sectors"] + 4))
    with pytest.raises(ValueError, match="different bins"):
        got.merge(other)
    with pytest.raises(TypeError):
        got.merge(whole)
    with pytest.raises(ValueError, match="int64"):
        polar.WindPolar(whole.astype(np.int32), polar.PolarSpec(kw["centre"], kw["radius"], kw["sectors"]))


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_the_package_finishes_as_the_restatement_does(name):
    s, want = pc.case(name)
    got = container(s, pc.spec(name))
    for field in pref.NAMES:
        assert pref.same_bits(got[field], want[field]), field
    ok = s[0] > 0
    assert np.isnan(got.vmax[~ok]).all() and (got.vmax[ok] >= got.wspd[ok]).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(got.inflow_angle[~ok]).all() and np.abs(got.inflow_angle[ok] - np.degrees(np.arctan2(-want["vr"][ok], want["vt"][ok]))).max() < 1e-9
    ring = got.ring_profile(min_coverage=0.0)
    assert np.array_equal(ring["count"], s[0].sum(axis=1)) and pref.same_bits(ring["wspd"], pref.finish(np.concatenate([s[:5].sum(axis=2), s[5:].max(axis=2)]))["wspd"])


def test_the_package_builds_the_tables_of_the_restatement():
    for lat_c, n_theta in ((10.08, 4), (-35.0, 360), (20.0 - 40.0 / 128.0, 16), (89.0, 72)):
        got, want = polar.PolarSpec((10.0, lat_c), (1.0, 3), n_theta).tables(), pref.tables(lat_c, n_theta)
        assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and len(got[2]) == n_theta // 4 + 1
    assert polar.PolarSpec((180.4, 10.1), (4.0, 12), 72) == polar.PolarSpec((-179.6, 10.1), (4.0, 12), 72) != polar.PolarSpec((-179.6, 10.1), (4.0, 12), 76)
    assert polar.PolarSpec((180.4, 10.1), (4.0, 12), 72).lon_c == pref.wrap_centre(180.4) == -179.6


# ---------------------------------------------------------------------------------------------- the public calls' host checks
@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the checks must have refused the call before."""
    def touched(*a, **k):
        raise AssertionError("a device call was reached before the host checks refused the arguments")
    monkeypatch.setattr(polar, "_Call", touched)
    monkeypatch.setattr(_lib, "default_context", touched)
    monkeypatch.delenv("XSW_GRID_PATH", raising=False)


def tie_points():
    tl, ts = np.array([0.0, 7.0, 22.0]), np.array([0.0, 4.0, 19.0, 30.0])
    return TiePoints(tl, ts, 10.0 + 0.1 * ts[None, :] + 0 * tl[:, None], 3.0 - 0.1 * tl[:, None] + 0 * ts[None, :], np.full((3, 4), 12.0))


GOOD = dict(centre=(11.0, 2.0), radius=(10.0, 8), sectors=8)


def calls():
    """The three public forms on a 23 x 31 raster, as functions of the keyword arguments."""
    w = np.ones((23, 31), np.complex128)
    codes = CopolCodes(w.real, np.zeros((23, 31), np.uint32), None)
    return (lambda tp=None, **k: polar.wind_polar(w, tp or tie_points(), **{**GOOD, **k}),
            lambda tp=None, **k: polar.wind_polar(w.astype(np.complex64), tp or tie_points(), **{**GOOD, **k}),
            lambda tp=None, **k: codes.polar(tp or tie_points(), **{**GOOD, **k}))


def test_centre_radius_and_sectors_are_checked(no_device):
    for call in calls():
        for bad in ((np.nan, 2.0), (11.0, np.inf), (11.0, 89.5), (11.0, -90.0), (11.0,), (11.0, 2.0, 3.0), 11.0, None):
            with pytest.raises(ValueError):
                call(centre=bad)
        with pytest.raises(TypeError):
            call(centre=("a", 2.0))
        for bad in ((0.0, 8), (-10.0, 8), (np.nan, 8), (np.inf, 8), (10.0, 0), (10.0, -2), (10.0,), 10.0):
            with pytest.raises(ValueError):
                call(radius=bad)
        for bad in ((10.0, 8.0), ("a", 8)):
            with pytest.raises(TypeError):
                call(radius=bad)
        for bad in (0, 2, 6, 9, 362, -4, 364):
            with pytest.raises(ValueError, match="multiple of 4"):
                call(sectors=bad)
        with pytest.raises(TypeError):
            call(sectors=8.0)
        with pytest.raises(ValueError, match="int32"):
            call(radius=(0.001, 2 ** 24), sectors=360)
    assert polar.PolarSpec((11.0, 89.0), (10.0, 8), 360).shape == (8, 360)


def test_rank_dtype_keep_tie_points_and_coordinates_are_checked(no_device):
    w = np.ones((23, 31), np.complex128)
    for bad in (w[0], w[None]):
        with pytest.raises(ValueError, match="2-D"):
            polar.wind_polar(bad, tie_points(), **GOOD)
    for bad in (w.real, np.ones((23, 31), np.int32)):
        with pytest.raises(TypeError, match="complex128 or complex64"):
            polar.wind_polar(bad, tie_points(), **GOOD)
    with pytest.raises(TypeError, match="uint32 or int32"):
        CopolCodes(w.real, np.zeros((23, 31), np.int64), None).polar(tie_points(), **GOOD)
    tp = tie_points()
    for call in calls():
        with pytest.raises(ValueError, match="shape"):
            call(keep=np.ones((23, 30), bool))
        with pytest.raises(TypeError, match="bool or uint8"):
            call(keep=np.ones((23, 31)))
        with pytest.raises(TypeError, match="TiePoints"):
            call(tp=(tp.line, tp.sample))
        for key, bad in (("line", np.arange(23.0) + 1.0), ("sample", np.arange(31.0) - 2.0)):
            with pytest.raises(ValueError, match="extrapolated"):
                call(**{key: bad})
        with pytest.raises(ValueError, match="do not match"):
            call(line=np.arange(22.0))


def test_path_switch_and_into_are_checked(no_device, monkeypatch):
    other = polar.WindPolar(np.zeros((6, 8, 12), np.int64), polar.PolarSpec(GOOD["centre"], GOOD["radius"], 12))
    moved = polar.WindPolar(np.zeros((6, 8, 8), np.int64), polar.PolarSpec((11.0, 2.5), GOOD["radius"], 8))
    wider = polar.WindPolar(np.zeros((6, 8, 8), np.int64), polar.PolarSpec(GOOD["centre"], (12.0, 8), 8))
    for call in calls():
        for bad in (other, moved, wider):
            with pytest.raises(ValueError, match="into lies on"):
                call(into=bad)
        with pytest.raises(TypeError, match="WindPolar"):
            call(into=np.zeros((6, 8, 8), np.int64))
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
    monkeypatch.setattr(polar, "_Call", device)
    for path in ("direct", "lds", None):
        if path is None:
            monkeypatch.delenv("XSW_GRID_PATH", raising=False)
        else:
            monkeypatch.setenv("XSW_GRID_PATH", path)
        for call in calls():
            with pytest.raises(RuntimeError, match="the device"):
                call(keep=np.ones((23, 31), bool), into=polar.WindPolar(np.zeros((6, 8, 8), np.int64), polar.PolarSpec(**GOOD)))
    assert len(reached) == 9


# --------------------------------------------------------------------------------------------------------------- declarations
def test_public_names():
    import xsarsea_amd
    assert xsarsea_amd.wind_polar is polar.wind_polar and xsarsea_amd.WindPolar is polar.WindPolar and xsarsea_amd.polar is polar
    assert {"polar", "wind_polar", "WindPolar"} <= set(xsarsea_amd.__all__) and {"WindPolar", "wind_polar", "codes_polar"} <= set(polar.__all__)
    assert callable(CopolCodes.polar) and callable(polar.WindPolar.merge) and polar.WindPolar.__iadd__ is polar.WindPolar.merge
    for helper in (polar.WindPolar.ring_profile, polar.WindPolar.vmax_rmax, polar.WindPolar.wind_radii):
        assert "only synchronisation" in helper.__doc__


def test_header_declares_the_entry_and_the_binding_has_one_letter_per_argument():
    entry = "xsw_wind_polar"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"include/xsw.h does not declare {entry}"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[0].startswith("xsw_ctx") and params[-1].startswith("int64_t *")
    sig = _lib.RASTER_ENTRIES[entry]
    assert len(sig) == len(params) - 1 == 26
    for letter, p in zip(sig, params[1:]):
        want = "p" if "*" in p else {"int64_t": "l", "int32_t": "i", "double": "d"}[p.split()[0]]
        assert letter == want, p
    assert entry in _lib.EXPORTS and hasattr(_lib.Context, "wind_polar_raw")
    assert hasattr(_lib.load(), entry)
    assert int(re.search(r"#\s*define\s+XSW_VERSION\s+(\d+)", txt).group(1)) == 4 == _lib.ABI_VERSION
    src = open(os.path.join(REPO, "xsarsea_amd", "csrc", "xsw_cells.hip")).read()
    assert int(re.search(r"#\s*define\s+XSW_POLAR_MAX_SECTORS\s+(\d+)", src).group(1)) == polar.MAX_SECTORS
