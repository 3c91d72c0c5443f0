"""CPU: the restatement of xsarsea_amd.centre (tests/centre_ref.py) against tests/polar_ref.py for one candidate and against a
per-pixel, per-candidate loop with Python integers; the inverse chart; a modified Rankine vortex recovered through
`CentreScores.best` and `find_centre` in both hemispheres; the merge, the finish, ties and coverage -- and the public calls' host
checks, which all precede the first device call."""
import os
import re

import numpy as np
import pytest

import centre_cases as cc
import centre_ref as cref
import polar_cases as pc
import polar_ref as pref
from conftest import REPO
from xsarsea_amd import TiePoints, _lib, centre
from xsarsea_amd.windspeed.crosspol import CopolCodes


def container(sums, kw):
    return centre.CentreScores(np.array(sums), centre.CentreSpec(kw["first_guess"], kw["step_km"], kw["n"], kw["annulus"]))


# ------------------------------------------------------------------------------------------- one candidate is one ring of wind_polar
@pytest.mark.parametrize("R", [7.5, 20.0, 90.0])
@pytest.mark.parametrize("grid", ["quadrants", "offscene", "antimeridian", "axes"])
def test_one_candidate_equals_planes_0_to_4_of_polar_added_over_sectors(grid, R):
    w, keep = pc.scene()
    guess = pc.spec(grid)["centre"]
    got = cref.sums(w, *pc.ties(grid), first_guess=guess, step_km=1.0, n=1, annulus=(0.0, R), keep=keep)
    want = pref.sums(w, *pc.ties(grid), centre=guess, radius=(R, 1), sectors=8, keep=keep)
    assert got.shape == (5, 1, 1) and np.array_equal(got[:, 0, 0], want[:5, 0, :].sum(axis=1))
    assert (want[0].sum() > 100) if (grid, R) != ("offscene", 7.5) and (grid, R) != ("offscene", 20.0) else want[0].sum() == 0   # (the scene begins 22 km from that centre)
    if grid == "antimeridian":
        twin = cref.sums(w, *pc.ties(grid), first_guess=pc.ANTIMERIDIAN_TWIN["centre"], step_km=1.0, n=1, annulus=(0.0, R), keep=keep)
        assert np.array_equal(twin, got)
    # with one candidate step_km is not read
    assert np.array_equal(cref.sums(w, *pc.ties(grid), first_guess=guess, step_km=float("nan"), n=1, annulus=(0.0, R), keep=keep), got)


def test_the_shared_cases_hold_their_properties():
    for name in cc.CASES:
        s, fields = cc.case(name)
        assert s.shape[1:] == (cc.spec(name)["n"],) * 2 and set(fields) == set(cref.NAMES)
    assert np.array_equal(cc.case("one_antimeridian")[0], cc.case("one_antimeridian_twin")[0])
    assert not np.array_equal(cc.case("small", np.complex64)[0], cc.case("small")[0])


# --------------------------------------------------------------------------------------------------- an independent brute force
@pytest.mark.parametrize("name", ["small", "ring", "offscene", "one_axes"])
def test_restatement_equals_a_per_pixel_per_candidate_loop(name):
    """Scalar Python arithmetic per pixel and candidate and Python integers as sums, on every 35th pixel."""
    import math
    kw = cc.spec(name)
    w, keep = pc.scene()
    pick = np.zeros(w.shape, bool)
    pick.reshape(-1)[::35] = True
    if name in ("ring", "one_axes"):
        pick[pc.AXES_PIXEL] = True     # r == 0 at the middle candidate
    sub = keep & pick
    want = cref.sums(w, *cc.ties(name), **kw, keep=sub)
    p = cc.pixels(name)
    n, step = kw["n"], kw["step_km"]
    h = (n - 1) // 2
    r_in, r_out = kw["annulus"]
    got = [[[0] * n for _ in range(n)] for _ in range(5)]
    hits = centre_hits = 0
    for a, b in zip(*np.nonzero(p["ok"] & sub)):
        x, y, u, v = (float(p[k][a, b]) for k in ("x", "y", "u", "v"))
        s24, q16 = round(float(p["sp"][a, b]) * 2.0 ** 24), round(float(p["q"][a, b]) * 2.0 ** 16)
        for i in range(n):
            for j in range(n):
                dx, dy = x - float(j - h) * step, y - float(i - h) * step
                r = math.sqrt(dx * dx + dy * dy)
                if not (r_in <= r and r < r_out):
                    continue
                vr, vt = (0.0, 0.0) if r == 0.0 else ((u * dx + v * dy) / r, (v * dx - u * dy) / r)
                hits += 1
                centre_hits += r == 0.0
                for plane, term in enumerate((1, s24, q16, round(vr * 2.0 ** 24), round(vt * 2.0 ** 24))):
                    got[plane][i][j] += term
    assert hits == want[0].sum() > 30 and np.array_equal(np.array(got, dtype=np.int64), want)
    assert centre_hits == (1 if name == "one_axes" else 0)   # (the ring's r_in leaves the pixel at r == 0 out)


# ----------------------------------------------------------------------------------------------------------- the inverse chart
@pytest.mark.parametrize("guess, step, n", [((130.0, 20.0), 1.0, 17), ((-179.99, -35.0), 8.0, 31), ((179.98, 60.0), 4.0, 31), ((10.0, 89.0), 0.5, 9),
                                            ((0.0, 0.0), 2.0, 1)])
def test_chart_of_every_candidate_returns_its_offsets(guess, step, n):
    lon, lat = cref.inverse_chart(guess, step, n)
    assert lon.shape == lat.shape == (n, n) and (lon >= -180.0).all() and (lon < 180.0).all()
    x, y = pref.chart(lon, lat, pref.wrap_centre(guess[0]), guess[1], *pref.tables(guess[1], 4)[:2])
    off = cref.lattice(n, step)
    assert np.abs(x - off[None, :]).max() <= 1e-9 and np.abs(y - off[:, None]).max() <= 1e-9
    assert n == 1 or (np.diff(lat[:, 0]) > 0).all()                     # row i runs south to north
    spec = centre.CentreSpec(guess, step, n, (0.0, 1.0))
    assert pref.same_bits(spec.longitude, lon) and pref.same_bits(spec.latitude, lat)
    assert np.array_equal(spec.x_km, off) and np.array_equal(spec.y_km, off) and spec.shape == (n, n)


# ------------------------------------------------------------------------------------------------------------ vortex recovery
def vortex_scores(offset, south, step, n, annulus):
    w, ties, guess = cc.vortex(offset, south)
    kw = dict(first_guess=guess, step_km=step, n=n, annulus=annulus)
    return container(cref.sums(w, *ties, **kw), kw)


@pytest.mark.parametrize("south", [False, True])
@pytest.mark.parametrize("offset", cc.TRUE_OFFSETS)
def test_vortex_centre_is_recovered(offset, south):
    """Vm 50 m/s at Rm 6 km, 20 degrees of inflow, 2 m/s of noise per component.  The southern vortex turns clockwise: only
    rotation = -1, which None picks there, finds it."""
    fine = vortex_scores(offset, south, 1.0, 17, (4.0, 9.0))
    fix = fine.best("vt")
    assert (fix.i, fix.j) == cc.true_node(offset, 1.0, 17) and (fix.x_km, fix.y_km) == offset and not fix.on_border and fix.score > 35.0
    assert (fine.count >= 0.9 * fine.count.max()).all() and fine.count.min() > 1000                    # all 289 are eligible
    assert (fix.i, fix.j, fix.score) == cref.best(fine.sums, fine.spec.lat_g, "vt")
    same = fine.best("vt", rotation=-1 if south else 1)
    assert (same.i, same.j, same.score) == (fix.i, fix.j, fix.score)
    other = fine.best("vt", rotation=1 if south else -1)
    assert (other.i, other.j) != (fix.i, fix.j) and other.score < 0.0
    lon, lat = cref.inverse_chart(fine.spec.key()[:2], 1.0, 17)
    assert fix.lon == lon[fix.i, fix.j] and fix.lat == lat[fix.i, fix.j]
    eye = vortex_scores(offset, south, 1.0, 17, (0.0, 3.0))
    calm = eye.best("calm")
    assert (calm.i, calm.j) == cc.true_node(offset, 1.0, 17) and (eye.count >= 0.9 * eye.count.max()).all()
    assert (calm.i, calm.j, calm.score) == cref.best(eye.sums, eye.spec.lat_g, "calm")
    coarse = vortex_scores(offset, south, 2.0, 9, (4.0, 9.0))
    fix2 = coarse.best("vt")
    assert max(abs(fix2.x_km - offset[0]), abs(fix2.y_km - offset[1])) <= 2.0 and (coarse.count >= 0.9 * coarse.count.max()).all()
    # the highest annulus-mean speed lies near the centre as well; the most uniform speed is some eligible candidate
    fast = fine.best("wspd")
    assert max(abs(fast.x_km - offset[0]), abs(fast.y_km - offset[1])) <= 2.0
    steady = fine.best("steady")
    assert (steady.i, steady.j, steady.score) == cref.best(fine.sums, fine.spec.lat_g, "steady") and steady.score == fine.wspd_std.min()


def host_route(monkeypatch):
    """The scoring calls answered by the restatement: `find_centre`'s own logic without a device."""
    def scores(wind, tie_points, *, first_guess, step_km, n, annulus, line=None, sample=None, keep=None, into=None):
        kw = dict(first_guess=first_guess, step_km=step_km, n=n, annulus=annulus)
        ties = (tie_points.line, tie_points.sample, tie_points.longitude, tie_points.latitude, tie_points.ground_heading)
        return container(cref.sums(wind, *ties, **kw, line=line, sample=sample, keep=keep), kw)
    monkeypatch.setattr(centre, "wind_centre_scores", scores)


@pytest.mark.parametrize("south", [False, True])
def test_find_centre_from_ten_kilometres_off(monkeypatch, south):
    host_route(monkeypatch)
    offset = cc.TRUE_OFFSETS[0]
    w, ties, guess = cc.vortex(offset, south)
    lon, lat = cref.inverse_chart(guess, 1.0, 31)
    start = (float(lon[15 + 4, 15 - 5]), float(lat[15 + 4, 15 - 5]))        # (-5, 4) km from the guess: 10 km from the truth
    fix = centre.find_centre(w, TiePoints(*ties), first_guess=start, steps_km=(4.0, 1.0), n=9, annulus=(4.0, 9.0))
    assert len(fix.levels) == 2 and all(level.found for level in fix.levels) and fix.found
    x, y = pref.chart(np.array([level.lon for level in fix.levels]), np.array([level.lat for level in fix.levels]), guess[0], guess[1],
                      *pref.tables(guess[1], 4)[:2])
    assert max(abs(x[0] - offset[0]), abs(y[0] - offset[1])) <= 4.0 and max(abs(x[1] - offset[0]), abs(y[1] - offset[1])) < 1e-3
    assert (fix.lon, fix.lat, fix.i, fix.j) == (fix.levels[1].lon, fix.levels[1].lat, fix.levels[1].i, fix.levels[1].j) and not fix.on_border
    # without a first guess: the middle of the tie points, here the vortex's own guess to a few metres
    auto = centre.find_centre(w, TiePoints(*ties), steps_km=(2.0, 1.0), n=9, annulus=(4.0, 9.0))
    xa, ya = pref.chart(np.array(auto.lon), np.array(auto.lat), guess[0], guess[1], *pref.tables(guess[1], 4)[:2])
    assert max(abs(float(xa) - offset[0]), abs(float(ya) - offset[1])) < 0.5
    # a level with nothing eligible: the search stops with the fix before it, or with its own NaN fix if it is the first
    none = centre.find_centre(w, TiePoints(*ties), first_guess=start, steps_km=(4.0, 1.0), n=9, annulus=(4.0, 9.0), keep=np.zeros(w.shape, bool))
    assert len(none.levels) == 1 and not none.found and np.isnan(none.lon) and (none.i, none.j) == (-1, -1)
    codes_like = centre.find_centre(w, TiePoints(*ties), first_guess=start, steps_km=(4.0,), n=9, annulus=(4.0, 9.0))
    assert (codes_like.lon, codes_like.lat) == (fix.levels[0].lon, fix.levels[0].lat)
    for bad in ((), (4.0, 0.0), (np.nan,)):
        with pytest.raises(ValueError, match="steps_km"):
            centre.find_centre(w, TiePoints(*ties), steps_km=bad, annulus=(4.0, 9.0))
    with pytest.raises(ValueError, match="criterion"):
        centre.find_centre(w, TiePoints(*ties), annulus=(4.0, 9.0), criterion="fastest")


# ----------------------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("name", ["small", "ring", "one_antimeridian"])
def test_merge_of_row_halves_equals_the_whole(name):
    w, keep = pc.scene()
    kw = cc.spec(name)
    whole, fields = cc.case(name)
    top = cref.sums(w[:48], *cc.ties(name), **kw, line=np.arange(48), keep=keep[:48])
    bottom = cref.sums(w[48:], *cc.ties(name), **kw, line=np.arange(48, pc.L), keep=keep[48:])
    assert top[0].sum() > 0 and bottom[0].sum() > 0 and np.array_equal(cref.merge(top, bottom), whole) and np.array_equal(cref.merge(bottom, top), whole)
    for a, b in ((top, bottom), (bottom, top)):
        got = container(a, kw)
        assert got.merge(container(b, kw)) is got and np.array_equal(got.sums, whole)
        for field in cref.NAMES:
            assert pref.same_bits(got[field], fields[field]), field
    got = container(top, kw)
    before = got.wspd.copy()
    got += container(bottom, kw)
    assert np.array_equal(got.sums, whole) and not pref.same_bits(before, got.wspd) and np.array_equal(got.host_sums(), whole)
    assert np.array_equal(cref.sums(w[48:], *cc.ties(name), **kw, line=np.arange(48, pc.L), keep=keep[48:], into=top.copy()), whole)
    other = container(np.zeros_like(whole), dict(kw, annulus=(kw["annulus"][0], kw["annulus"][1] + 1.0)))
    with pytest.raises(ValueError, match="different lattices"):
        got.merge(other)
    with pytest.raises(TypeError):
        got.merge(whole)
    with pytest.raises(ValueError, match="int64"):
        centre.CentreScores(whole.astype(np.int32), got.spec)
    with pytest.raises(ValueError, match="int64"):
        centre.CentreScores(whole[:, :-1] if kw["n"] > 1 else np.zeros((5, 2, 1), np.int64), got.spec)


# ------------------------------------------------------------------------------------------------------------ ties and coverage
def hand_made(n_plane, vt, wspd=None, lat=10.0):
    """Sums whose finished vt (and wspd) are the given short dyadic values: Sr = 0, St = vt * n * 2**24, Ss = wspd * n * 2**24."""
    n_plane = np.asarray(n_plane, np.int64)
    vt = np.asarray(vt, np.float64)
    wspd = np.full(vt.shape, 8.0) if wspd is None else np.asarray(wspd, np.float64)
    s = np.zeros((5,) + n_plane.shape, np.int64)
    s[0] = n_plane
    s[1] = np.rint(wspd * n_plane * 2.0 ** 24)
    s[2] = np.rint(wspd * wspd * n_plane * 2.0 ** 16)
    s[4] = np.rint(vt * n_plane * 2.0 ** 24)
    return centre.CentreScores(s, centre.CentreSpec((20.0, lat), 1.0, n_plane.shape[0], (0.0, 5.0)))


def test_ties_coverage_and_borders_on_hand_made_sums():
    n = np.full((3, 3), 100)
    vt = np.array([[1.0, 5.0, 2.0], [5.0, 5.0, 0.5], [-7.0, 5.0, 3.0]])
    tied = hand_made(n, vt)
    fix = tied.best("vt")
    assert (fix.i, fix.j, fix.score, fix.on_border) == (0, 1, 5.0, True) and (fix.x_km, fix.y_km) == (0.0, -1.0)      # the smallest flat index of four
    south = hand_made(n, vt, lat=-10.0).best("vt")
    assert (south.i, south.j, south.score, south.on_border) == (2, 0, 7.0, True)                                   # rotation -1 by the latitude
    assert hand_made(n, vt, lat=-10.0).best("vt", rotation=1).score == 5.0 and tied.best("vt", rotation=-1).score == 7.0
    assert (lambda f: (f.i, f.j))(hand_made(n, vt, lat=0.0).best("vt")) == (0, 1)                                    # the equator counts as north
    # coverage: exactly min_coverage * max is eligible, one pixel less is not
    n2 = np.array([[100, 100, 100], [100, 90, 100], [89, 100, 100]])
    vt2 = np.array([[1.0, 1.0, 1.0], [1.0, 5.0, 1.0], [9.0, 1.0, 1.0]])
    assert (lambda f: (f.i, f.j, f.on_border))(hand_made(n2, vt2).best("vt")) == (1, 1, False)
    assert (lambda f: (f.i, f.j))(hand_made(n2, vt2).best("vt", min_coverage=0.89)) == (2, 0)
    assert (lambda f: (f.i, f.j))(hand_made(n2, vt2).best("vt", min_coverage=0.0)) == (2, 0)
    n3 = n2.copy()
    n3[1, 1] = 89
    assert (lambda f: (f.i, f.j))(hand_made(n3, vt2).best("vt")) == (0, 0)
    # an empty candidate is never eligible, whatever min_coverage; nothing eligible: NaN
    n4 = np.zeros((3, 3), np.int64)
    n4[2, 2] = 1
    only = hand_made(n4, np.zeros((3, 3))).best("vt", min_coverage=0.0)
    assert (only.i, only.j) == (2, 2)
    assert (lambda f: (f.i, f.j, f.found))(hand_made(n4, np.zeros((3, 3))).best("steady")) == (-1, -1, False)         # one pixel has no scatter
    empty = hand_made(np.zeros((3, 3), np.int64), np.zeros((3, 3))).best("vt")
    assert (empty.i, empty.j, empty.on_border, empty.found) == (-1, -1, False, False)
    assert all(np.isnan(v) for v in (empty.lon, empty.lat, empty.x_km, empty.y_km, empty.score))
    # wspd maximises, calm minimises, ties to the first
    wspd = np.array([[8.0, 9.0, 4.0], [9.0, 6.0, 4.0], [5.0, 5.0, 5.0]])
    speeds = hand_made(n, np.zeros((3, 3)), wspd)
    assert (lambda f: (f.i, f.j, f.score))(speeds.best("wspd")) == (0, 1, 9.0) and (lambda f: (f.i, f.j, f.score))(speeds.best("calm")) == (0, 2, 4.0)
    for field in cref.NAMES:
        assert pref.same_bits(speeds[field], cref.finish(speeds.sums)[field])
    for kw in (dict(criterion="fast"), dict(rotation=0), dict(rotation=2), dict(min_coverage=1.5), dict(min_coverage=-0.1)):
        with pytest.raises(ValueError):
            tied.best(**kw)


@pytest.mark.parametrize("name", ["small", "ring", "offscene"])
def test_the_package_finishes_and_chooses_as_the_restatement_does(name):
    s, want = cc.case(name)
    got = container(s, cc.spec(name))
    for field in cref.NAMES:
        assert pref.same_bits(got[field], want[field]), field
    for criterion in centre.CRITERIA:
        for cover in (0.9, 0.5, 0.0):
            fix = got.best(criterion, cover)
            i, j, score = cref.best(s, got.spec.lat_g, criterion, cover)
            assert (fix.i, fix.j) == (i, j) and fix.score == score, (criterion, cover)


# ---------------------------------------------------------------------------------------------- the public calls' host checks
@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the checks must have refused the call before."""
    def touched(*a, **k):
        raise AssertionError("a device call was reached before the host checks refused the arguments")
    monkeypatch.setattr(centre, "_Call", touched)
    monkeypatch.setattr(_lib, "default_context", touched)
    monkeypatch.delenv("XSW_CENTRE_PATH", raising=False)


def tie_points():
    tl, ts = np.array([0.0, 7.0, 22.0]), np.array([0.0, 4.0, 19.0, 30.0])
    return TiePoints(tl, ts, 10.0 + 0.1 * ts[None, :] + 0 * tl[:, None], 3.0 - 0.1 * tl[:, None] + 0 * ts[None, :], np.full((3, 4), 12.0))


GOOD = dict(first_guess=(11.0, 2.0), step_km=2.0, n=9, annulus=(4.0, 9.0))


def calls():
    """The three public forms on a 23 x 31 raster, as functions of the keyword arguments."""
    w = np.ones((23, 31), np.complex128)
    codes = CopolCodes(w.real, np.zeros((23, 31), np.uint32), None)
    return (lambda tp=None, **k: centre.wind_centre_scores(w, tp or tie_points(), **{**GOOD, **k}),
            lambda tp=None, **k: centre.wind_centre_scores(w.astype(np.complex64), tp or tie_points(), **{**GOOD, **k}),
            lambda tp=None, **k: codes.centre_scores(tp or tie_points(), **{**GOOD, **k}))


def test_first_guess_lattice_and_annulus_are_checked(no_device):
    for call in calls():
        for bad in ((np.nan, 2.0), (11.0, np.inf), (11.0, 89.5), (11.0, -90.0), (11.0,), (11.0, 2.0, 3.0), 11.0, None):
            with pytest.raises(ValueError):
                call(first_guess=bad)
        with pytest.raises(TypeError):
            call(first_guess=("a", 2.0))
        for bad in (0, 2, 8, 33, -3, 32):
            with pytest.raises(ValueError, match="odd"):
                call(n=bad)
        with pytest.raises(TypeError):
            call(n=9.0)
        for bad in (0.0, -2.0, np.nan, np.inf):
            with pytest.raises(ValueError, match="step_km"):
                call(step_km=bad)
        with pytest.raises(TypeError):
            call(step_km="a")
        for bad in ((9.0, 4.0), (4.0, 4.0), (-1.0, 4.0), (np.nan, 4.0), (0.0, np.inf), (4.0,), 4.0):
            with pytest.raises(ValueError, match="annulus"):
                call(annulus=bad)
        with pytest.raises(TypeError):
            call(annulus=("a", 4.0))
    assert centre.CentreSpec((11.0, 89.0), 0.5, 31, (0.0, 1.0)).shape == (31, 31)
    assert centre.CentreSpec((11.0, 2.0), np.nan, 1, (0.0, 1.0)) == centre.CentreSpec((371.0, 2.0), -3.0, 1, (0.0, 1.0))       # one candidate: step_km is not read
    assert centre.CentreSpec((180.4, 2.0), 1.0, 3, (0.0, 1.0)) == centre.CentreSpec((-179.6, 2.0), 1.0, 3, (0.0, 1.0)) != centre.CentreSpec((-179.6, 2.0), 1.0, 5, (0.0, 1.0))
    assert centre.CentreSpec((180.4, 2.0), 1.0, 3, (0.0, 1.0)).lon_g == pref.wrap_centre(180.4) == -179.6
    assert centre.CentreSpec((11.0, -35.0), 1.0, 3, (0.0, 1.0)).tables() == pref.tables(-35.0, 4)[:2]


def test_rank_dtype_keep_tie_points_and_coordinates_are_checked(no_device):
    w = np.ones((23, 31), np.complex128)
    for bad in (w[0], w[None]):
        with pytest.raises(ValueError, match="2-D"):
            centre.wind_centre_scores(bad, tie_points(), **GOOD)
    for bad in (w.real, np.ones((23, 31), np.int32)):
        with pytest.raises(TypeError, match="complex128 or complex64"):
            centre.wind_centre_scores(bad, tie_points(), **GOOD)
    with pytest.raises(TypeError, match="uint32 or int32"):
        CopolCodes(w.real, np.zeros((23, 31), np.int64), None).centre_scores(tie_points(), **GOOD)
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
    with pytest.raises(TypeError, match="TiePoints"):
        centre.find_centre(w, (tp.line, tp.sample), annulus=(4.0, 9.0))
    with pytest.raises(TypeError, match="TiePoints"):
        CopolCodes(w.real, np.zeros((23, 31), np.uint32), None).find_centre((tp.line, tp.sample), annulus=(4.0, 9.0))


def test_path_switch_and_into_are_checked(no_device, monkeypatch):
    spec = lambda **k: centre.CentreSpec(**{**GOOD, **k})
    other = centre.CentreScores(np.zeros((5, 11, 11), np.int64), spec(n=11))
    moved = centre.CentreScores(np.zeros((5, 9, 9), np.int64), spec(first_guess=(11.0, 2.5)))
    wider = centre.CentreScores(np.zeros((5, 9, 9), np.int64), spec(annulus=(4.0, 10.0)))
    for call in calls():
        for bad in (other, moved, wider):
            with pytest.raises(ValueError, match="into lies on"):
                call(into=bad)
        with pytest.raises(TypeError, match="CentreScores"):
            call(into=np.zeros((5, 9, 9), np.int64))
    for bad in ("staged", "", "DIRECT", "direct ", "lds"):
        monkeypatch.setenv("XSW_CENTRE_PATH", bad)
        for call in calls():
            with pytest.raises(ValueError, match="XSW_CENTRE_PATH"):
                call()


def test_good_arguments_reach_the_device(monkeypatch):
    reached = []

    def device(*arrays):
        reached.append(arrays)
        raise RuntimeError("the device")
    monkeypatch.setattr(centre, "_Call", device)
    for path in ("direct", None):
        if path is None:
            monkeypatch.delenv("XSW_CENTRE_PATH", raising=False)
        else:
            monkeypatch.setenv("XSW_CENTRE_PATH", path)
        for call in calls():
            with pytest.raises(RuntimeError, match="the device"):
                call(keep=np.ones((23, 31), bool), into=centre.CentreScores(np.zeros((5, 9, 9), np.int64), centre.CentreSpec(**GOOD)))
            with pytest.raises(RuntimeError, match="the device"):
                call(n=1, step_km=np.nan, annulus=(0.0, 3.0))
    assert len(reached) == 12


# --------------------------------------------------------------------------------------------------------------- declarations
def test_public_names():
    import xsarsea_amd
    assert xsarsea_amd.wind_centre_scores is centre.wind_centre_scores and xsarsea_amd.find_centre is centre.find_centre and xsarsea_amd.centre is centre
    assert xsarsea_amd.CentreScores is centre.CentreScores and xsarsea_amd.CentreSpec is centre.CentreSpec and xsarsea_amd.CentreFix is centre.CentreFix
    assert {"centre", "wind_centre_scores", "find_centre", "CentreScores", "CentreSpec", "CentreFix"} <= set(xsarsea_amd.__all__)
    assert {"CentreSpec", "CentreScores", "CentreFix", "wind_centre_scores", "codes_centre_scores", "find_centre"} <= set(centre.__all__)
    assert callable(CopolCodes.centre_scores) and callable(CopolCodes.find_centre) and centre.CentreScores.__iadd__ is centre.CentreScores.merge
    assert "only synchronisation" in centre.CentreScores.best.__doc__


def test_header_declares_the_entry_and_the_binding_has_one_letter_per_argument():
    entry = "xsw_wind_centre"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"include/xsw.h does not declare {entry}"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[0].startswith("xsw_ctx") and params[-1].startswith("int64_t *")
    polar = [p.strip() for p in re.search(r"\bint\s+xsw_wind_polar\s*\(([^)]*)\)\s*;", txt).group(1).split(",")]
    assert params[:17] == polar[:17]                       # xsw_wind_polar's arguments up to the tie tables
    assert [p.split()[-1] for p in params[17:]] == ["lon_g", "lat_g", "cos_lat_g", "sin_lat_g", "step_km", "n_c", "r_in_km", "r_out_km", "*sums"]
    sig = _lib.RASTER_ENTRIES[entry]
    assert len(sig) == len(params) - 1 == 25
    for letter, p in zip(sig, params[1:]):
        want = "p" if "*" in p else {"int64_t": "l", "int32_t": "i", "double": "d"}[p.split()[0]]
        assert letter == want, p
    assert entry in _lib.EXPORTS and hasattr(_lib.Context, "wind_centre_raw")
    assert hasattr(_lib.load(), entry)
    assert int(re.search(r"#\s*define\s+XSW_VERSION\s+(\d+)", txt).group(1)) == 4 == _lib.ABI_VERSION
    src = open(os.path.join(REPO, "xsarsea_amd", "csrc", "xsw_cells.hip")).read()
    assert int(re.search(r"#\s*define\s+XSW_CENTRE_MAX_N\s+(\d+)", src).group(1)) == centre.MAX_N
