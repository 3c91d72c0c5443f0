"""The scene and the bins that tests/test_polar_cpu.py and tests/test_gpu_polar.py share, and the restatement's results on them
(tests/polar_ref.py), computed once and read-only.  `case(name, dtype)` asserts the property each case is there for on the
restatement, before anything runs on a device.  The scene is tests/grid_cases.py's 97 x 300 raster and tie points (the 300 m/s
pixel, the three NaN forms, the keep mask) with one more pixel of 200 m/s, which must set its bin's largest speed."""
import functools

import numpy as np

import grid_cases as gc
import polar_ref as pref

L, S = gc.L, gc.S
FAST = (20, 40)   # the pixel of 200 m/s

# name -> dict(centre=(lon, lat), radius=(dr_km, n_r), sectors=n_theta).  The tie grid is linear in line and sample with steps of
# 1e-4 degree, so a centre given to four decimals has pixels on its meridian and its parallel to the last bit; the centres carry a
# fifth decimal, and `antimeridian`, whose longitude is given, keeps the two pixels of longitude 180.4 (8 km away) outside its rings.
CASES = {
    "quadrants": dict(centre=(179.85137, 10.07873), radius=(15.0, 6), sectors=4),     # most occupied bins above 256 pixels: register runs, LDS merges
    "fine": dict(centre=(179.85137, 10.07873), radius=(0.1, 800), sectors=360),       # bisection depth 7, most pixels alone in their bin
    "offscene": dict(centre=(179.00013, 10.60007), radius=(5.0, 14), sectors=24),     # fewer than a third of the valid pixels inside
    "antimeridian": dict(centre=(-179.6, 10.03637), radius=(0.5, 15), sectors=72),    # the same centre as (180.4, 10.03637); a whole disc
    "axes": dict(centre=None, radius=(2.0, 40), sectors=16),                          # the centre is a pixel of the second tie grid
}
ANTIMERIDIAN_TWIN = dict(CASES["antimeridian"], centre=(180.4, 10.03637))

# the second tie grid: every blend weight and every value is a short dyadic fraction, so that longitude depends on the sample
# alone, latitude on the line alone, and both exactly
AXES_PIXEL = (40, 100)
AXES_TIE_LINE, AXES_TIE_SAMPLE = np.array([0.0, 32.0, 64.0, 96.0]), np.array([0.0, 512.0])


def axes_ties():
    l, s = AXES_TIE_LINE[:, None], AXES_TIE_SAMPLE[None, :]
    return AXES_TIE_LINE, AXES_TIE_SAMPLE, 100.0 + s / 128.0 + 0.0 * l, 20.0 - l / 128.0 + 0.0 * s, 7.0 + 0.02 * l + 0.004 * s


def ties(name):
    return axes_ties() if name == "axes" else gc.ties()


@functools.lru_cache(maxsize=None)
def scene(dtype=np.complex128):
    """(wind, keep) of tests/grid_cases.py with the pixel of 200 m/s."""
    w, keep = gc.scene(np.complex128)
    w, keep = np.array(w), np.array(keep)
    w[FAST] = 120.0 - 160.0j
    keep[FAST] = True
    w = w.astype(dtype)
    w.setflags(write=False)
    keep.setflags(write=False)
    return w, keep


@functools.lru_cache(maxsize=None)
def geolocation(name):
    """(lon, lat, ch, sh) of every pixel, by the restatement."""
    tl, ts, lon, lat, heading = ties(name)
    return pref.gref.geolocate(*pref.tie_tables(tl, ts, lon, lat, heading, np.arange(float(L)), np.arange(float(S))))


@functools.lru_cache(maxsize=None)
def spec(name):
    """The public call's keyword arguments of a case."""
    kw = dict(CASES[name])
    if name == "axes":
        lon, lat, _, _ = geolocation("axes")
        kw["centre"] = (float(lon[AXES_PIXEL]), float(lat[AXES_PIXEL]))
    return kw


def pixels(name, dtype=np.complex128, kw=None):
    """What the restatement makes of every pixel of a case: polar_ref.pixel_bins."""
    kw = kw or spec(name)
    w, keep = scene(dtype)
    (lon_c, lat_c), (dr_km, n_r), n_theta = kw["centre"], kw["radius"], kw["sectors"]
    cos_c, sin_c, ssin, scos = pref.tables(lat_c, n_theta)
    return pref.pixel_bins(*geolocation(name), w, keep, lon_c, lat_c, cos_c, sin_c, dr_km, n_r, n_theta, ssin, scos)


@functools.lru_cache(maxsize=None)
def case(name, dtype=np.complex128):
    """(sums, finished fields) of the restatement for case `name`, with the case's property asserted."""
    w, keep = scene(dtype)
    kw = spec(name)
    s = pref.sums(w, *ties(name), **kw, keep=keep)
    p = pixels(name, dtype)
    n, mq = s[0], kw["sectors"] // 4
    valid = int(p["valid"].sum())
    assert s.shape == (6, kw["radius"][1], kw["sectors"]) and n.sum() == p["ok"].sum()
    assert not p["valid"][50, 150] and p["q"][50, 150] == 90000.0 and p["valid"][FAST] and p["q"][FAST] == 40000.0 and 0.8 * L * S < valid < 0.9 * L * S
    assert p["ok"][FAST] == (name in ("quadrants", "fine", "axes"))
    if p["ok"][FAST]:   # the 200 m/s pixel is its bin's largest speed, and every bin's largest is at least its mean
        assert s[5][p["kr"][FAST], p["sector"][FAST]] == 200 * 2 ** 24 == s[5].max()
    assert (s[5][n > 0] * n[n > 0] >= s[1][n > 0]).all() and (s[5][n == 0] == 0).all()
    if name == "quadrants":
        assert n.sum() == valid and (n > 256).sum() > 0.5 * (n > 0).sum() and (n > 0).sum() >= 12, (int((n > 0).sum()), int((n > 256).sum()))
    elif name == "fine":
        assert mq == 90 and int(np.ceil(np.log2(mq))) == 7 and kw["radius"][0] < 0.3          # a pixel is 0.39 km x 0.44 km
        assert n.sum() > 0.9 * valid and (n == 1).sum() > 0.5 * n.sum(), (int(n.sum()), int((n == 1).sum()))
        assert len(np.unique(p["sector"][p["ok"]])) > 350   # (a sector along the raster's own lines can stay empty)
    elif name == "offscene":
        lon, lat, _, _ = geolocation(name)
        assert not (lon.min() <= kw["centre"][0] <= lon.max() and lat.min() <= kw["centre"][1] <= lat.max())
        assert 0 < n.sum() < valid / 3
    elif name == "antimeridian":
        twin = pref.sums(w, *ties(name), **ANTIMERIDIAN_TWIN, keep=keep)
        assert np.array_equal(twin, s) and n.sum() > 700 and (n.sum(axis=0) > 0).sum() >= 70   # (two pixels lie on the centre's meridian exactly, 8 km away: outside)
        lon = geolocation(name)[0]
        assert lon.min() < 180.0 < kw["centre"][0] + 360.0 < lon.max()     # the scene straddles the antimeridian, the centre beyond it
    elif name == "axes":
        lon, lat, _, _ = geolocation(name)
        i, j = AXES_PIXEL
        assert np.array_equal(lon, np.broadcast_to(100.0 + np.arange(float(S)) / 128.0, (L, S))) and np.array_equal(lat, np.broadcast_to(20.0 - np.arange(float(L))[:, None] / 128.0, (L, S)))
        assert (p["r"] == 0.0).sum() == 1 and p["r"][i, j] == 0.0 and p["sector"][i, j] == 0 and p["kr"][i, j] == 0
        assert (p["y"][i] == 0.0).all() and (p["x"][:, j] == 0.0).all() and (p["x"][:, :j] < 0.0).all() and (p["x"][:, j + 1:] > 0.0).all()
        assert (p["y"][:i] > 0.0).all() and (p["y"][i + 1:] < 0.0).all()
        # on the axes the sign rules alone decide: north -> Q 0, east -> Q 1, south -> Q 2, west -> Q 3, each at its first sector
        for rows, cols, sector in ((slice(0, i), j, 0), (i, slice(j + 1, None), mq), (slice(i + 1, None), j, 2 * mq), (i, slice(0, j), 3 * mq)):
            assert (p["sector"][rows, cols] == sector).all() and p["ok"][rows, cols].sum() > 10
        assert p["ok"][i, j] and (p["vr"][i, j], p["vt"][i, j]) == (0.0, 0.0)
        assert len(np.unique(p["sector"][p["ok"]])) == 16
    s.setflags(write=False)
    return s, pref.finish(s)
