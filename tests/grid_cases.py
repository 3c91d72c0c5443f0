"""The scene and the grids that tests/test_grid_cpu.py and tests/test_gpu_grid.py share, and the restatement's results on them
(tests/grid_ref.py), computed once and read-only.  `case(name, dtype)` asserts the property each grid is there for on the
restatement, before anything runs on a device."""
import functools

import numpy as np

import grid_ref as gref

L, S = 97, 300
TIE_LINE, TIE_SAMPLE = np.array([0.0, 40.0, 96.0]), np.array([0.0, 100.0, 220.0, 299.0])

# name -> (lon0, dlon, n_lon, lat0, dlat, n_lat)
GRIDS = {
    "coarse": (179.0, 0.25, 8, 9.5, 0.25, 6),          # 15 occupied bins, 13 of more than 256 pixels: register runs, LDS merges
    "fine": (179.2, 0.001, 1400, 9.8, 0.001, 600),     # every valid pixel alone in its bin: table conflicts, the direct fallback
    "desc": (179.0, 0.05, 30, 10.4, -0.05, 12),        # a descending latitude axis, more than 200 occupied bins
    "partial": (179.5, 0.1, 5, 10.0, 0.1, 2),          # fewer than a third of the valid pixels fall inside
    "periodic": (-180.0, 0.5, 720, 9.0, 0.5, 4),       # bins occupied at both ends of the longitude axis
}


def wrap(lon):
    return (lon + 180.0) % 360.0 - 180.0


def ties():
    """(tie_line, tie_sample, longitude as a product gives it: wrapped into [-180, 180), latitude, heading in degrees)."""
    l, s = TIE_LINE[:, None], TIE_SAMPLE[None, :]
    return TIE_LINE, TIE_SAMPLE, wrap(179.2 + 0.004 * s + 0.0007 * l), 10.0 + 0.0035 * l - 0.0006 * s, -12.0 + 0.01 * l + 0.002 * s


@functools.lru_cache(maxsize=None)
def scene(dtype=np.complex128):
    """(wind, keep): winds N(0, 12) + 1j N(0, 12), 5 % of them NaN in the three forms of tests/test_gpu_cells.py, one pixel of
    300 m/s, a keep mask with a tenth of zeros."""
    rng = np.random.default_rng(2310)
    w = rng.normal(0.0, 12.0, (L, S)) + 1j * rng.normal(0.0, 12.0, (L, S))
    kind = rng.uniform(size=(L, S))
    w[kind < 0.017] = complex(np.nan, 0.0)
    w[(kind >= 0.017) & (kind < 0.034)] = complex(np.nan, np.nan)
    w.imag[(kind >= 0.034) & (kind < 0.05)] = np.nan        # finite + NaN j
    w[50, 150] = 180.0 - 240.0j                              # 300 m/s: dropped by the speed cap alone
    keep = rng.uniform(size=(L, S)) < 0.9
    keep[50, 150] = True
    w = w.astype(dtype)
    w.setflags(write=False)
    keep.setflags(write=False)
    return w, keep


@functools.lru_cache(maxsize=None)
def pixels(dtype=np.complex128):
    """What the restatement makes of every pixel of the scene: dict(ok, u, v, sp, q, lon, lat)."""
    w, keep = scene(dtype)
    tl, ts, lon, lat, heading = ties()
    h = np.deg2rad(heading)
    lf, lt = gref.bracket(tl, np.arange(float(L)))
    sf, st = gref.bracket(ts, np.arange(float(S)))
    plon, plat, ch, sh = gref.geolocate(gref.continuous(lon), lat, np.cos(h), np.sin(h), lf, lt, sf, st)
    ok, u, v, sp, q = gref.pixel_terms(w, keep, ch, sh)
    return dict(ok=ok, u=u, v=v, sp=sp, q=q, lon=plon, lat=plat)


@functools.lru_cache(maxsize=None)
def case(name, dtype=np.complex128):
    """(sums, finished fields) of the restatement for grid `name`, with the grid's property asserted."""
    w, keep = scene(dtype)
    grid = GRIDS[name]
    s = gref.sums(w, *ties(), grid, keep=keep)
    p = pixels(dtype)
    n = s[0]
    valid = int(p["ok"].sum())
    assert not p["ok"][50, 150] and p["q"][50, 150] == 90000.0 and 0.8 * L * S < valid < 0.9 * L * S
    if name == "coarse":
        # 13 of the 15 bins hold more than 256 pixels; the scene's corners leave 16 and 49 in the other two
        assert (n > 0).sum() == 15 and (n > 256).sum() == 13 and n.sum() == valid, (int((n > 0).sum()), int((n > 256).sum()))
    elif name == "fine":
        assert n.max() == 1 and n.sum() == valid and n.size == 840000
    elif name == "desc":
        assert grid[4] < 0 and (n > 0).sum() > 200 and n.sum() == valid
    elif name == "partial":
        assert 0 < n.sum() < valid / 3
    elif name == "periodic":
        assert gref.periodic_of(grid[1], grid[2]) and n[:, 0].sum() > 0 and n[:, -1].sum() > 0 and n.sum() == valid
    s.setflags(write=False)
    return s, gref.finish(s)
