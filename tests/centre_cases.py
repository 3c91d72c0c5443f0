"""The scene and the lattices that tests/test_centre_cpu.py and tests/test_gpu_centre.py share, and the restatement's results on
them (tests/centre_ref.py), computed once and read-only.  `case(name, dtype)` asserts the property each case is there for on the
restatement, before anything runs on a device.  The scene is tests/polar_cases.py's 97 x 300 raster (pixels of about half a
kilometre, the 300 m/s pixel, the NaN forms, the keep mask) with its two tie grids: k_wind_centre gives a workgroup 32 lines x 256 columns of it,
so that a tile of 512 entries is swept many times per workgroup and the sample axis needs a second, ragged workgroup -- the
smallest shape that reaches every part of the kernel.  `vortex()` is the modified Rankine vortex of the recovery tests."""
import functools

import numpy as np

import centre_ref as cref
import polar_cases as pc
import polar_ref as pref

L, S = pc.L, pc.S
MID = pc.CASES["quadrants"]["centre"]

# name -> (the tie grid of polar_cases, the public call's keyword arguments; first_guess None: that polar case's own centre,
# "east": near pixel (48, 250), so that the lattice lies across the border of the two workgroup columns)
CASES = {
    # n = 1, r_in = 0: planes 0-4 of wind_polar with one ring, added over its sectors -- at every centre of polar_cases
    "one_quadrants": ("quadrants", dict(first_guess=None, step_km=1.0, n=1, annulus=(0.0, 20.0))),
    "one_offscene": ("offscene", dict(first_guess=None, step_km=1.0, n=1, annulus=(0.0, 90.0))),
    "one_antimeridian": ("antimeridian", dict(first_guess=None, step_km=1.0, n=1, annulus=(0.0, 7.5))),
    "one_antimeridian_twin": ("antimeridian", dict(first_guess=pc.ANTIMERIDIAN_TWIN["centre"], step_km=1.0, n=1, annulus=(0.0, 7.5))),
    "one_axes": ("axes", dict(first_guess=None, step_km=1.0, n=1, annulus=(0.0, 20.0))),
    "small": ("quadrants", dict(first_guess=MID, step_km=2.0, n=9, annulus=(0.0, 5.0))),      # 81 candidates: three thread groups share the tile
    "wide": ("quadrants", dict(first_guess="east", step_km=1.5, n=17, annulus=(0.0, 4.0))),      # 289: a thread owns two
    "full": ("quadrants", dict(first_guess="east", step_km=1.0, n=31, annulus=(0.0, 5.0))),      # 961: a thread owns four
    "ring": ("axes", dict(first_guess=None, step_km=2.0, n=9, annulus=(3.0, 8.0))),           # r_in > 0; the guess is a pixel: r == 0 there
    "offscene": ("offscene", dict(first_guess=None, step_km=10.0, n=9, annulus=(0.0, 12.0))), # the guess outside the raster, candidates without a pixel
}
ONES = [n for n in CASES if n.startswith("one_")]


def ties(name):
    return pc.ties(CASES[name][0])


@functools.lru_cache(maxsize=None)
def spec(name):
    """The public call's keyword arguments of a case."""
    grid, kw = CASES[name]
    kw = dict(kw)
    if kw["first_guess"] is None:
        kw["first_guess"] = pc.spec(grid)["centre"]
    elif kw["first_guess"] == "east":
        lon, lat, _, _ = pc.geolocation(grid)
        kw["first_guess"] = (round(float(lon[48, 250]), 5), round(float(lat[48, 250]), 5))
    return kw


def pixels(name, dtype=np.complex128):
    """centre_ref.pixel_chart of a case: ok, x, y, u, v, sp, q of every pixel."""
    w, keep = pc.scene(dtype)
    lon_g, lat_g = spec(name)["first_guess"]
    return cref.pixel_chart(*pc.geolocation(CASES[name][0]), w, keep, lon_g, lat_g, *pref.tables(lat_g, 4)[:2])


def survivors(name):
    """The pixels k_wind_centre's walk stages: inside the square of half width h * step_km + r_out_km (the margin is rounding's)."""
    kw, p = spec(name), pixels(name)
    bound = (kw["n"] - 1) // 2 * (kw["step_km"] if kw["n"] > 1 else 0.0) + kw["annulus"][1]
    with np.errstate(invalid="ignore"):
        return p["ok"] & (np.abs(p["x"]) < bound) & (np.abs(p["y"]) < bound)


@functools.lru_cache(maxsize=None)
def case(name, dtype=np.complex128):
    """(sums, finished fields) of the restatement for case `name`, with the case's property asserted."""
    w, keep = pc.scene(dtype)
    kw = spec(name)
    s = cref.sums(w, *ties(name), **kw, keep=keep)
    n, nn = s[0], kw["n"]
    p, sv = pixels(name, dtype), survivors(name)
    valid = int(p["ok"].sum())
    assert s.shape == (5, nn, nn) and s.dtype == np.int64 and 0.8 * L * S < valid < 0.9 * L * S
    assert not p["ok"][50, 150] and p["q"][50, 150] == 90000.0 and p["ok"][pc.FAST]           # the 300 m/s pixel is dropped, the 200 m/s one is not
    assert n.max() <= sv.sum() and 0 < sv.sum() < valid                                      # the cull keeps some pixels and drops others
    if name in ONES:
        assert nn == 1 and kw["annulus"][0] == 0.0 and n[0, 0] > 300
    elif name in ("small", "wide", "full"):
        assert (nn * nn < 256 and 256 // (nn * nn) == 3) if name == "small" else (256 < nn * nn <= 512) if name == "wide" else nn == 31
        assert (n > 0).all() and n.sum() > 8 * sv.sum()                                      # a staged pixel meets many candidates
        # a workgroup's 32 lines x 256 columns hold more survivors than a tile: `small` three tiles in one workgroup column, the
        # other two more than one in each of the six workgroups of the first 96 lines, on both sides of the column border
        blocks = [int(sv[a:a + 32, b:b + 256].sum()) for a in range(0, L, 32) for b in range(0, S, 256)]
        assert max(blocks) > 3 * 512 if name == "small" else min(blocks[:6]) > 512, blocks
    elif name == "ring":
        i, j = pc.AXES_PIXEL
        h = (nn - 1) // 2
        r = np.hypot(p["x"], p["y"])
        assert p["x"][i, j] == 0.0 and p["y"][i, j] == 0.0 and p["ok"][i, j] and kw["annulus"][0] > 0.0
        inside, beyond = p["ok"] & (r < kw["annulus"][0]), p["ok"] & (r >= kw["annulus"][1])
        assert inside.sum() > 20 and beyond.sum() > 1000 and n[h, h] == (p["ok"] & ~inside & ~beyond).sum() > 150
        assert not (p["ok"] & ((r == kw["annulus"][0]) | (r == kw["annulus"][1]))).any()     # pixels on neither border
    elif name == "offscene":
        lon, lat, _, _ = pc.geolocation(CASES[name][0])
        g = kw["first_guess"]
        assert not (lon.min() <= g[0] <= lon.max() and lat.min() <= g[1] <= lat.max())
        assert 5 < (n > 0).sum() < nn * nn - 5 and n[(nn - 1) // 2, (nn - 1) // 2] == 0, int((n > 0).sum())
    s.setflags(write=False)
    return s, cref.finish(s)


# ---------------------------------------------------------------------------------------------------- the vortex of the recovery tests
VM, RM, DECAY, INFLOW, NOISE, SEED = 50.0, 6.0, 0.5, 20.0, 2.0, 3
DX_KM, DY_KM = 0.44, 0.39                     # the pixel of the vortex's raster, east and north
TRUE_OFFSETS = ((3.0, -2.0), (-6.0, 4.0))     # the true centre's (x, y) from the first guess, km: nodes of the lattices below


@functools.lru_cache(maxsize=None)
def vortex(offset=TRUE_OFFSETS[0], south=False):
    """A modified Rankine vortex (Vm = 50 m/s at Rm = 6 km, V ~ r**-0.5 outside, 20 degrees of inflow, Gaussian noise of 2 m/s per
    component, seed 3) on the scene's 97 x 300 pixels, laid out in the chart's own coordinates around the first guess (a tie point
    per pixel, heading 0), its centre `offset` km east and north of the guess; counter-clockwise, or its mirror image, clockwise,
    for the southern hemisphere.  Returns (wind, tie arguments, first guess)."""
    guess = (130.0, -20.0 if south else 20.0)
    x, y = np.meshgrid((np.arange(S) - 149.5) * DX_KM, -(np.arange(L) - 48.0) * DY_KM)   # east, north; line 0 is the northernmost
    cos_g, sin_g = pref.tables(guess[1], 4)[:2]
    dy = y / pref.R_KM
    h = 0.5 * dy
    lat = guess[1] + dy / pref.D2R
    lon = guess[0] + x / (pref.KX * ((cos_g - sin_g * h) - (0.5 * cos_g) * (h * h)))
    dx, dy = x - offset[0], y - offset[1]
    r = np.hypot(dx, dy)
    assert r.min() > 0.0
    speed = np.where(r < RM, VM * r / RM, VM * (RM / r) ** DECAY)
    turn = -1.0 if south else 1.0
    a = np.deg2rad(INFLOW)
    u = speed * (np.cos(a) * turn * (-dy / r) - np.sin(a) * dx / r)
    v = speed * (np.cos(a) * turn * (dx / r) - np.sin(a) * dy / r)
    rng = np.random.default_rng(SEED)
    u, v = u + NOISE * rng.standard_normal(u.shape), v + NOISE * rng.standard_normal(v.shape)
    w = -u - 1j * v
    w.setflags(write=False)
    return w, (np.arange(float(L)), np.arange(float(S)), lon, lat, np.zeros((L, S))), guess


def true_node(offset, step_km, n):
    """(i, j) of the lattice node at `offset`."""
    h = (n - 1) // 2
    i, j = h + offset[1] / step_km, h + offset[0] / step_km
    assert i == int(i) and j == int(j) and 0 <= i < n and 0 <= j < n
    return int(i), int(j)
