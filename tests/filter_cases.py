"""The shapes and inputs that tests/test_filtering_cpu.py and tests/test_gpu_filter_seams.py share for the 32 x 32 tile kernels of
the rain filter (k_grad_mean, k_grad_filter) and for k_grad_smooth, with the restatement's results on them
(tests/filtering_ref.py), computed once and read-only.  Every property a case is there for is asserted on the restatement when
the case is built, before anything runs on a device; `check_all()` builds every case.

Seam pixel: an index i of an axis of length n is a seam index if i % 32 is 0 or 31 (the first and last row of a tile), or i < 6,
or i >= n - 6 (within Mean's reach of the raster's edge); a pixel is a seam pixel if either of its indices is one.

Designed inputs of the raw filter entry (xsw_grad_filter takes r2, G3, c and q4 separately): on rain scenes 70 - 95 % of a
filter's pixels sit on a plateau (exactly 0 or 1), where a wrong J, J1, G4 or zoom tap changes nothing.  Here, with
cb = (-1)**(x + y), u fresh uniform(-1, 1) noise per use and T a smooth tilt (a few 1e-3 per pixel, so that a read shifted by one
pixel changes a value at first order; B4 annihilates cb itself):
  set A   r2 = T (1 + 0.045 cb (1 + 0.1 u)):    P1 = sqrt(J1 - J**2) / J ~ 0.045, inside f1's ramp (0.035, 0.055)
  set B   r2 = 1 + 0.0224 cb (1 + 0.02 u):      (r2 - Z)**2 ~ 5.0e-4, inside f2's ramp (4e-4, 6e-4) J**2; no tilt, Z stays 1
  g3 = 3 T (1 + 0.4 cb phase) (1 + 0.05 u):     G3 / G4 ~ 1.4 or 0.6: f3's ramp (1.2, 1.6) on the pixels of one colour per phase
  c uniform in (0.29, 0.39):                    sqrt(c) inside f4's ramp (0.53, 0.63)
  q4 = 1 + 0.002 u on the (L // 2, S // 2) grid
f1's ramp begins at the P1 >= 0.035 that the derivation of ATOL = 1e-9 in tests/test_gpu_filtering.py assumes.
Test infrastructure only: the product never imports it.
"""
import functools

import numpy as np
from scipy import ndimage

import filtering_ref as fr

TILE, REACH = 32, 6

# output grids: the shape of Mean's input, of the filter's half-resolution rasters.  32k - 1 and 32k + 1 (a tile's reflected halo
# comes from its own last real row; a last tile of one row), exactly 32k on more than one tile, last tiles of 2, 5 and 6 (narrower
# than the reach: all of the right-hand halo reflects into the previous tile), 2-, 3- and 5-pixel axes across many tiles
OUTPUT_GRIDS = [(31, 33), (63, 65), (64, 32), (32, 96), (34, 37), (38, 70), (5, 66), (2, 700), (700, 3)]
RAW_GRIDS = OUTPUT_GRIDS + [(2, 2), (3, 2), (4, 4)]
MEAN_GRIDS = OUTPUT_GRIDS + [(1, 1), (1, 700), (700, 1)]
SMOOTH_GRIDS = MEAN_GRIDS + [(3, 63), (4, 64), (5, 65), (1, 129), (9, 130)]  # k_grad_smooth: 64 x 4 outputs per workgroup
BIG_GRIDS = [g for g in OUTPUT_GRIDS if min(g) >= 31]

SETS, PHASES = ("A", "B"), (1, -1)
NAN_KINDS = ("r2", "g3", "q4")
# the NaN variants of the designed inputs: (set, input with the NaN); f2 is inside its ramp on set B, where q4's NaN shows
NAN_CASES = (("A", "r2"), ("A", "g3"), ("B", "q4"))

# sigma0 shapes of the chain scenes: twice the output grids (the 4-row strip of 100 tiles' worth is (8, 200)), one odd pair
CHAIN_SHAPES = [(62, 66), (126, 130), (128, 64), (64, 192), (68, 74), (76, 140), (10, 132), (8, 200), (4, 1400), (1400, 6), (127, 131)]
CHAIN_GAMMA = {(10, 132): 200}  # everything else 20
CHAIN_NAN_EDGES = [(126, 130), (76, 140), (64, 192), (128, 64), (4, 1400), (1400, 6)]
CHAIN_CASES = [(s, False) for s in CHAIN_SHAPES] + [(s, True) for s in CHAIN_NAN_EDGES]

COARSEN_SHAPES = [(3, 2), (8, 128), (9, 131), (10, 258), (11, 127)]


def frozen(a):
    a.setflags(write=False)
    return a


def seam_index(n):
    i = np.arange(n)
    return (i % TILE == 0) | (i % TILE == TILE - 1) | (i < REACH) | (i >= n - REACH)


def seam_mask(shape):
    return seam_index(shape[0])[:, None] | seam_index(shape[1])[None, :]


def inside(f):
    """Strictly inside the ramp: neither plateau, not NaN."""
    with np.errstate(invalid="ignore"):
        return (f > 0) & (f < 1)


def edge_points(L, S):
    """The four corners and one pixel on each edge, as test_tile_kernels_on_seams_and_thin_rasters places its NaN."""
    return ((0, 0), (0, S - 1), (L - 1, 0), (L - 1, S - 1), (0, S // 2), (L - 1, S // 3), (L // 2, 0), (L // 3, S - 1))


# ------------------------------------------------------------------------------------- Mean / smoothing
@functools.lru_cache(maxsize=None)
def mean_input(shape, nan_edges=False):
    """A float64 raster of rain-scene values (positive, no plateau in play); nan_edges: NaN at the corners and on each edge."""
    x = fr.rain_scene(shape, np.float64, 100 + shape[0] + shape[1], land=False)
    if nan_edges:
        assert min(shape) >= 31
        for y, xx in edge_points(*shape):
            x[y, xx] = np.nan
    assert np.isnan(x).sum() == (8 if nan_edges else 0) and (x[~np.isnan(x)] > 0).all()
    return frozen(x)


@functools.lru_cache(maxsize=None)
def mean_want(shape, nan_edges=False):
    want = fr.Mean(mean_input(shape, nan_edges))
    if nan_edges:  # the reflected halos carry NaN, and something is left to compare
        assert np.isnan(want[0, 0]) and np.isnan(want[-1, -1]) and np.isfinite(want).mean() >= 0.1
    else:
        assert np.isfinite(want).all()
    return frozen(want)


@functools.lru_cache(maxsize=None)
def smoothing_want(shape, nan_edges=False):
    want = fr.smoothing(mean_input(shape, nan_edges))
    assert np.isnan(want).any() == nan_edges and np.isfinite(want).mean() >= 0.5
    return frozen(want)


# ------------------------------------------------------------------------------------- k_grad_smooth<true>
@functools.lru_cache(maxsize=None)
def coarsen_input(shape):
    """(x, want): x with NaN sprinkled so that the 2 x 2 groups of the NaN-skipping mean show every valid-count 0 .. 4 (one group
    only on the 3 x 2 raster: three valid, and a NaN in the trimmed row), want = smoothing(coarsen_mean(x))."""
    L, S = shape
    rng = np.random.default_rng(300 + L + S)
    x = 0.1 + rng.uniform(0, 0.05, shape)
    Lo, So = L // 2, S // 2
    if Lo * So == 1:
        missing = np.array([[1]])
    else:
        missing = rng.choice(5, size=(Lo, So), p=(0.70, 0.14, 0.08, 0.05, 0.03))
    for y, xx in np.argwhere(missing > 0):
        cells = rng.permutation(4)[: missing[y, xx]]
        for k in cells:
            x[2 * y + k // 2, 2 * xx + k % 2] = np.nan
    if L % 2:
        x[L - 1, S // 2] = np.nan  # trimmed: must not reach any output
    if S % 2:
        x[L // 2, S - 1] = np.nan
    coarse = fr.coarsen_mean(x, 2)
    valid = (~np.isnan(x[:2 * Lo, :2 * So])).reshape(Lo, 2, So, 2).sum(axis=(1, 3))
    np.testing.assert_array_equal(valid == 0, np.isnan(coarse))
    if Lo * So == 1:
        assert valid[0, 0] == 3
    else:
        assert set(np.unique(valid)) == {0, 1, 2, 3, 4}, np.unique(valid)
    want = fr.smoothing(coarse)
    assert want.shape == (Lo, So) and (Lo * So == 1 or (np.isnan(want).any() and np.isfinite(want).mean() >= 0.5))
    return frozen(x), frozen(want)


# ------------------------------------------------------------------------------------- the raw filter entry
def tilt(L, S):
    """Smooth, within 1 +- 0.1, at most 3.7e-3 per pixel."""
    y, x = np.mgrid[0:L, 0:S].astype(np.float64)
    return 1 + 0.1 * np.sin(0.03 * x + 0.021 * y + 0.5)


def nan_position(grid, kind):
    L, S = grid
    if kind == "r2":
        return min(31, L - 1), min(32, S - 1)  # the corner of four tiles, or the grid's nearest seam corner
    if kind == "g3":
        return L - 1, min(31, S - 1)           # on the raster's last row, on a tile's last column
    return (L // 2) // 2, S // 2 - 1           # q4: its last column


@functools.lru_cache(maxsize=None)
def designed(grid, which, phase, nan=None):
    """dict(r2, g3, c, q4) of input set `which` ("A" / "B") and g3 phase (+1 / -1) on `grid`; nan: None or the input that gets a
    single NaN ("r2", "g3", "q4")."""
    L, S = grid
    assert which in SETS and phase in PHASES and L >= 2 and S >= 2
    rng = np.random.default_rng(7003 + 10 * L + S + (0 if which == "A" else 500) + (0 if phase == 1 else 250))
    u = lambda shape=(L, S): rng.uniform(-1, 1, shape)
    y, x = np.mgrid[0:L, 0:S]
    cb = np.where((x + y) % 2 == 0, 1.0, -1.0)
    T = tilt(L, S)
    if which == "A":
        r2 = T * (1 + 0.045 * cb * (1 + 0.1 * u()))
    else:
        r2 = 1 + 0.0224 * cb * (1 + 0.02 * u())
    t = dict(r2=r2, g3=3 * T * (1 + 0.4 * cb * phase) * (1 + 0.05 * u()), c=rng.uniform(0.29, 0.39, (L, S)),
             q4=1 + 0.002 * u((L // 2, S // 2)))
    if nan is not None:
        assert nan in NAN_KINDS and min(grid) >= 31
        t[nan][nan_position(grid, nan)] = np.nan
    assert sum(int(np.isnan(v).sum()) for v in t.values()) == (0 if nan is None else 1)
    return {k: frozen(v) for k, v in t.items()}


def zoomed(q4, grid):
    """Z on `grid`: the restatement's zoom, which is asserted to be scipy's own (to the 1e-15 relative of
    test_zoom_linear_is_scipy_zoom, NaN positions equal)."""
    Z = fr.zoom_linear(q4, grid)
    z = ndimage.zoom(q4, (grid[0] / q4.shape[0], grid[1] / q4.shape[1]), order=1)
    assert z.shape == Z.shape == tuple(grid)
    np.testing.assert_array_equal(np.isnan(Z), np.isnan(z))
    m = ~np.isnan(z)
    assert (np.abs(Z[m] - z[m]) <= 1e-15 * np.abs(z[m])).all()
    return Z


def combine_with(t, mean=fr.Mean, Z=None):
    """The restatement's (f1, f2, f3, f4, F, d, J1) of designed inputs; `mean` / `Z` let a test put a wrong one in."""
    r2, g3 = t["r2"], t["g3"]
    Z = zoomed(t["q4"], r2.shape) if Z is None else Z
    return fr.combine(dict(r2=r2, G3=g3, c=t["c"], J=mean(r2), J1=mean(r2 ** 2), G4=mean(g3)), Z)


@functools.lru_cache(maxsize=None)
def designed_want(grid, which, phase, nan=None):
    want = combine_with(designed(grid, which, phase, nan))
    if nan is None:
        designed_conditions(grid)
    else:
        clean = designed_want(grid, which, phase)
        hit = {"r2": (0, 1), "g3": (2,), "q4": (1,)}[nan]
        for k in range(4):  # the NaN reaches the filters it should, and leaves at least half of every field
            assert np.isnan(want[k]).any() == (k in hit), (grid, nan, k)
            assert np.isfinite(want[k]).mean() >= 0.5 and np.isfinite(want[4]).mean() >= 0.5
            m = np.isfinite(want[k])
            np.testing.assert_array_equal(want[k][m], clean[k][m])
    return tuple(frozen(w) for w in want)


@functools.lru_cache(maxsize=None)
def designed_conditions(grid):
    """Asserts on the restatement, for the four (set, phase) inputs of `grid` without NaN: no NaN, no ill-conditioned pixel
    (d <= 1e-9 J1), f1 inside its ramp on >= 99 % of the pixels of set A, f2 on >= 99 % of set B, f4 on >= 99 % of both, f3 on
    >= 99 % of the pixels in one phase or the other.  Returns the shares."""
    shares = {}
    for which in SETS:
        f3_in = np.zeros(grid, bool)
        for phase in PHASES:
            w = combine_with(designed(grid, which, phase))
            f1, f2, f3, f4, F, d, J1 = w
            assert all(np.isfinite(a).all() for a in w), (grid, which, phase)
            assert not (d <= 1e-9 * J1).any(), (grid, which, phase)
            if which == "A":
                shares["f1", phase] = inside(f1).mean()
                assert inside(f1).mean() >= 0.99, (grid, phase, inside(f1).mean())
            else:
                shares["f2", phase] = inside(f2).mean()
                assert inside(f2).mean() >= 0.99, (grid, phase, inside(f2).mean())
            shares["f4", which, phase] = inside(f4).mean()
            assert inside(f4).mean() >= 0.99, (grid, which, phase)
            f3_in |= inside(f3)
        shares["f3", which] = f3_in.mean()
        assert f3_in.mean() >= 0.99, (grid, which, f3_in.mean())
    return shares


# ------------------------------------------------------------------------------------- the chain on sigma0
@functools.lru_cache(maxsize=None)
def chain_scene(shape, dtype, nan_edges=False):
    L, S = shape
    s0 = fr.rain_scene(shape, dtype, 40 + L + S, CHAIN_GAMMA.get(shape, 20), land=False)
    if nan_edges:
        assert shape in CHAIN_NAN_EDGES
        for y, x in edge_points(L, S):
            s0[y, x] = np.nan
    assert np.isnan(s0).sum() == (8 if nan_edges else 0) and s0.dtype == dtype
    return frozen(s0)


@functools.lru_cache(maxsize=None)
def chain_want(shape, dtype, nan_edges=False):
    """The restatement's (f1, f2, f3, f4, F, d, J1) of the chain scene.  Without NaN: every filter has at least 16 seam pixels
    strictly inside its ramp, at most 0.1 % ill-conditioned pixels and at least 80 % finite outputs.  With nan_edges: at least
    half of every field finite (what `compare` demands) and NaN on the half-resolution raster's corners."""
    want = fr.filtering_parameters(chain_scene(shape, dtype, nan_edges))
    seam = seam_mask(want[0].shape)
    counts = [int((inside(f) & seam).sum()) for f in want[:4]]
    ill, _min_ramp, finite, _ramps = fr.conditions(*want)
    assert ill <= 1e-3, (shape, ill)
    if nan_edges:
        assert all(np.isfinite(f).mean() >= 0.5 for f in want[:5]), shape
        assert all(np.isnan(want[4][p]) for p in ((0, 0), (0, -1), (-1, 0), (-1, -1)))
    else:
        assert min(counts) >= 16, (shape, np.dtype(dtype).name, counts)
        assert finite >= 0.8, (shape, finite)
    return tuple(frozen(w) for w in want)


def check_all():
    """Builds every case, so that each case's assertions run."""
    for g in SMOOTH_GRIDS:
        smoothing_want(g)
        if g in MEAN_GRIDS:
            mean_want(g)
    for g in BIG_GRIDS:
        mean_want(g, True), smoothing_want(g, True)
    for s in COARSEN_SHAPES:
        coarsen_input(s)
    for g in RAW_GRIDS:
        designed_conditions(g)
        for which in SETS:
            for phase in PHASES:
                designed_want(g, which, phase)
    for g in BIG_GRIDS:
        for which, nan in NAN_CASES:
            designed_want(g, which, 1, nan)
    for shape, nan_edges in CHAIN_CASES:
        for dtype in (np.float32, np.float64):
            chain_want(shape, dtype, nan_edges)

