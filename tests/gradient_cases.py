"""The inputs that tests/test_gradients_exact_cpu.py and tests/test_gpu_gradients_exact.py share for the bit-for-bit comparison of
k_grad_r2, k_grad_local, k_grad_smooth, k_grad_mean and k_grad_filter with tests/gradients_exact.py: the smallest shapes that reach
each edge of the 16 x 16 and 32 x 32 tiles, and designed inputs whose property is asserted on the restatement when the case is
built, before anything runs on a device.  Everything is computed once and read-only; `check_all()` builds every case.

sigma0 cases (float32 and float64; R2 by both entries, the local gradients of ampl = sqrt(sigma0) by both entries):
  thin-*      THIN_CASES of tests/test_gpu_gradients.py: one tile or less, one coarse row or column across 22 tiles, coarse axes
              of 16k - 1 and 16k + 1, two of them with NaN on the corners and edges
  chain-*     the chain scenes of tests/filter_cases.py (the half-resolution grids are the seam shapes of the 32 x 32 tiles)
  tiles-70x134, scene-203x317   several tiles both ways (coarse 35 x 67; 101 x 158), with NaN land
  designed-90x101   NaN on the four corners, on each edge and once alone; two pairs of NaN placed so that the 2 x 2 groups of the
              NaN-skipping mean show every valid count 0 .. 4 (asserted for k_grad_r2's groups and for k_grad_local's); negative
              sigma0 (NaN under the root-on-load entries) and exact zeros; a flat patch, where zr = zi = za = 0: the (0, y)
              branch of the complex root and c = 0 / 1e-5 = 0
ampl cases (float64, xsw_grad_local only; a root on load would bend them):
  ramp-*      ampl = (a x + b y) k for (a, b) in (3, 4), (4, 3), (3, -4), (-4, 3) and k in 1, 2**20: away from the border grad**2 is
              the Pythagorean triple (dx**2 - dy**2, 2 dx dy, dx**2 + dy**2) in exact integers, both branches of the root occur
              (zr < 0, zr > 0) with both signs of zi, and at k = 2**20 za + 1e-5 rounds to za: c = 1.0 exactly, which must be kept.
filter cases (the raw entry xsw_grad_filter): the designed in-ramp inputs of tests/filter_cases.py with their NaN variants, and
  noise-*     r2 = 1 + 2e-9 u: J1 - J**2 is rounding noise of both signs; where the exact restatement has it negative f1 and F are
              NaN, and a kernel that follows the stated order has the same sign on every pixel.
Test infrastructure only: the product never imports it.
"""
import functools

import numpy as np

import filter_cases as fc
import gradients_exact as gx
from test_gpu_gradients import THIN_CASES, scene

DTYPES = (np.float32, np.float64)
frozen = fc.frozen


def shape_name(prefix, shape, nan_edges=False):
    return f"{prefix}-{shape[0]}x{shape[1]}" + ("-nan" if nan_edges else "")


# ------------------------------------------------------------------------------------------------------ sigma0 cases
DESIGNED = (90, 101)
FLAT = (slice(44, 72), slice(50, 80))          # fine pixels of the flat patch
ZEROS = (slice(20, 24), slice(60, 66))
NEGATIVE = ((30, 12), (31, 12), (60, 20))
# two NaN whose footprints overlap into an inner corner on the 2 x 2 grid (valid counts 1 and 3): the first's last row even and
# the second's first column odd, for the 5 x 5 footprint of k_grad_r2 and for the 7 x 7 (Scharr, then B4) of k_grad_local
NAN_PAIRS = ((10, 26), (13, 29), (41, 11), (44, 14))
NAN_ALONE = (32, 84)


def designed_sigma0(dtype):
    L, S = DESIGNED
    s0 = scene(DESIGNED, np.float64, 77, land=False)
    for p in fc.edge_points(L, S) + NAN_PAIRS + (NAN_ALONE,):
        s0[p] = np.nan
    for p in NEGATIVE:
        s0[p] = -s0[p]
    s0[FLAT] = 0.0625
    s0[ZEROS] = 0.0
    return s0.astype(dtype)


def thin_sigma0(shape, nan_edges, dtype):
    """The scene of test_tile_kernels_on_seams_and_thin_rasters."""
    L, S = shape
    s0 = scene(shape, dtype, 14 + L + S, land=False)
    if nan_edges:
        for p in fc.edge_points(L, S):
            s0[p] = np.nan
    return s0


SIGMA0 = {}
for _shape, _nan in THIN_CASES:
    SIGMA0[shape_name("thin", _shape, _nan)] = functools.partial(thin_sigma0, _shape, _nan)
for _shape, _nan in fc.CHAIN_CASES:
    SIGMA0[shape_name("chain", _shape, _nan)] = functools.partial(lambda s, n, dt: np.array(fc.chain_scene(s, dt, n)), _shape, _nan)
SIGMA0["tiles-70x134"] = lambda dt: scene((70, 134), dt, 204)
SIGMA0["scene-203x317"] = lambda dt: scene((203, 317), dt, 1)
SIGMA0[shape_name("designed", DESIGNED)] = designed_sigma0
SIGMA0_NAMES = tuple(SIGMA0)
# cases whose sigma0 has at least 4 x 4 pixels: filtering_parameters runs on them
CHAIN_NAMES = tuple(n for n in SIGMA0_NAMES if min(int(v) for v in n.split("-")[1].split("x")) >= 4)


@functools.lru_cache(maxsize=None)
def sigma0(name, dtype):
    s0 = SIGMA0[name](dtype)
    assert s0.dtype == dtype and s0.ndim == 2 and max(s0.shape) <= 1400 and s0.size <= 203 * 317 and not np.isinf(s0).any()
    return frozen(s0)


def valid_counts(planes):
    """Valid members of every 2 x 2 group of the conv5 results of `planes` (a member is skipped when any plane is NaN there)."""
    nan = None
    for p in planes:
        q = [np.isnan(m) for m in gx.quad(gx.conv5(p))]
        nan = q if nan is None else [a | b for a, b in zip(nan, q)]
    return sum((~m).astype(int) for m in nan)


@functools.lru_cache(maxsize=None)
def r2_want(name, dtype, root_on_load, take_sqrt):
    return frozen(gx.r2_exact(sigma0(name, dtype), root_on_load, take_sqrt))


@functools.lru_cache(maxsize=None)
def ampl(name, dtype):
    """sqrt(sigma0) in the input's dtype, widened: what xsw_grad_local_sqrt loads and what xsw_grad_local is handed."""
    return frozen(gx.rooted(sigma0(name, dtype)))


def no_knife_edge(b, label):
    """The condition of the bracket on c: no pixel whose cut to 0 could fall either way, none that is cut for certain."""
    assert int(b.knife.sum()) == 0 and int(b.above.sum()) == 0, (label, int(b.knife.sum()), int(b.above.sum()))


@functools.lru_cache(maxsize=None)
def local_bracket(name, dtype):
    b = gx.LocalBracket(ampl(name, dtype))
    no_knife_edge(b, name)
    if name.startswith("designed"):
        designed_conditions(dtype, b)
    return b


def designed_conditions(dtype, b):
    s0 = sigma0(shape_name("designed", DESIGNED), dtype)
    a = ampl(shape_name("designed", DESIGNED), dtype)
    L, S = s0.shape
    assert all(np.isnan(s0[p]) for p in fc.edge_points(L, S)) and (s0[ZEROS] == 0).all() and all(s0[p] < 0 for p in NEGATIVE)
    assert all(np.isnan(a[p]) for p in NEGATIVE) and (a[ZEROS] == 0).all() and (a[FLAT] == 0.25).all()
    # every valid count of the 2 x 2 mean: R2 with and without the root on load (a negative sigma0 is a NaN only with it), and
    # the complex pair and the modulus plane of the local gradients
    re, im = gx.grad2(a)
    for planes in ((s0.astype(np.float64),), (a,), (re, im), (gx.hyp_centre(re, im),)):
        assert set(np.unique(valid_counts(planes))) == {0, 1, 2, 3, 4}
    # the corners and the edge points reach the output as NaN, the NaN that stands alone has its own island
    r2 = gx.r2_exact(s0, True)
    assert all(np.isnan(r2[p]) for p in ((0, 0), (0, -1), (-1, 0), (-1, -1))) and np.isnan(r2[NAN_ALONE[0] // 2, NAN_ALONE[1] // 2])
    assert np.isfinite(r2).mean() >= 0.5 and np.isfinite(b.za).mean() >= 0.5
    # the flat patch: zr = zi = za = 0 on the coarse pixels whose whole footprint is flat, the (0, y) branch, c = 0
    inner = (slice(FLAT[0].start // 2 + 4, FLAT[0].stop // 2 - 4), slice(FLAT[1].start // 2 + 4, FLAT[1].stop // 2 - 4))
    assert b.zr[inner].size >= 16
    for v in (b.zr, b.zi, b.za, b.za_lo, b.za_hi, b.re, b.im, b.c):
        assert gx.same_bits(v[inner], np.zeros_like(v[inner])), "the flat patch is not exactly +0.0"
    assert (b.branch[inner] == 1).all() and {0, 1, 2, 3} <= set(np.unique(b.branch))


# -------------------------------------------------------------------------------------------------------- the ramps
RAMP_SHAPE = (44, 70)   # coarse 22 x 35: more than one tile both ways
RAMPS = tuple((a, b, k) for (a, b) in ((3, 4), (4, 3), (3, -4), (-4, 3)) for k in (1, 2 ** 20))
RAMP_NAMES = tuple(f"ramp-{a}x{b:+d}y-k{'1' if k == 1 else '2p20'}" for a, b, k in RAMPS)


@functools.lru_cache(maxsize=None)
def ramp(name):
    """(ampl, bracket, interior): interior marks the coarse pixels whose whole footprint lies away from the border.  There
    (zr, zi, za) is exactly (dx**2 - dy**2, 2 dx dy, dx**2 + dy**2) with (dx, dy) = 32 k (a, b), the modulus of every fine pixel
    is an exact integer and d = za; the centre restatement (whose longdouble hypot is exact there) is demanded of the device
    bit for bit, G2 = (|dx|, dy sign(dx)), the principal root of grad**2, included.  Any hypot that is built from IEEE products, sums and a root of
    the scaled operands is exact on these operands: the squares and their sum fit 53 bits.  At k = 2**20 c = za / (za + 1e-5)
    = 1.0 exactly, so the interior is inside `knife` by construction (c_hi > 1 whatever hypot does to a value it may move by
    two spacings); these are the only knife-edge pixels of any case and the exact demand replaces the bracket's either-or."""
    a, b, k = RAMPS[RAMP_NAMES.index(name)]
    L, S = RAMP_SHAPE
    y, x = np.mgrid[0:L, 0:S].astype(np.float64)
    am = (a * x + b * y) * k
    br = gx.LocalBracket(am)
    dx, dy = 32.0 * k * a, 32.0 * k * b
    interior = np.zeros(br.za.shape, bool)
    interior[3:-3, 3:-3] = True
    assert interior.sum() >= 16 * 16
    triple = (dx * dx - dy * dy, 2 * dx * dy, dx * dx + dy * dy)
    assert triple[2] < 2.0 ** 53 * k * k
    for v, t in zip((br.zr, br.zi, br.za, br.d), triple + (triple[2],)):
        assert (v[interior] == t).all(), name
    g = (abs(dx), dy * np.sign(dx)) if triple[0] > 0 else (abs(dx), np.copysign(abs(dy), triple[1]))
    assert (br.re[interior] == g[0]).all() and (br.im[interior] == g[1]).all(), name
    assert (br.branch[interior] == (2 if triple[0] > 0 else 3)).all()
    if k == 1:
        no_knife_edge(br, name)
        assert (br.c[interior] < 1).all() and (br.c[interior] > 0.999999).all()
    else:
        assert (br.c[interior] == 1.0).all(), name
        assert not (br.knife & ~interior).any() and br.knife[interior].all() and not br.above.any(), name
    return frozen(am), br, frozen(interior)


# ----------------------------------------------------------------------------------------------- the raw filter entry
FILTER_CASES = ([(g, w, p, None) for g in fc.RAW_GRIDS for w in fc.SETS for p in fc.PHASES]
                + [(g, w, 1, n) for g in fc.BIG_GRIDS for w, n in fc.NAN_CASES])
NOISE_GRIDS = fc.BIG_GRIDS


def filter_id(case):
    g, w, p, n = case
    return f"{g[0]}x{g[1]}-{w}{'+' if p == 1 else '-'}" + (f"-nan_{n}" if n else "")


@functools.lru_cache(maxsize=None)
def noise_inputs(grid):
    """The designed inputs of set A with r2 = 1 + 2e-9 u: the variance of r2 under Mean's weights is about 1e-18, below the
    rounding of J1 and J * J, so d = J1 - J * J takes both signs."""
    t = {k: np.array(v) for k, v in fc.designed(grid, "A", 1).items()}
    rng = np.random.default_rng(9100 + 10 * grid[0] + grid[1])
    t["r2"] = 1 + 2e-9 * rng.uniform(-1, 1, grid)
    _J, _J1, _G4, d = gx.filter_terms(t["r2"], t["g3"])
    assert (d < 0).sum() >= 16 and (d >= 0).sum() >= 16, (grid, int((d < 0).sum()), int((d >= 0).sum()))
    return {k: frozen(v) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def inf_input():
    """Mean's input with one +inf away from the edges: B42's zero taps multiply it, so its 13 x 13 footprint is NaN (+inf on
    the four corners, which only the outermost taps reach)."""
    x = np.array(fc.mean_input((63, 65)))
    x[20, 30] = np.inf
    return frozen(x)


def filter_exact_of(t):
    return gx.filter_exact(t["r2"], t["g3"], t["c"], t["q4"])


@functools.lru_cache(maxsize=None)
def noise_want(grid):
    """The exact restatement on `noise_inputs`: NaN in f1 and F exactly where d < 0, which happens; the other filters finite."""
    t = noise_inputs(grid)
    want = filter_exact_of(t)
    d = gx.filter_terms(t["r2"], t["g3"])[3]
    assert np.array_equal(np.isnan(want[0]), d < 0) and np.array_equal(np.isnan(want[4]), d < 0) and (d < 0).any()
    assert np.isfinite(want[1:4]).all()
    return frozen(want)


def check_all():
    """Builds every case, so that each case's assertions run."""
    for name in SIGMA0_NAMES:
        for dtype in DTYPES:
            sigma0(name, dtype), local_bracket(name, dtype)
    for name in RAMP_NAMES:
        ramp(name)
    for g in NOISE_GRIDS:
        noise_want(g)
