"""TEST-SIDE restatement, in vectorised numpy, of the tables a co-pol LUT install derives on the device (csrc/xsw_lutbuild.hpp,
xsw_misc.hpp: k_pad_co, k_transpose_slices, k_mono_rows, k_tail_min, k_inv_range, k_inv_rows, k_block_minmax, k_band_minmax).

Written from what the tables MEAN (the kernels' comments), not from how the kernels walk them: no sparse-table
recurrence, no merge pointer, no tile.  float64 throughout; every function returns an array of exactly the device layout,
pad columns and slack included, so that a read-back (`Context.read_lut_table`) compares element by element, bit for bit:
everything here is comparisons, minima and maxima, one fused multiply-add and one directed cast -- there is no tolerance.

`dense` is the dB table [n_inc][n_w][n_phi] that went into the install.  tests/test_lut_tables_cpu.py holds this module to
tests/prune_model.py's loop versions and to what the kernels that READ the tables assume; tests/test_gpu_lut_tables.py holds
the device to it."""
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

INV_BINS, TAIL_LEVELS = 2048, 7
BLK_R, BLK_C, BLK_C4, CELL_R, CELL_C = 4, 16, 4, 8, 2
SLACK_ROWS, COT_SLACK = 260, 512

TABLES = ("co", "co32", "coT", "mono_rows", "tail_min", "inv_grid", "inv_rows", "blk", "blk4", "cellmm", "bandmm")
OPTIONAL = ("tail_min", "inv_grid", "inv_rows", "blk", "blk4", "cellmm", "bandmm")


def _up(a, b):
    return -(-a // b)


def geometry(n_inc, n_w, n_phi):
    """CoGeometry (csrc/xsw_lutplan.hpp) restated: pads, block / cell / band counts, element counts, gates, launch grids."""
    g = SimpleNamespace(n_inc=n_inc, n_w=n_w, n_phi=n_phi)
    g.ppad, g.wpad = _up(n_phi, 4) * 4, _up(n_w, 4) * 4
    g.nbr, g.nbc, g.nbc4 = _up(n_w, BLK_R), _up(n_phi, BLK_C), _up(n_phi, BLK_C4)
    g.ncr, g.ncc = _up(g.nbr, CELL_R), _up(g.nbc, CELL_C)
    g.blk_g = max(1, 64 // g.nbc)
    g.nbands = _up(g.nbr, g.blk_g)
    g.rows = n_inc * n_w
    g.n_body, g.n_slack = g.rows * g.ppad, SLACK_ROWS * g.ppad
    g.n_pad = g.n_body + g.n_slack
    g.tail_n = n_inc * (TAIL_LEVELS + 1) * g.ppad
    g.inv_n = n_inc * INV_BINS * g.ppad
    g.coT_n = n_inc * n_phi * g.wpad + COT_SLACK
    g.nblk, g.nblk4, g.ncell, g.nband = n_inc * g.nbr * g.nbc, n_inc * g.nbr * g.nbc4, n_inc * g.ncr * g.ncc, n_inc * g.nbands
    g.inv_ok = n_w < 65536 and n_inc < 65536 and g.inv_n * 2 < 1 << 32
    g.blk_ok, g.blk4_ok = g.nblk < 1 << 31, g.nblk4 < 1 << 31
    g.pad_grid = min((g.rows + 3) // 4, 256 * 32)  # k_pad_co: workgroups of 4 waves, one row per wave trip
    g.col_grid = _up(n_inc * n_phi, 256)           # k_mono_rows / k_inv_rows: one thread per (slice, direction)
    return g


def _geometry_of(dense):
    return geometry(*dense.shape)


# ---- co / co32 / coT
def co(dense):
    """The dense table in place in [rows + 260][ppad]; every pad column and slack row exactly 0.0.  Flat."""
    g = _geometry_of(dense)
    out = np.zeros((g.rows + SLACK_ROWS, g.ppad), np.float64)
    out[:g.rows, :g.n_phi] = dense.reshape(g.rows, g.n_phi)
    return out.reshape(-1)


def co32(dense):
    """The round-to-nearest float32 cast of `co`."""
    with np.errstate(over="ignore", invalid="ignore"):
        return co(dense).astype(np.float32)


def coT(dense):
    """[n_inc][n_phi][wpad] + 512 elements: slice i, direction p, speed row w at (i, p, w); pads and slack 0.0.  Flat."""
    g = _geometry_of(dense)
    out = np.zeros(g.coT_n, np.float64)
    body = out[:g.n_inc * g.n_phi * g.wpad].reshape(g.n_inc, g.n_phi, g.wpad)
    body[:, :, :g.n_w] = dense.transpose(0, 2, 1)
    return out


# ---- mono_rows
def mono_rows(dense):
    """int32 [n_inc]: per slice the smallest, over the directions, row that is LOWER than its predecessor; n_w when there is
    none.  Equal neighbours are not a descent."""
    n_inc, n_w, _ = dense.shape
    if n_w < 2:
        return np.full(n_inc, n_w, np.int32)
    lower = dense[:, 1:, :] < dense[:, :-1, :]                 # [i][r - 1][p]: row r is lower than row r - 1
    row_has = lower.any(axis=2)                                # some direction descends at row r
    first = np.where(row_has.any(axis=1), row_has.argmax(axis=1) + 1, n_w)
    return first.astype(np.int32)


# ---- tail_min
def tail_min(dense, mono):
    """float64 [n_inc][8][ppad].  Level 0: per direction the minimum over the rows >= mono.  Level k = 1..6: the minimum of
    level 0 over the directions p .. p + 2^k - 1, clipped to the axis.  Level 7: the minimum over all directions, in every slot.
    +inf in the pad slots of levels 0..6 and everywhere in a slice that is monotone throughout."""
    g = _geometry_of(dense)
    out = np.full((g.n_inc, TAIL_LEVELS + 1, g.ppad), np.inf)
    past = np.arange(g.n_w)[None, :, None] >= np.asarray(mono)[:, None, None]
    lvl0 = np.where(past, dense, np.inf).min(axis=1)           # [i][p]
    out[:, 0, :g.n_phi] = lvl0
    ext = np.full((g.n_inc, g.n_phi + (1 << (TAIL_LEVELS - 1))), np.inf)
    ext[:, :g.n_phi] = lvl0
    for k in range(1, TAIL_LEVELS):
        win = np.stack([ext[:, j:j + g.n_phi] for j in range(1 << k)]).min(axis=0)
        out[:, k, :g.n_phi] = win
    out[:, TAIL_LEVELS, :] = lvl0.min(axis=1)[:, None]
    return out


# ---- inv_grid / inv_rows
def inv_grid(dense, mono):
    """float64 [n_inc][3] = {t0, width, 1 / width}: t0 and t0 + 2048 width are the minimum and maximum of the slice's monotone
    rows (rows < mono).  Three zeros for a slice of no width (or one whose range is not finite)."""
    n_inc = dense.shape[0]
    out = np.zeros((n_inc, 3))
    for i in range(n_inc):
        part = dense[i, :mono[i]]
        lo, hi = float(part.min()), float(part.max())
        with np.errstate(over="ignore", invalid="ignore"):
            width = (hi - lo) / INV_BINS
        if width > 0.0 and width < 1e300 and lo > -1e300:
            out[i] = lo, width, 1.0 / width
    return out


def fma(a, b, c):
    """a * b + c rounded once: math.fma where the interpreter has it, exact rational arithmetic otherwise (float() of a
    Fraction rounds to nearest even)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return fma_exact(a, b, c)


def fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@functools.lru_cache(maxsize=4096)
def _thresholds(t0, width, bins, rounded):
    t = np.array([rounded(float(b), width, t0) for b in range(bins)])
    t.setflags(write=False)
    return t


def thresholds(t0, width, rounded=fma, bins=INV_BINS):
    """t_b = the correctly rounded b width + t0, b = 0 .. bins - 1 (t_0 is never compared: bin 0 holds row 0).  Formed once per
    grid (t0, width) and kept: every column of a slice shares them.  Read-only."""
    return _thresholds(float(t0), float(width), int(bins), rounded)


def inv_rows(dense, mono, grid, slices=None, strict=True, rounded=fma):
    """uint16 [n_inc][2048][ppad] (or [len(slices)][2048][ppad]): [b][p] = the number of rows r < mono with col[r] < t_b; bin 0
    and the pad columns zero.  The column is non-decreasing over those rows, so the count is where t_b would be inserted.
    strict=False (<=) and `rounded` (another threshold arithmetic) are the wrong tables of test_lut_tables_cpu.py."""
    g = _geometry_of(dense)
    slices = range(g.n_inc) if slices is None else list(slices)
    out = np.zeros((len(slices), INV_BINS, g.ppad), np.uint16)
    for k, i in enumerate(slices):
        t = thresholds(grid[i, 0], grid[i, 1], rounded)
        m = int(mono[i])
        for p in range(g.n_phi):
            out[k, 1:, p] = np.searchsorted(dense[i, :m, p], t[1:], side="left" if strict else "right")
    return out


def inv_rows_by_count(sl, mono, t):
    """The definition itself, for one slice: [b][p] = #{r < mono : sl[r][p] < t[b]} (bin 0: zero).  Small tables only."""
    out = (sl[:mono, None, :] < t[None, :, None]).sum(axis=0)
    out[0] = 0
    return out


# ---- block pyramid
def f32_down(x):
    """float32, rounded toward -inf; a value float32 holds exactly does not move."""
    with np.errstate(over="ignore"):
        y = np.asarray(x, np.float64).astype(np.float32)
    return np.where(y.astype(np.float64) > x, np.nextafter(y, np.float32(-np.inf)), y).astype(np.float32)


def f32_up(x):
    with np.errstate(over="ignore"):
        y = np.asarray(x, np.float64).astype(np.float32)
    return np.where(y.astype(np.float64) < x, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


def _blocks_of(a, axis, size, op):
    """op over consecutive groups of `size` entries along `axis`; the last group holds what is left."""
    n = a.shape[axis]
    whole = n // size
    lead = np.moveaxis(a, axis, -1)
    parts = [op.reduce(lead[..., :whole * size].reshape(lead.shape[:-1] + (whole, size)), axis=-1)]
    if n % size:
        parts.append(op.reduce(lead[..., whole * size:], axis=-1, keepdims=True))
    return np.moveaxis(np.concatenate(parts, axis=-1), -1, axis)


def block_minmax64(dense, rows, cols):
    """float64 (min, max) [n_inc][ceil(n_w / rows)][ceil(n_phi / cols)] of the blocks of rows x cols entries, the last ones
    clipped at the slice's last row and direction."""
    lo = _blocks_of(_blocks_of(dense, 1, rows, np.minimum), 2, cols, np.minimum)
    hi = _blocks_of(_blocks_of(dense, 1, rows, np.maximum), 2, cols, np.maximum)
    return lo, hi


def block_minmax(dense, rows, cols):
    """float32 [..][..][..][2] = {min rounded down, max rounded up}."""
    lo, hi = block_minmax64(dense, rows, cols)
    return np.stack([f32_down(lo), f32_up(hi)], axis=-1)


def blk(dense):
    return block_minmax(dense, BLK_R, BLK_C)


def blk4(dense):
    return block_minmax(dense, BLK_R, BLK_C4)


def cellmm(dense):
    return block_minmax(dense, CELL_R * BLK_R, CELL_C * BLK_C)


def bandmm(dense, blk_g=None):
    """float32 [n_inc][nbands][2]: over blk_g block rows (4 blk_g speed rows) and all directions."""
    g = _geometry_of(dense)
    return block_minmax(dense, BLK_R * (g.blk_g if blk_g is None else blk_g), g.n_phi)[:, :, 0, :]


# ---- everything, and the comparison
def all_tables(dense, inv_slices=None, bounds=True):
    """name -> array (None: the install does not build it at this shape) for every name of TABLES.  inv_slices: inv_rows of these
    slices only.  bounds=False: co / co32 / coT alone (a table with a NaN or an inf: the derived bounds are not defined here)."""
    dense = np.ascontiguousarray(dense, np.float64)
    g = _geometry_of(dense)
    t = {"co": co(dense), "co32": co32(dense), "coT": coT(dense)}
    if not bounds:
        return t
    mono = t["mono_rows"] = mono_rows(dense)
    t["tail_min"] = tail_min(dense, mono)
    t["inv_grid"] = inv_grid(dense, mono) if g.inv_ok else None
    t["inv_rows"] = inv_rows(dense, mono, t["inv_grid"], inv_slices) if g.inv_ok else None
    t["blk"] = blk(dense) if g.blk_ok else None
    t["cellmm"] = cellmm(dense) if g.blk_ok else None
    t["bandmm"] = bandmm(dense) if g.blk_ok else None
    t["blk4"] = blk4(dense) if g.blk_ok and g.blk4_ok else None
    return t


def scalars(dense):
    """{finite flag, largest finite |dB|} as the install reads them back (`prunable` also depends on the axes)."""
    fin = np.isfinite(dense)
    return float(fin.all()), float(np.abs(dense[fin]).max()) if fin.any() else 0.0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).reshape(-1)


def count_differing(got, want):
    """Elements of `got` whose BITS differ from `want` (so -0.0 is not 0.0 and a NaN equals only the same NaN); every element when
    one side is absent, or dtype or size differ; 0 when both are absent."""
    if got is None and want is None:
        return 0
    if got is None or want is None:
        return int(np.size(want if got is None else got))
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.size != want.size:
        return int(max(got.size, want.size))
    return int(np.count_nonzero(_bits(got) != _bits(want)))


def compare(got, want):
    """name -> number of differing elements, over the names of `want`."""
    return {name: count_differing(got.get(name), ref) for name, ref in want.items()}
