"""CPU: the restatement of a LUT install's device-built tables (tests/lut_tables_ref.py) and the tables it is evaluated on
(tests/lut_table_shapes.py), before tests/test_gpu_lut_tables.py holds the device to them.

- every entry of lut_table_shapes.SHAPES reaches the edge it is there for (from the geometry, itself held to
  test_host_lutplan.p_geometry, which the compiled header answers to), and the content holds the classes its docstring lists;
- (a) the restatement equals tests/prune_model.py's loop versions on every small table;
- (b) the restatement gives what the kernels that READ the tables assume (band_wave's sparse-table query, the bins of stage 1,
  bounds that enclose, coarser levels that enclose finer ones);
- (c) the comparison the GPU test uses reports every wrong table of WRONG_TABLES."""
import math

import numpy as np
import pytest

import lut_table_shapes as ls
import lut_tables_ref as ref
import prune_model as pm
from test_host_lutplan import p_geometry

SMALL = ("one_block", "default_phi", "wide_phi", "band_per_row")  # loop versions and brute force stay quick on these


@pytest.fixture(scope="module")
def tables():
    """key -> the restatement's tables of ls.table(key); built once, never written to."""
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = ref.all_tables(ls.table(key))
            for a in cache[key].values():
                if a is not None:
                    a.setflags(write=False)
        return cache[key]

    return get


# ------------------------------------------------------------------------------------------------ shapes and content
def test_geometry_restatement_and_binding_sizes():
    """ref.geometry == the expressions test_host_lutplan holds the compiled CoGeometry to; _lib.co_table_layouts (the sizes the
    read-back is asked with) follows from it."""
    from xsarsea_amd import _lib
    for shape in list(ls.SHAPES.values()) + [(501, 499, 181), (1, 1, 1), (65536, 2, 4), (3, 70000, 2)]:
        g = ref.geometry(*shape)
        assert [g.ppad, g.wpad, g.nbr, g.nbc, g.nbc4, g.ncr, g.ncc, g.blk_g, g.nbands, g.rows * g.n_phi, g.n_body, g.n_slack, g.n_pad, g.tail_n,
                g.inv_n, 3 * g.n_inc, g.coT_n, g.rows, g.nblk, g.nband, g.ncell, g.nblk4, int(g.inv_ok), int(g.blk_ok), int(g.blk4_ok), g.pad_grid,
                g.col_grid] == p_geometry(*shape)[:27], shape
        want = {"co": g.n_pad, "co32": g.n_pad, "coT": g.coT_n, "mono_rows": g.n_inc, "tail_min": g.tail_n, "inv_grid": 3 * g.n_inc,
                "inv_rows": g.inv_n, "blk": 2 * g.nblk, "blk4": 2 * g.nblk4, "cellmm": 2 * g.ncell, "bandmm": 2 * g.nband, "scalars": 3}
        lay = _lib.co_table_layouts(*shape)
        assert {k: int(np.prod(s)) for k, (_i, _d, s) in lay.items()} == want, shape
        assert sorted(i for i, _d, _s in lay.values()) == list(range(12))
    small = {k: _lib.co_table_layouts(*ls.SHAPES["one_block"])[k] for k in ref.TABLES}
    full = ref.all_tables(ls.table("one_block"))
    assert all(full[k].dtype == d and full[k].shape == s for k, (_i, d, s) in small.items())


def test_each_shape_reaches_its_edge():
    G = {k: ref.geometry(*s) for k, s in ls.SHAPES.items()}
    g = G["one_block"]
    assert (g.nbc, g.ncr, g.ncc, g.nbands) == (1, 1, 1, 1) and g.n_w <= 32 and g.n_phi <= 32 and g.ppad <= 64
    assert g.ppad == 8 > g.n_phi and g.nbr == 3 and g.n_w == 2 * ref.BLK_R + 1
    g = G["default_phi"]
    assert g.n_phi == 181 and g.ppad == 184
    assert g.n_phi - (g.nbc - 1) * ref.BLK_C == 5 and g.n_phi - (g.nbc4 - 1) * ref.BLK_C4 == 1
    assert (g.nbc, g.blk_g, g.nbands) == (12, 5, 2) and g.nbr % g.blk_g != 0 and g.ncr == 2 and g.n_w % (ref.CELL_R * ref.BLK_R) != 0
    assert g.n_phi > 128 and -(-g.ppad // 64) == 3
    g = G["wide_phi"]
    assert g.n_phi > 256 and g.ppad == g.n_phi
    assert (-(-g.n_phi // 32), -(-g.n_w // 32)) == (10, 3) and g.n_phi % 32 and g.n_w % 32
    g = G["band_per_row"]
    assert g.nbc == 65 > 64 and g.blk_g == 1 and g.nbands == g.nbr > 1 and g.n_inc == 1
    g = G["many_rows"]
    assert g.pad_grid == 8192 and g.rows == 35000 > g.pad_grid * 4
    assert g.col_grid == 2 and (g.n_inc * g.n_phi) % 256 != 0
    g = G["no_inverse"]
    assert g.inv_n * 2 == 1 << 32 and not g.inv_ok and g.blk_ok and g.blk4_ok
    assert all(x.inv_ok and x.blk_ok and x.blk4_ok for k, x in G.items() if k != "no_inverse")
    # the install order puts a smaller table after a larger one and a larger one after a smaller one, and visits every shape
    sizes = [G[k].n_pad for k in ls.INSTALL_ORDER]
    steps = np.sign(np.diff(sizes))
    assert set(ls.INSTALL_ORDER) == set(ls.SHAPES) and (steps < 0).any() and (steps > 0).any()
    assert any(a < 0 < b for a, b in zip(steps, steps[1:])) and any(a > 0 > b for a, b in zip(steps, steps[1:]))


@pytest.mark.parametrize("key", list(ls.SHAPES))
def test_content_classes(key, tables):
    """The classes of lut_table_shapes' docstring, read off the restatement's tables."""
    dense, t = ls.table(key), tables(key)
    n_inc, n_w, n_phi = dense.shape
    assert np.isfinite(dense).all() and (dense > 0).any() and (dense < 0).any()
    kinds = [ls.kind(key, i) for i in range(n_inc)]
    mono = t["mono_rows"]
    for i, what in enumerate(kinds):
        sl = dense[i]
        lower = sl[1:] < sl[:-1]
        if what in ("mono", "flat"):
            assert mono[i] == n_w and not lower.any() and np.isinf(t["tail_min"][i]).all()
        else:
            m = 1 if what == "mono1" else ls.descent_row(n_w, i)
            first = np.where(lower.any(axis=0), lower.argmax(axis=0) + 1, n_w)
            p1 = ls.descent_phi(n_phi, i)
            assert mono[i] == m and first[p1] == m and (np.delete(first, p1) > m).all() and p1 != 0
            assert first[0] > m or n_phi == 1, "direction 0 alone would give another mono_rows"
            assert np.isfinite(t["tail_min"][i, 0, :n_phi]).all()
            if n_w > 2:
                assert (sl[1:] == sl[:-1]).any(), "equal neighbours along the speed axis"
        if what == "flat":
            assert (sl == sl[0, 0]).all()
            if t["inv_grid"] is not None:
                assert not t["inv_grid"][i].any()
        elif t["inv_grid"] is not None:
            assert t["inv_grid"][i, 1] > 0
    sat = [m for m, what in zip(mono, kinds) if what == "sat"]
    assert len(sat) < 2 or n_w < 4 or len(set(sat)) > 1, "mono_rows differs between the saturating slices"
    exact32 = dense.astype(np.float32).astype(np.float64) == dense
    assert exact32[:, :, 0].all() and exact32.all(axis=(0, 1)).sum() < n_phi  # whole directions of float32 values beside others
    if n_phi > 1:
        assert not exact32[:, :, 1].all()
    # the planted entries: one equal to its threshold exactly; one at a bin where the unfused threshold is another double
    pl = ls.plants(key)
    assert ("exact" in pl) == (key != "no_inverse") and ("unfused" in pl) == (key != "no_inverse")
    for name, p in pl.items():
        t0, width, _ = t["inv_grid"][p.slice]
        tf, tu = ref.fma_exact(float(p.bin), width, t0), ls.unfused(p.bin, width, t0)
        assert 1 <= p.row < mono[p.slice] - 1 and 1 <= p.bin < ref.INV_BINS
        assert dense[p.slice, p.row, p.phi] == min(tf, tu) and (tf != tu) == (name == "unfused")


def test_every_class_is_somewhere():
    kinds = {ls.kind(k, i) for k, s in ls.SHAPES.items() for i in range(s[0])}
    assert kinds == {"sat", "mono", "mono1", "flat"}


def test_fused_threshold_arithmetic():
    """fma_exact is a * b + c rounded once: exact cases, a case where rounding twice gives another double, and math.fma on a
    sample wherever the interpreter has one."""
    assert ref.fma_exact(3.0, 0.5, 0.25) == 1.75
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0  # a * b = 1 + 2^-29 + 2^-60: the product's rounding loses the last term
    assert ref.fma_exact(a, b, c) == 2.0 ** -29 + 2.0 ** -60 != a * b + c
    rng = np.random.default_rng(5)
    n_diff = 0
    for _ in range(2000):
        b, w, t0 = float(rng.integers(1, 2048)), float(rng.uniform(1e-3, 0.1)), float(rng.uniform(-30, 5))
        f = ref.fma_exact(b, w, t0)
        n_diff += f != b * w + t0
        assert abs(f - (b * w + t0)) <= max(math.ulp(b * w), math.ulp(f))  # the product's own rounding, seen through the sum's
        if hasattr(math, "fma"):
            assert f == math.fma(b, w, t0)
    assert n_diff > 0
    assert ref.fma(1023.0, 0.0123, -7.5) == ref.fma_exact(1023.0, 0.0123, -7.5)


# ------------------------------------------------------------------------------------------------ (a) the loop versions
@pytest.mark.parametrize("key", SMALL)
def test_restatement_equals_prune_model(key, tables):
    dense, t = ls.table(key), tables(key)
    g = ref.geometry(*dense.shape)
    for i in range(g.n_inc):
        sl = dense[i]
        mono = pm.mono_rows(sl)
        assert t["mono_rows"][i] == mono
        assert t["tail_min"][i, ref.TAIL_LEVELS, 0] == pm.tail_min(sl, mono)
        for p in range(g.n_phi):
            assert t["tail_min"][i, 0, p] == pm.tail_min(sl, mono, p, p)
        t0, width, _ = t["inv_grid"][i]
        every = range(g.n_phi) if g.n_phi <= 300 else range(0, g.n_phi, 7)  # the loop version, 2048 bins a direction; all of them by count below
        for p in sorted(set(every) | {g.n_phi - 1} | {pl.phi for pl in ls.plants(key).values() if pl.slice == i}):
            assert np.array_equal(t["inv_rows"][i, :, p], pm.inverse_rows(sl[:, p], mono, t0, width, ref.INV_BINS)), (i, p)
        thr = ref.thresholds(t0, width)
        assert np.array_equal(t["inv_rows"][i, :, :g.n_phi], ref.inv_rows_by_count(sl, mono, thr))
        lo, hi = pm.block_tables(sl)
        assert np.array_equal(t["blk"][i, :, :, 0], lo) and np.array_equal(t["blk"][i, :, :, 1], hi)
        lo4, hi4 = pm.subblock_tables(sl)
        assert np.array_equal(t["blk4"][i, :, :, 0], lo4) and np.array_equal(t["blk4"][i, :, :, 1], hi4)
        clo, chi = pm.cell_tables(lo, hi)
        assert np.array_equal(t["cellmm"][i, :, :, 0], clo) and np.array_equal(t["cellmm"][i, :, :, 1], chi)
        blo, bhi = pm.band_tables(lo, hi, g.n_phi)
        assert pm.band_rows(g.n_phi) == g.blk_g
        assert np.array_equal(t["bandmm"][i, :, 0], blo) and np.array_equal(t["bandmm"][i, :, 1], bhi)


def test_directed_casts():
    x = np.array([0.1, -0.1, 0.25, -7.25, 1e-50, -1e-50, 3.0e38, -3.0e38, 0.0])
    dn, up = ref.f32_down(x), ref.f32_up(x)
    assert dn.dtype == up.dtype == np.float32
    for k, v in enumerate(x):
        assert dn[k] == pm.f32_down(v) and up[k] == pm.f32_up(v)
        assert float(dn[k]) <= v <= float(up[k])
        assert (dn[k] == up[k]) == (float(np.float32(v)) == v), "a value float32 holds exactly does not move; another does"


# ------------------------------------------------------------------------------------------------ (b) what the readers assume
def tail_query(tm, ip_lo, ip_hi):
    """band_wave's query of one slice's sparse table tm[8][ppad]."""
    n = ip_hi - ip_lo + 1
    if n >= 128:
        return tm[ref.TAIL_LEVELS, ip_lo]
    k = min(int(math.floor(math.log2(n))), ref.TAIL_LEVELS)
    return min(tm[k, ip_lo], tm[k, ip_hi - (1 << k) + 1])


@pytest.mark.parametrize("key", SMALL)
def test_tail_query_is_the_window_minimum(key, tables):
    dense, t = ls.table(key), tables(key)
    n_phi = dense.shape[2]
    # every window [lo, hi] of the slice; at 1030 directions (half a million windows) every 13th lo and the ones where a length class ends
    los = range(n_phi) if n_phi <= 300 else sorted(set(range(0, n_phi, 13)) | {n_phi - 1, n_phi - 2, n_phi - 64, n_phi - 127, n_phi - 128})
    for i in range(dense.shape[0]):
        mono, tm = t["mono_rows"][i], t["tail_min"][i]
        lvl0 = dense[i, mono:].min(axis=0) if mono < dense.shape[1] else np.full(n_phi, np.inf)
        for lo in los:
            run = np.minimum.accumulate(lvl0[lo:])  # run[n - 1] = the brute-force minimum of [lo, lo + n - 1]
            for hi in range(lo, n_phi):
                q = tail_query(tm, lo, hi)
                assert (q == run[hi - lo]) if hi - lo + 1 < 128 else (q <= run[hi - lo]), (i, lo, hi)
        assert tm[ref.TAIL_LEVELS].min() == tm[ref.TAIL_LEVELS].max() == lvl0.min()


@pytest.mark.parametrize("key", SMALL)
def test_inverse_rows_split_the_column(key, tables):
    """For every bin b: rows >= inv[b] of the monotone part are >= t_b, rows below are < t_b."""
    dense, t = ls.table(key), tables(key)
    n_phi = dense.shape[2]
    for i in range(dense.shape[0]):
        mono = int(t["mono_rows"][i])
        thr = ref.thresholds(*t["inv_grid"][i, :2])
        inv = t["inv_rows"][i].astype(np.int64)
        assert not inv[:, n_phi:].any() and not inv[0].any() and inv.max() <= mono
        assert (np.diff(inv, axis=0) >= 0).all()
        r = np.arange(mono)[:, None, None]
        at_or_above = r >= inv[None, 1:, :n_phi]
        vals = dense[i, :mono, None, :]
        assert (vals >= thr[None, 1:, None])[at_or_above].all() and (vals < thr[None, 1:, None])[~at_or_above].all()
        assert thr[0] == dense[i, :mono].min() and t["inv_grid"][i, 1] == (dense[i, :mono].max() - thr[0]) / ref.INV_BINS
        assert t["inv_grid"][i, 2] == 1.0 / t["inv_grid"][i, 1]


@pytest.mark.parametrize("key", SMALL + ("many_rows",))
def test_bounds_enclose(key, tables):
    """Every block, sub-block, cell and band bound encloses its entries; each coarser level encloses the finer one."""
    dense, t = ls.table(key), tables(key)
    g = ref.geometry(*dense.shape)

    def spread(tab, rows, cols):  # the table's {min, max} at every entry of the block it covers
        return np.repeat(np.repeat(tab, rows, axis=1), cols, axis=2)[:, :g.n_w, :g.n_phi].astype(np.float64)

    levels = {"blk4": (ref.BLK_R, ref.BLK_C4), "blk": (ref.BLK_R, ref.BLK_C), "cellmm": (ref.CELL_R * ref.BLK_R, ref.CELL_C * ref.BLK_C),
              "bandmm": (g.blk_g * ref.BLK_R, g.n_phi)}
    at = {}
    for name, (rows, cols) in levels.items():
        tab = t[name] if name != "bandmm" else t[name][:, :, None, :]
        at[name] = spread(tab, rows, cols)
        assert (at[name][..., 0] <= dense).all() and (dense <= at[name][..., 1]).all(), name
        assert (dense - at[name][..., 0]).min() < 1e-5 and (at[name][..., 1] - dense).min() < 1e-5, name  # and is no looser than a float32 step
    for fine, coarse in (("blk4", "blk"), ("blk", "cellmm"), ("blk", "bandmm")):
        assert (at[coarse][..., 0] <= at[fine][..., 0]).all() and (at[fine][..., 1] <= at[coarse][..., 1]).all(), (fine, coarse)


# ------------------------------------------------------------------------------------------------ (c) the comparison is not vacuous
def _edge_blocks(dense, rows, cols, d_rows=0, d_cols=0):
    """block_minmax whose LAST block row / column takes in d_rows rows / d_cols columns more (+1) or fewer (-1) than the slice has:
    the extra column is what follows in memory (the next row's first entry), the extra row the next slice's first."""
    n_inc, n_w, n_phi = dense.shape
    out = ref.block_minmax(dense, rows, cols).copy()
    flat = np.concatenate([dense.reshape(-1), dense.reshape(-1)[:n_phi + 1]])
    if d_cols:
        c0 = (out.shape[2] - 1) * cols
        idx = (np.arange(n_inc * n_w) * n_phi)[:, None] + np.arange(c0, n_phi + d_cols)[None, :]
        strip = flat[idx].reshape(n_inc, n_w, -1)
        out[:, :, -1, :] = ref.block_minmax(strip, rows, n_phi)[:, :, 0, :] if strip.shape[2] else (np.inf, -np.inf)
    if d_rows:
        r0 = (out.shape[1] - 1) * rows
        ext = np.concatenate([dense, np.concatenate([dense[1:, :1], dense[:1, :1]])], axis=1)  # row n_w = the next slice's row 0
        strip = ext[:, r0:n_w + d_rows]
        out[:, -1, :, :] = ref.block_minmax(strip, n_w + 1, cols)[:, 0, :, :] if strip.shape[1] else (np.inf, -np.inf)
    return out


def _tail_levels_from(t, half_of):
    """tail_min rebuilt level by level as a sparse table whose level k joins the neighbour at p + half_of(k)."""
    out = t.copy()
    ppad = t.shape[2]
    for k in range(1, ref.TAIL_LEVELS):
        h = half_of(k)
        shifted = np.full_like(out[:, k - 1], np.inf)
        if h < ppad:
            shifted[:, :ppad - h] = out[:, k - 1, h:]
        out[:, k] = np.minimum(out[:, k - 1], shifted)
    return out


def _swap_in_ragged_tile(dense, coT):
    """coT whose last (ragged) 32 x 32 tile was written with w and p exchanged."""
    g = ref.geometry(*dense.shape)
    out = coT.copy()
    body = out[:g.n_inc * g.n_phi * g.wpad].reshape(g.n_inc, g.n_phi, g.wpad)
    w0, p0 = (g.n_w - 1) // 32 * 32, (g.n_phi - 1) // 32 * 32
    n = min(g.n_w - w0, g.n_phi - p0)
    body[:, p0:p0 + n, w0:w0 + n] = dense[:, w0:w0 + n, p0:p0 + n]
    return out


def _set(a, index, value):
    out = a.copy()
    out[index] = value
    return out


def _trim(a, n):
    """The first n bands of a band table built with another blk_g, repeated last band where it has fewer."""
    return a[:, :n] if a.shape[1] >= n else np.concatenate([a, np.repeat(a[:, -1:], n - a.shape[1], axis=1)], axis=1)


# name -> (the table it spoils, the shapes that must catch it, how).  d = the dense table, t = the restatement's tables, g = geometry.
WRONG_TABLES = {
    "blk min to nearest": ("blk", ("one_block", "default_phi"),
                           lambda d, t, g: np.stack([ref.block_minmax64(d, 4, 16)[0].astype(np.float32), t["blk"][..., 1]], axis=-1)),
    "blk last column +1": ("blk", ("default_phi", "wide_phi"), lambda d, t, g: _edge_blocks(d, 4, 16, d_cols=1)),
    "blk last column -1": ("blk", ("default_phi", "wide_phi"), lambda d, t, g: _edge_blocks(d, 4, 16, d_cols=-1)),
    "blk last row +1": ("blk", ("one_block", "default_phi"), lambda d, t, g: _edge_blocks(d, 4, 16, d_rows=1)),
    "blk last row -1": ("blk", ("one_block", "default_phi"), lambda d, t, g: _edge_blocks(d, 4, 16, d_rows=-1)),
    "blk4 last column +1": ("blk4", ("default_phi", "one_block"), lambda d, t, g: _edge_blocks(d, 4, 4, d_cols=1)),
    "blk4 last column -1": ("blk4", ("default_phi", "one_block"), lambda d, t, g: _edge_blocks(d, 4, 4, d_cols=-1)),
    "blk4 last row +1": ("blk4", ("one_block", "default_phi"), lambda d, t, g: _edge_blocks(d, 4, 4, d_rows=1)),
    "blk4 last row -1": ("blk4", ("one_block", "default_phi"), lambda d, t, g: _edge_blocks(d, 4, 4, d_rows=-1)),
    "cell last column +1": ("cellmm", ("default_phi", "wide_phi"), lambda d, t, g: _edge_blocks(d, 32, 32, d_cols=1)),
    "cell last column -1": ("cellmm", ("default_phi", "wide_phi"), lambda d, t, g: _edge_blocks(d, 32, 32, d_cols=-1)),
    "cell last row +1": ("cellmm", ("default_phi", "wide_phi"), lambda d, t, g: _edge_blocks(d, 32, 32, d_rows=1)),
    "cell last row -1": ("cellmm", ("default_phi", "wide_phi"), lambda d, t, g: _edge_blocks(d, 32, 32, d_rows=-1)),
    "tail level k from p + 2^k": ("tail_min", ("one_block", "default_phi", "wide_phi"), lambda d, t, g: _tail_levels_from(t["tail_min"], lambda k: 1 << k)),
    "tail level 7 = level 6": ("tail_min", ("default_phi", "wide_phi"), lambda d, t, g: _set(t["tail_min"], (slice(None), 7), t["tail_min"][:, 6])),
    "tail pad slot finite": ("tail_min", ("one_block", "default_phi"), lambda d, t, g: _set(t["tail_min"], (0, 1, g.n_phi), t["tail_min"][0, 1, g.n_phi - 1])),
    "mono_rows + 1": ("mono_rows", ("one_block", "many_rows"), lambda d, t, g: np.minimum(t["mono_rows"] + 1, g.n_w).astype(np.int32)),
    "mono_rows - 1": ("mono_rows", ("one_block", "many_rows"), lambda d, t, g: (t["mono_rows"] - 1).astype(np.int32)),
    "mono_rows of direction 0": ("mono_rows", ("one_block", "default_phi", "many_rows"), lambda d, t, g: ref.mono_rows(d[:, :, :1])),
    "inv_rows with <=": ("inv_rows", ("one_block", "default_phi", "wide_phi", "band_per_row", "many_rows"),
                         lambda d, t, g: ref.inv_rows(d, t["mono_rows"], t["inv_grid"], strict=False)),
    "inv_rows unfused": ("inv_rows", SMALL + ("many_rows",), lambda d, t, g: ref.inv_rows(d, t["mono_rows"], t["inv_grid"], rounded=ls.unfused)),
    "inv_rows bin 0": ("inv_rows", ("one_block",), lambda d, t, g: _set(t["inv_rows"], (slice(None), 0, slice(0, g.n_phi)), 1)),
    "co pad column": ("co", ("one_block", "default_phi"), lambda d, t, g: _set(t["co"], g.ppad * 3 + g.n_phi, 1.0)),
    "co slack": ("co", ("one_block", "wide_phi"), lambda d, t, g: _set(t["co"], g.n_pad - 1, 1.0)),
    "co32 pad column": ("co32", ("one_block", "default_phi"), lambda d, t, g: _set(t["co32"], g.ppad * 3 + g.n_phi, 1.0)),
    "co32 slack": ("co32", ("one_block", "wide_phi"), lambda d, t, g: _set(t["co32"], g.n_body, -0.0)),
    "coT pad column": ("coT", ("one_block", "default_phi", "wide_phi"), lambda d, t, g: _set(t["coT"], g.n_w, 1.0)),
    "coT slack": ("coT", ("one_block", "wide_phi"), lambda d, t, g: _set(t["coT"], g.coT_n - 1, 1.0)),
    "coT ragged tile exchanged": ("coT", ("one_block", "wide_phi"), lambda d, t, g: _swap_in_ragged_tile(d, t["coT"])),
    "bandmm over blk_g + 1": ("bandmm", ("default_phi", "band_per_row"), lambda d, t, g: _trim(ref.bandmm(d, g.blk_g + 1), g.nbands)),
    "bandmm over blk_g - 1": ("bandmm", ("default_phi",), lambda d, t, g: _trim(ref.bandmm(d, g.blk_g - 1), g.nbands)),
    "absent table as zeros": ("inv_rows", ("no_inverse",), lambda d, t, g: np.zeros((g.n_inc, ref.INV_BINS, g.ppad), np.uint16)),
    "table missing": ("blk4", ("one_block",), lambda d, t, g: None),
}


@pytest.mark.parametrize("name", list(WRONG_TABLES))
def test_comparison_reports_each_wrong_table(name, tables):
    """Each wrong table of WRONG_TABLES, put in place of the device's read-back, is reported by ref.compare -- on the shapes named
    beside it -- in its own table and in no other.  Which shape catches which:
      one_block     to-nearest block minimum; a last block row (9 = 2 x 4 + 1 rows) or sub-block column (5 = 4 + 1) one too many or too
                    few; a finite tail pad slot (phi_pad 8 > 5); a sparse-table level from the wrong neighbour; mono_rows off by one or
                    from direction 0; <= and unfused thresholds (planted entries); bin 0; pad and slack of co / co32 / coT; the ragged
                    9 x 5 tile exchanged
      default_phi   the last block (5 wide), sub-block (1 wide) and cell column and row (33 = 32 + 1 rows); level 7 = level 6 (181 >
                    64 directions); bandmm over 4 or 6 instead of 5 block rows; the pad columns of phi_pad 184
      wide_phi      the same block and cell edges at 300 directions; the second trip's slots of the tail levels; the ragged tile (70 x 300)
      band_per_row  bandmm over 2 block rows instead of 1; thresholds
      many_rows     mono_rows off by one or from direction 0 in 70 slices; <= and unfused thresholds
      no_inverse    an absent inv_rows reported as zeros"""
    which, keys, make = WRONG_TABLES[name]
    for key in keys:
        dense, t = ls.table(key), tables(key)
        got = dict(t)
        got[which] = make(dense, t, ref.geometry(*dense.shape))
        report = ref.compare(got, t)
        assert report[which] > 0, (name, key)
        assert not any(n for k, n in report.items() if k != which), (name, key)


def test_comparison_passes_the_tables_themselves(tables):
    for key in ("one_block", "no_inverse"):
        t = tables(key)
        assert set(ref.compare({k: (None if a is None else a.copy()) for k, a in t.items()}, t).values()) == {0}
    assert ref.count_differing(np.array([0.0]), np.array([-0.0])) == 1
    assert ref.count_differing(np.array([np.nan]), np.array([np.nan])) == 0
    assert ref.count_differing(np.zeros(3, np.float32), np.zeros(3)) == 3


def test_scalars_of_a_table_that_is_not_finite():
    d = ls.table("one_block").copy()
    big = float(np.abs(d).max())
    for bad in (np.nan, np.inf):
        e = d.copy()
        e[1, 4, 2] = bad
        assert ref.scalars(e) == (0.0, float(np.abs(np.delete(e.ravel(), (1 * 9 + 4) * 5 + 2)).max()))
    assert ref.scalars(d) == (1.0, big)
