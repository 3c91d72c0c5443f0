"""numpy restatement of xsarsea_amd.cells (include/xsw.h: xsw_wind_cells, xsw_raster_cells), written from the statement and
independent of the package.  Every numpy operation rounds once, as every kernel operation does, and the sums run in the stated
order, so that the GPU tests can ask for equal bits.

    ordered_sum(x)             the stated order on one cell's valid-or-zero values, literally (256 accumulators, then the folds)
    cell_sums(values, cell)    the same for every cell of a raster at once
    wind(w, cell, keep)        count, wind, wspd, wspd_std, steadiness per cell
    real(x, cell, keep)        count, mean, std per cell
    centres(coords, step)      the cells' centre coordinates
    geo(res, ...)              longitude, latitude, u, v at the centres: the tie-point blend in the expression order of
                               tests/ancillary_model_ref.py, then the rotation
"""
import numpy as np

from ancillary_model_ref import bracket, continuous

FOLDS = (128, 64, 32, 16, 8, 4, 2, 1)


def ordered_sum(x):
    """The sum of the statement: pixel p to accumulator p mod 256, each accumulator from +0.0 in ascending p, then
    a[i] += a[i + h] for i < h, h = 128 .. 1."""
    x = np.asarray(x, dtype=np.float64).ravel()
    rows = np.zeros((max(1, -(-len(x) // 256)), 256))
    rows.ravel()[:len(x)] = x
    a = np.zeros(256)
    for row in rows:
        a = a + row
    for h in FOLDS:
        a[:h] = a[:h] + a[h:2 * h]
    return a[0]


def _sum_rows(v):
    """`ordered_sum` of every row of v [cells, N].  Rows are padded with +0.0 to P = 256 (N > 256: to a multiple of it), or for
    N <= 128 only to the next power of two: an accumulator is never -0.0 (it starts at +0.0, and +0.0 + -0.0 = +0.0), so the
    folds that would add nothing but padding, a[i] + 0.0, change no bit and are left out (test_cells_cpu.py holds this form
    to the literal one)."""
    ncell, N = v.shape
    P = 256
    while P // 2 >= max(N, 1):
        P //= 2
    trips = max(1, -(-N // P))
    out = np.empty(ncell)
    step = max(1, (1 << 22) // (trips * P))
    for a0 in range(0, ncell, step):
        rows = np.zeros((min(step, ncell - a0), trips * P))
        rows[:, :N] = v[a0:a0 + step]
        rows = rows.reshape(len(rows), trips, P)
        a = np.zeros((len(rows), P))
        for k in range(trips):
            a = a + rows[:, k]
        h = P // 2
        while h >= 1:
            a = a[:, :h] + a[:, h:2 * h]
            h //= 2
        out[a0:a0 + step] = a[:, 0]
    return out


def _groups(n, step):
    """(first pixel, last pixel + 1, cells, cell extent) of the full cells of an axis and of its clipped last one."""
    full = n // step
    g = [(0, full * step, full, step)] if full else []
    if n % step:
        g.append((full * step, n, 1, n % step))
    return g


def cell_sums(values, cell):
    """[nLc, nSc] ordered sums of a float64 raster of valid-or-zero values; a cell's pixels in the order p = r * w + c."""
    values = np.asarray(values, dtype=np.float64)
    L, S = values.shape
    cl, cs = cell
    out = np.empty((-(-L // cl), -(-S // cs)))
    i = 0
    for r0, r1, nr, h in _groups(L, cl):
        j = 0
        for c0, c1, nc, w in _groups(S, cs):
            block = values[r0:r1, c0:c1].reshape(nr, h, nc, w).transpose(0, 2, 1, 3).reshape(nr * nc, h * w)
            out[i:i + nr, j:j + nc] = _sum_rows(block).reshape(nr, nc)
            j += nc
        i += nr
    return out


def _scatter(sq, s, nd):
    with np.errstate(invalid="ignore", divide="ignore"):
        var = (sq - (s * s) / nd) / (nd - 1.0)
        return np.where(nd < 2, np.nan, np.sqrt(np.where(var < 0, 0.0, var)))


def _valid(ok, keep):
    return ok if keep is None else ok & (np.asarray(keep).astype(np.uint8) != 0)


def wind(w, cell, keep=None):
    """dict(count, wind, wspd, wspd_std, steadiness) of a complex raster (complex64: widened first)."""
    w = np.asarray(w)
    re, im = w.real.astype(np.float64), w.imag.astype(np.float64)
    ok = _valid(~np.isnan(re) & ~np.isnan(im), keep)
    with np.errstate(invalid="ignore", over="ignore"):
        q = re * re + im * im
        s = np.sqrt(q)
    z = lambda a: cell_sums(np.where(ok, a, 0.0), cell)
    n = cell_sums(ok.astype(np.float64), cell)  # whole numbers below 2**53: exact in any order
    s_re, s_im, s_s, s_q = z(re), z(im), z(s), z(q)
    with np.errstate(invalid="ignore", divide="ignore"):
        mre, mim, wspd = s_re / n, s_im / n, s_s / n
        steadiness = np.sqrt(mre * mre + mim * mim) / wspd
    out = np.empty(n.shape, np.complex128)
    out.real, out.imag = mre, mim
    return dict(count=n.astype(np.int32), wind=out, wspd=wspd, wspd_std=_scatter(s_q, s_s, n), steadiness=steadiness)


def real(x, cell, keep=None):
    """dict(count, mean, std) of a float32 / float64 raster (widened first)."""
    x = np.asarray(x).astype(np.float64)
    ok = _valid(~np.isnan(x), keep)
    with np.errstate(invalid="ignore", over="ignore"):
        xx = x * x
    n = cell_sums(ok.astype(np.float64), cell)
    s_x, s_xx = cell_sums(np.where(ok, x, 0.0), cell), cell_sums(np.where(ok, xx, 0.0), cell)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s_x / n
    return dict(count=n.astype(np.int32), mean=mean, std=_scatter(s_xx, s_x, n))


def centres(coords, step):
    c = np.asarray(coords, dtype=np.float64)
    first = np.arange(0, len(c), step)
    last = np.minimum(first + step, len(c)) - 1
    return (c[first] + c[last]) / 2


def geo_core(mean_wind, tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t, sample_first, sample_t):
    """dict(longitude, latitude, u, v) from the entry's own arguments: continuous tie longitudes, cosine / sine tables, prepared
    brackets of the centres."""
    nl, ns = tie_lon.shape
    i0 = np.clip(np.asarray(line_first, np.int64), 0, nl - 1)
    i1 = np.minimum(i0 + 1, nl - 1)
    j0 = np.clip(np.asarray(sample_first, np.int64), 0, ns - 1)
    j1 = np.minimum(j0 + 1, ns - 1)
    ws1 = np.asarray(sample_t, np.float64)[None, :]
    ws0 = 1.0 - ws1
    wl1 = np.asarray(line_t, np.float64)[:, None]
    wl0 = 1.0 - wl1

    def tie(f):
        r0 = ws0 * f[i0][:, j0] + ws1 * f[i0][:, j1]
        r1 = ws0 * f[i1][:, j0] + ws1 * f[i1][:, j1]
        return wl0 * r0 + wl1 * r1

    lon, lat, c, s = tie(tie_lon), tie(tie_lat), tie(tie_cos), tie(tie_sin)
    mre, mim = mean_wind.real, mean_wind.imag
    with np.errstate(invalid="ignore", divide="ignore"):
        nh = np.hypot(c, s)
        ch, sh = c / nh, s / nh  # nh == 0: NaN
        u, v = -(mre * ch + mim * sh), -(mim * ch - mre * sh)
    return dict(longitude=lon, latitude=lat, u=u, v=v)


def geo(mean_wind, tie_line, tie_sample, tie_lon, tie_lat, tie_heading, cline, csample):
    """The same from the public call's arguments: raw tie longitudes (made continuous here), headings in degrees."""
    h = np.deg2rad(np.asarray(tie_heading, dtype=np.float64))
    lf, lt = bracket(tie_line, cline)
    sf, st = bracket(tie_sample, csample)
    return geo_core(mean_wind, continuous(tie_lon), np.asarray(tie_lat, dtype=np.float64), np.cos(h), np.sin(h), lf, lt, sf, st)


def same_bits(got, want):
    """NaN where and only where `want` has NaN (per part, payloads aside), every other value bit for bit; integers equal."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind in "iub":
        return np.array_equal(got, want)
    parts = ((got.real, want.real), (got.imag, want.imag)) if got.dtype.kind == "c" else ((got, want),)
    for g, w in parts:
        g, w = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        nan = np.isnan(w)
        if not np.array_equal(np.isnan(g), nan) or not np.array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64)):
            return False
    return True
