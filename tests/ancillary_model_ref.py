"""numpy restatement of xsarsea_amd.ancillary (include/xsw.h: xsw_ancillary_model), written from its per-pixel statement and
independent of the package: its own bracket, its own longitude continuity step, its own uniformity rule.  Vectorised, in the
kernel's operation order (every numpy operation rounds once, as every kernel operation does), so that the GPU tests can ask for
equal bits.

    core(...)                  the C entry's arguments (prepared brackets, signed dlat) -> raster
    ancillary_from_model(...)  the public call's arguments -> raster; ValueError where the public call refuses
"""
import numpy as np

TOL = 1e-3  # of a step


def bracket(ties, coords):
    """(first, t) per coordinate: the last tie point <= x and the weight of the next one, one division; at or before the first
    tie point, at or beyond the last one and for a single tie point, that tie point alone (t = 0)."""
    c, x = np.asarray(ties, dtype=np.float64), np.asarray(coords, dtype=np.float64)
    first, t = np.zeros(len(x), np.int32), np.zeros(len(x))
    for k, xv in enumerate(x):
        if len(c) == 1 or xv <= c[0]:
            continue
        if xv >= c[-1]:
            first[k] = len(c) - 1
            continue
        i = int(np.nonzero(c <= xv)[0][-1])
        first[k], t[k] = i, (xv - c[i]) / (c[i + 1] - c[i])
    return first, t


def continuous(lon):
    """lon - 360 K: K counts the whole turns between raw neighbours (round(difference / 360), halves to even), down the first
    column, then along each line."""
    lon = np.asarray(lon, dtype=np.float64)
    K = np.zeros(lon.shape)
    for i in range(lon.shape[0]):
        if i:
            K[i, 0] = K[i - 1, 0] + np.round((lon[i, 0] - lon[i - 1, 0]) / 360.0)
        for j in range(1, lon.shape[1]):
            K[i, j] = K[i, j - 1] + np.round((lon[i, j] - lon[i, j - 1]) / 360.0)
    return lon - 360.0 * K


def uniform(axis, what):
    """(first, step, n) of a uniform axis, ValueError for any other."""
    a = np.asarray(axis, dtype=np.float64)
    if a.ndim != 1 or len(a) < 2 or not np.isfinite(a).all():
        raise ValueError(f"{what}: two finite nodes or more")
    step = (a[-1] - a[0]) / (len(a) - 1)
    if step == 0 or any(abs(a[k] - (a[0] + k * step)) > TOL * abs(step) for k in range(len(a))):
        raise ValueError(f"{what} is not uniform")
    return a[0], step, len(a)


def cell(x, n, periodic):
    """(i, i1, t, inside) of coordinate x on an axis of n nodes."""
    if periodic:
        r = x - np.floor(x / float(n)) * float(n)
        r = np.where(~(r >= 0.0) | (r >= float(n)), 0.0, r)
        f = np.floor(r)
        i = np.minimum(f.astype(np.int64), n - 1)
        return i, np.where(i + 1 == n, 0, i + 1), r - f, np.ones(x.shape, bool)
    inside = (x >= 0.0) & (x <= float(n - 1))
    f = np.clip(np.floor(x), 0.0, float(n - 2))
    i = f.astype(np.int64)
    return i, i + 1, x - f, inside


def core(u, v, lon0, dlon, periodic, lat0, dlat, tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t, sample_first, sample_t, chunk=256):
    """The raster of xsw_ancillary_model: u, v [n_lat, n_lon] on lon0 + i dlon, lat0 + j dlat (dlat signed); tie_* [nl, ns]."""
    u64, v64 = np.asarray(u).astype(np.float64), np.asarray(v).astype(np.float64)
    n_lat, n_lon = u64.shape
    nl, ns = tie_lon.shape
    L, S = len(line_first), len(sample_first)
    j0 = np.clip(np.asarray(sample_first, np.int64), 0, ns - 1)
    j1 = np.minimum(j0 + 1, ns - 1)
    ws1 = np.asarray(sample_t, np.float64)[None, :]
    ws0 = 1.0 - ws1
    out = np.empty((L, S), np.complex128)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a in range(0, L, chunk):
            i0 = np.clip(np.asarray(line_first[a:a + chunk], np.int64), 0, nl - 1)
            i1 = np.minimum(i0 + 1, nl - 1)
            wl1 = np.asarray(line_t[a:a + chunk], np.float64)[:, None]
            wl0 = 1.0 - wl1

            def tie(f):
                r0 = ws0 * f[i0][:, j0] + ws1 * f[i0][:, j1]
                r1 = ws0 * f[i1][:, j0] + ws1 * f[i1][:, j1]
                return wl0 * r0 + wl1 * r1

            lon, lat, c, s = tie(tie_lon), tie(tie_lat), tie(tie_cos), tie(tie_sin)
            nh = np.hypot(c, s)
            ch, sh = c / nh, s / nh  # nh == 0: NaN
            ix, ix1, tx, in_x = cell((lon - lon0) / dlon, n_lon, periodic)
            iy, iy1, ty, in_y = cell((lat - lat0) / dlat, n_lat, False)
            wx0, wx1, wy0, wy1 = 1.0 - tx, tx, 1.0 - ty, ty
            blend = lambda g: wy0 * (wx0 * g[iy, ix] + wx1 * g[iy, ix1]) + wy1 * (wx0 * g[iy1, ix] + wx1 * g[iy1, ix1])
            uu, vv = blend(u64), blend(v64)
            re, im = -(uu * ch - vv * sh), -(uu * sh + vv * ch)
            ok = in_x & in_y
            o = out[a:a + chunk]
            o.real, o.imag = np.where(ok, re, np.nan), np.where(ok, im, np.nan)
    return out


def ancillary_from_model(u, v, model_lon, model_lat, tie_line, tie_sample, tie_lon, tie_lat, tie_heading, line, sample):
    """The public call on host arrays.  A descending latitude axis is read backwards (the flipped grid, bit for bit)."""
    u, v = np.asarray(u), np.asarray(v)
    if u.shape != v.shape or u.dtype != v.dtype or u.ndim != 2 or u.dtype not in (np.float32, np.float64):
        raise ValueError("u / v: one 2-D shape, one dtype, float32 or float64")
    tie_line, tie_sample = np.asarray(tie_line, np.float64), np.asarray(tie_sample, np.float64)
    grids = [np.asarray(g, dtype=np.float64) for g in (tie_lon, tie_lat, tie_heading)]
    for g in grids:
        if g.shape != (len(tie_line), len(tie_sample)):
            raise ValueError("tie grids must be [line, sample]")
        if np.isnan(g).any():
            raise ValueError("NaN tie value")
    line, sample = np.asarray(line, np.float64), np.asarray(sample, np.float64)
    for c, t in ((line, tie_line), (sample, tie_sample)):
        if len(c) and (c.min() < t[0] or c.max() > t[-1]):
            raise ValueError("raster coordinate outside the tie span")
    lon0, dlon, n_lon = uniform(model_lon, "model_lon")
    lat0, dlat, n_lat = uniform(model_lat, "model_lat")
    if dlon < 0 or u.shape != (n_lat, n_lon):
        raise ValueError("model axes do not fit")
    if dlat < 0:
        u, v, lat0, dlat = u[::-1], v[::-1], np.asarray(model_lat, np.float64)[-1], -dlat
    periodic = abs(n_lon * dlon - 360.0) <= TOL * abs(dlon)
    h = np.deg2rad(grids[2])
    lf, lt = bracket(tie_line, line)
    sf, st = bracket(tie_sample, sample)
    return core(u, v, lon0, dlon, periodic, lat0, dlat, continuous(grids[0]), grids[1], np.cos(h), np.sin(h), lf, lt, sf, st)


def same_bits(got, want):
    """NaN where and only where `want` has NaN (per part, payloads aside), every other part bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.complex128:
        return False
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        nan = np.isnan(w)
        if not np.array_equal(np.isnan(g), nan):
            return False
        if not np.array_equal(np.ascontiguousarray(g[~nan]).view(np.uint64), np.ascontiguousarray(w[~nan]).view(np.uint64)):
            return False
    return True
