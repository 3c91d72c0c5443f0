"""numpy restatement of xsarsea_amd.polar (include/xsw.h: xsw_wind_polar), written from the statement and independent of the
package, on the geolocation, the pixel terms and the brackets of tests/grid_ref.py.  Every numpy operation rounds once, as every
kernel operation does; the sums are int64 (`np.add.at`, `np.maximum.at`), which have no order, so that the GPU tests can ask
for equal bits.

    tables(lat_c, n_theta)     what the caller of the entry supplies: cos, sin of the centre's latitude and the sector borders
    chart(lon, lat, ...)       step 3: x (east), y (north) in km
    ring_sector(x, y, ...)     steps 4-5: (inside, r, kr, sector)
    sums_core(...)             the entry's own arguments -> int64 [6, n_r, n_theta]
    sums(...)                  the public call's arguments -> the same
    merge(a, b)                planes 0-4 added, plane 5 the maximum
    finish(sums)               dict(count, wspd, wspd_std, vr, vt, vmax)
"""
import numpy as np

import grid_ref as gref
from grid_ref import Q16, Q24, bracket, continuous, quantise, same_bits  # noqa: F401  (what the tests use)

R_KM = 6371.0088
D2R = 0.017453292519943295
KX = R_KM * D2R
NAMES = ("count", "wspd", "wspd_std", "vr", "vt", "vmax")


def tables(lat_c, n_theta):
    """(cos_lat_c, sin_lat_c, sector_sin, sector_cos [n_theta / 4 + 1])."""
    mq = n_theta // 4
    lat = np.deg2rad(np.float64(lat_c))
    borders = np.deg2rad(np.arange(mq + 1, dtype=np.float64) * (90.0 / mq))
    return float(np.cos(lat)), float(np.sin(lat)), np.sin(borders), np.cos(borders)


def wrap_centre(lon_c):
    """Step 0."""
    return lon_c - 360.0 * float(np.rint(lon_c / 360.0))


def chart(lon, lat, lon_c, lat_c, cos_c, sin_c):
    """(x, y) in km of every pixel; lon_c as step 0 left it."""
    dl = lon - lon_c
    dl = dl - 360.0 * np.rint(dl / 360.0)
    dy = (lat - lat_c) * D2R
    h = 0.5 * dy
    m = (cos_c - sin_c * h) - (0.5 * cos_c) * (h * h)
    return (KX * dl) * m, R_KM * dy


def quadrant_of(x, y):
    """(Q, a, b) by the four sign rules; x = y = 0 (and NaN, which no rule takes) gives Q = 0 with (a, b) = (0, 1): sector 0."""
    rules = [(x >= 0.0) & (y > 0.0), (x > 0.0) & (y <= 0.0), (x <= 0.0) & (y < 0.0), (x < 0.0) & (y >= 0.0)]
    pairs = [(x, y), (-y, x), (-x, -y), (y, -x)]
    assert not (rules[0] & rules[1]).any() and not (rules[1] & rules[2]).any() and not (rules[2] & rules[3]).any() and not (rules[3] & rules[0]).any()
    Q = np.zeros(x.shape, np.int64)
    a, b = np.zeros(x.shape), np.ones(x.shape)
    for k in range(4):
        Q = np.where(rules[k], k, Q)
        a, b = np.where(rules[k], pairs[k][0], a), np.where(rules[k], pairs[k][1], b)
    return Q, a, b


def ring_sector(x, y, dr_km, n_r, n_theta, sector_sin, sector_cos):
    """(inside, r, kr, sector) per pixel."""
    mq = n_theta // 4
    with np.errstate(invalid="ignore"):
        rr = x * x + y * y
        r = np.sqrt(rr)
        fr = np.floor(r / dr_km)
        inside = fr < float(n_r)
        Q, a, b = quadrant_of(x, y)
        lo, hi = np.zeros(x.shape, np.int64), np.full(x.shape, mq, np.int64)
        while True:
            active = hi - lo > 1
            if not active.any():
                break
            mid = (lo + hi) >> 1
            ge = a * sector_cos[mid] >= b * sector_sin[mid]
            lo = np.where(active & ge, mid, lo)
            hi = np.where(active & ~ge, mid, hi)
    kr = np.where(inside, fr, 0.0).astype(np.int64)
    return inside, r, kr, Q * mq + lo


def components(u, v, x, y, r):
    """Step 6: (vr, vt), both 0 where r == 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        vr = np.where(r == 0.0, 0.0, (u * x + v * y) / r)
        vt = np.where(r == 0.0, 0.0, (v * x - u * y) / r)
    return vr, vt


def accumulate(out, kr, sector, sp, q, vr, vt):
    """Step 8 for the pixels given as vectors, in the order given."""
    at = (kr, sector)
    np.add.at(out[0], at, 1)
    for plane, a, scale in ((1, sp, Q24), (2, q, Q16), (3, vr, Q24), (4, vt, Q24)):
        np.add.at(out[plane], at, quantise(a, scale))
    np.maximum.at(out[5], at, quantise(sp, Q24))
    return out


def pixel_bins(lon, lat, ch, sh, w, keep, lon_c, lat_c, cos_c, sin_c, dr_km, n_r, n_theta, sector_sin, sector_cos):
    """dict(ok, x, y, r, kr, sector, sp, q, u, v, vr, vt) of every pixel: steps 2-7 (ok: the pixel is added)."""
    ok, u, v, sp, q = gref.pixel_terms(w, keep, ch, sh)
    x, y = chart(lon, lat, wrap_centre(lon_c), lat_c, cos_c, sin_c)
    inside, r, kr, sector = ring_sector(x, y, dr_km, n_r, n_theta, sector_sin, sector_cos)
    vr, vt = components(u, v, x, y, r)
    return dict(ok=ok & inside, valid=ok, x=x, y=y, r=r, kr=kr, sector=sector, sp=sp, q=q, u=u, v=v, vr=vr, vt=vt)


def sums_core(w, keep, lon_c, lat_c, cos_c, sin_c, dr_km, n_r, n_theta, sector_sin, sector_cos, tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t,
              sample_first, sample_t, into=None):
    """int64 [6, n_r, n_theta] (n, Ss, Sq, Sr, St, Mx) from the entry's own arguments; `into` is accumulated into."""
    lon, lat, ch, sh = gref.geolocate(tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t, sample_first, sample_t)
    p = pixel_bins(lon, lat, ch, sh, w, keep, lon_c, lat_c, cos_c, sin_c, dr_km, n_r, n_theta, sector_sin, sector_cos)
    ok = p["ok"]
    out = np.zeros((6, n_r, n_theta), np.int64) if into is None else into
    return accumulate(out, *[p[k][ok] for k in ("kr", "sector", "sp", "q", "vr", "vt")])


def tie_tables(tie_line, tie_sample, tie_lon, tie_lat, tie_heading, line, sample):
    """The entry's tie arguments from the public call's: (tie_lon continuous, tie_lat, cos, sin, line bracket, sample bracket)."""
    h = np.deg2rad(np.asarray(tie_heading, dtype=np.float64))
    lf, lt = bracket(tie_line, line)
    sf, st = bracket(tie_sample, sample)
    return continuous(tie_lon), np.asarray(tie_lat, dtype=np.float64), np.cos(h), np.sin(h), lf, lt, sf, st


def sums(w, tie_line, tie_sample, tie_lon, tie_lat, tie_heading, centre, radius, sectors, line=None, sample=None, keep=None, into=None):
    """The same from the public call's arguments: centre = (lon, lat), radius = (dr_km, n_r), sectors = n_theta."""
    L, S = np.asarray(w).shape
    line = np.arange(L, dtype=np.float64) if line is None else np.asarray(line, np.float64)
    sample = np.arange(S, dtype=np.float64) if sample is None else np.asarray(sample, np.float64)
    (lon_c, lat_c), (dr_km, n_r) = centre, radius
    return sums_core(w, keep, float(lon_c), float(lat_c), *tables(lat_c, sectors)[:2], float(dr_km), n_r, sectors, *tables(lat_c, sectors)[2:],
                     *tie_tables(tie_line, tie_sample, tie_lon, tie_lat, tie_heading, line, sample), into=into)


def merge(a, b):
    out = a + b
    out[5] = np.maximum(a[5], b[5])
    return out


def finish(s):
    """dict(count, wspd, wspd_std, vr, vt, vmax) from int64 sums [6, ...], in the statement's order."""
    n, ss, sq, sr, st, mx = (np.asarray(a) for a in s)
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = n.astype(np.float64)
        wspd = (ss.astype(np.float64) / nd) * 2.0 ** -24
        vr = (sr.astype(np.float64) / nd) * 2.0 ** -24
        vt = (st.astype(np.float64) / nd) * 2.0 ** -24
        s1, s2 = ss.astype(np.float64) * 2.0 ** -24, sq.astype(np.float64) * 2.0 ** -16
        var = (s2 - (s1 * s1) / nd) / (nd - 1.0)
        std = np.where(n < 2, np.nan, np.sqrt(np.where(var < 0.0, 0.0, var)))
        vmax = np.where(n == 0, np.nan, mx.astype(np.float64) * 2.0 ** -24)
    return dict(count=n.copy(), wspd=wspd, wspd_std=std, vr=vr, vt=vt, vmax=vmax)
