"""numpy restatement of the forward operator on rasters (include/xsw.h: xsw_lut_eval, xsw_lut_eval_cr):
sigma0 in dB that a table predicts for a wind field, and the derivatives of that interpolant.  Per point, in float64, with only
IEEE + - * / in the order written here (numpy never fuses a multiply with an add):

  fold (fold_phi only)   p = fmod(phi, 360); p < 0: p = p + 360; reflected = p > ap[-1]; reflected: p = 360 - p
  cell, per axis         hi = clip(searchsorted(axis, x, side left), 1, n - 1), lo = hi - 1
  lerp, always           slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (x - x_lo) + y_lo
                         incidence for the four (w, p) corners, then wind speed (slopes s_b), then direction (slope sp)
  dphi = reflected ? -sp : sp;  dwspd = ((s_1 - s_0) / (p_hi - p_lo)) * (p - p_lo) + s_0
  NaN everywhere where a coordinate is NaN or outside [axis[0], axis[-1]] (the direction: after the fold)

tests/test_forward_cpu.py pins sigma0_db to `LutModel.__call__` bit for bit; the GPU tests hold the kernels to this file."""
import numpy as np


def fold(phi, phi_last):
    """(p, reflected) of the fold step."""
    phi = np.asarray(phi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        p = np.fmod(phi, 360.0)
        p = np.where(p < 0, p + 360.0, p)
        reflected = p > phi_last
    return np.where(reflected, 360.0 - p, p), reflected


def _cell(axis, x):
    """(lo, hi, outside) of lerp_axis: an outside or NaN point gets the clipped cell and is NaN in the end."""
    with np.errstate(invalid="ignore"):
        outside = ~((x >= axis[0]) & (x <= axis[-1]))
    hi = np.clip(np.searchsorted(axis, x), 1, len(axis) - 1)
    return hi - 1, hi, outside


def _lerp(y_lo, y_hi, x_lo, x_hi, x):
    slope = (y_hi - y_lo) / (x_hi - x_lo)
    return slope, slope * (x - x_lo) + y_lo


def eval_co(table, ai, aw, ap, inc, wspd, phi, fold_phi=True):
    """dict(sigma0_db, dwspd, dphi, reflected) for the co-pol table[i][w][p] with axes ai, aw, ap."""
    table, ai, aw, ap = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw, ap))
    inc, wspd, phi = (np.asarray(v).astype(np.float64) for v in (inc, wspd, phi))
    if fold_phi:
        p, reflected = fold(phi, ap[-1])
    else:
        p, reflected = phi, np.zeros(phi.shape, bool)
    il, ih, out_i = _cell(ai, inc)
    wl, wh, out_w = _cell(aw, wspd)
    pl, ph, out_p = _cell(ap, p)
    with np.errstate(all="ignore"):
        v = [[_lerp(table[il, w, q], table[ih, w, q], ai[il], ai[ih], inc)[1] for q in (pl, ph)] for w in (wl, wh)]
        s0, u0 = _lerp(v[0][0], v[1][0], aw[wl], aw[wh], wspd)
        s1, u1 = _lerp(v[0][1], v[1][1], aw[wl], aw[wh], wspd)
        sp, db = _lerp(u0, u1, ap[pl], ap[ph], p)
        dwspd = _lerp(s0, s1, ap[pl], ap[ph], p)[1]
        dphi = np.where(reflected, -sp, sp)
    bad = out_i | out_w | out_p
    return dict(sigma0_db=np.where(bad, np.nan, db), dwspd=np.where(bad, np.nan, dwspd), dphi=np.where(bad, np.nan, dphi), reflected=reflected)


def eval_cr(table, ai, aw, inc, wspd):
    """dict(sigma0_db, dwspd) for the cross-pol table[i][w]: incidence, then wind speed."""
    table, ai, aw = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw))
    inc, wspd = (np.asarray(v).astype(np.float64) for v in (inc, wspd))
    il, ih, out_i = _cell(ai, inc)
    wl, wh, out_w = _cell(aw, wspd)
    with np.errstate(all="ignore"):
        v0 = _lerp(table[il, wl], table[ih, wl], ai[il], ai[ih], inc)[1]
        v1 = _lerp(table[il, wh], table[ih, wh], ai[il], ai[ih], inc)[1]
        s, db = _lerp(v0, v1, aw[wl], aw[wh], wspd)
    bad = out_i | out_w
    return dict(sigma0_db=np.where(bad, np.nan, db), dwspd=np.where(bad, np.nan, s))


def points(rng, axes, n, margins=(1.0, 0.5, 5.0)):
    """n test points per axis of `axes` (2 or 3 of them): drawn up to the margins beyond the axes, every node of each axis put in
    exactly (first and last included, cycling through them), and one NaN per coordinate."""
    cols = []
    for k, (ax, m) in enumerate(zip(axes, margins)):
        ax = np.asarray(ax, dtype=np.float64)
        x = rng.uniform(ax[0] - m, ax[-1] + m, n)
        at = rng.choice(n, size=min(n // 4, 4 * len(ax)), replace=False)
        x[at] = ax[np.arange(len(at)) % len(ax)]
        x[at[0]], x[at[1]] = ax[0], ax[-1]
        cols.append(x)
    for k, x in enumerate(cols):
        x[n - 1 - k] = np.nan
    return cols


def nonuniform_tables():
    """Smooth dB tables on NON-uniform axes: co[3][11][9] (phi_pad = 12: rows alternate between 8- and 4-entry offsets in a 64-byte
    line) and cr[3][13], as (co, ai, aw, ap), (cr, ai, awcr)."""
    ai = np.array([20.0, 30.0, 45.0])
    aw = np.cumsum(0.5 + 0.25 * (np.arange(11) % 3)) - 0.25
    ap = 180.0 * (np.arange(9) / 8.0) ** 1.3
    awcr = np.cumsum(0.75 + 0.5 * (np.arange(13) % 2))
    co = -22.0 + 9.0 * np.log10(1.0 + aw)[None, :, None] + 2.0 * np.cos(np.deg2rad(2.0 * ap))[None, None, :] * (1.0 + 0.1 * aw)[None, :, None] \
        - 0.15 * (ai - 20.0)[:, None, None]
    cr = -36.0 + 12.0 * np.log10(1.0 + awcr)[None, :] - 0.05 * (ai - 20.0)[:, None]
    return (co, ai, aw, ap), (cr, ai, awcr)


AFFINE = dict(a=3.0, b=2.0, c=5.0, d=-3.0, e=1.0)  # T = a + b inc + c w + d p + e w p


def affine_table():
    """(co, ai, aw, ap) with small-integer axes and entries, affine in each axis: every operation of the definition is exact for
    coordinates that are multiples of 1/8."""
    ai, aw, ap = np.array([20.0, 22.0, 26.0]), np.array([1.0, 2.0, 4.0, 8.0]), np.array([0.0, 8.0, 16.0, 32.0, 40.0])
    k = AFFINE
    co = k["a"] + k["b"] * ai[:, None, None] + k["c"] * aw[None, :, None] + k["d"] * ap[None, None, :] + k["e"] * aw[None, :, None] * ap[None, None, :]
    return co, ai, aw, ap
