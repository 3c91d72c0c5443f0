"""numpy restatement of xsarsea_amd.streaks, written from its rules and from the steps of the reference's
notebook docs/examples/streaks.ipynb: mean of the histograms over the leading axes, circular smoothing, peak bin, + pi/2; then the
ambiguity removal against the a-priori wind and the bilinear spreading over the raster.  Loops where the order of a sum is part
of the rule."""
import numpy as np

import gradients_ref as ref

TAPS = [np.array(k, float) / 4 for k in ([1, 2, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 2, 0, 0, 0, 1],
                                         [1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1])]


def nanmean_leading(a, keep):
    """NaN-skipping mean over every axis but the last `keep`: the sum in the order of the flattened leading axes, one division
    by the count of non-NaN terms, NaN where there is none."""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape((-1,) + a.shape[a.ndim - keep:])
    s, cnt = np.zeros(a.shape[1:]), np.zeros(a.shape[1:])
    for plane in a:
        ok = ~np.isnan(plane)
        s = np.where(ok, s + np.where(ok, plane, 0.0), s)
        cnt = cnt + ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, s / cnt, np.nan)


def circ_smooth(m):
    """Bx, Bx2, Bx4, Bx8 in turn along the last axis, circular: out[i] = 0 + B[0] m[i - h] + B[1] m[i - h + 1] + ..., every tap
    multiplying (the zero ones too)."""
    x = np.asarray(m, dtype=np.float64)
    n = x.shape[-1]
    for B in TAPS:
        h = len(B) // 2
        out = np.zeros_like(x)
        for j, b in enumerate(B):
            out = out + b * x[..., (np.arange(n) + j - h) % n]
        x = out
    return x


def smoothed_mean(weight, smooth=True):
    m = nanmean_leading(weight, 3)
    return circ_smooth(m) if smooth else m


def streaks_direction(weight, used_ratio, angles, smooth=True, orthogonal=True):
    """dict(angle, weight, used_ratio, index) [line, sample] from weight [..., line, sample, angles]."""
    m = smoothed_mean(weight, smooth)
    index = np.argmax(np.where(np.isnan(m), 0.0, m), axis=-1)  # numpy's argmax: the first maximum
    angles = np.asarray(angles, dtype=np.float64)
    angle = angles[index] + np.pi / 2 if orthogonal else angles[index]
    return dict(angle=angle, weight=np.take_along_axis(m, index[..., None], -1)[..., 0], used_ratio=nanmean_leading(used_ratio, 2),
                index=index.astype(np.int32), m=m)


def near_tie(m, rel=1e-9):
    """Windows whose two largest (NaN-filled) values differ by less than `rel` relative: their peak bin may legitimately differ
    between two float64 evaluations."""
    f = np.sort(np.where(np.isnan(m), 0.0, m), axis=-1)
    return (f[..., -1] - f[..., -2]) < rel * np.abs(f[..., -1])


def at_windows(anc, line, sample, windows_line, windows_sample):
    """The raster pixel nearest each window centre (a tie goes to the larger coordinate)."""
    return np.asarray(anc)[np.ix_(ref.nearest(line, windows_line), ref.nearest(sample, windows_sample))]


def resolve(angle, weight, used_ratio, a, min_weight=None, min_used_ratio=None):
    """exp(1j angle), negated where Re(d conj(a)) < 0; NaN + NaN j where the rules say so.  `a`: the a-priori wind at the windows."""
    a = np.asarray(a, dtype=np.complex128)
    d = np.exp(1j * np.asarray(angle, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        dot = d.real * a.real + d.imag * a.imag
        d = np.where(dot < 0, -d, d)
        bad = np.isnan(angle) | np.isnan(weight) | np.isnan(a.real) | np.isnan(a.imag) | ((a.real == 0) & (a.imag == 0))
        if min_weight is not None:
            bad |= weight < min_weight
        if min_used_ratio is not None:
            bad |= used_ratio < min_used_ratio
    return np.where(bad, complex(np.nan, np.nan), d)


def bracket(centres, coords):
    """Per coordinate: (first, second, t): the neighbouring centres around it and the weight of the second, t from one division;
    outside the centres (and for a single centre) the edge centre alone, t = 0."""
    c = np.asarray(centres, dtype=np.float64)
    first, second, t = [], [], []
    for x in np.asarray(coords, dtype=np.float64):
        if len(c) == 1 or x <= c[0]:
            k = (0, 0, 0.0)
        elif x >= c[-1]:
            k = (len(c) - 1, len(c) - 1, 0.0)
        else:
            i = max(j for j in range(len(c)) if c[j] <= x)
            k = (i, i + 1, (x - c[i]) / (c[i + 1] - c[i]))
        first.append(k[0]), second.append(k[1]), t.append(k[2])
    return np.array(first), np.array(second), np.array(t)


def blend_sums(dirs, windows_line, windows_sample, line, sample):
    """(vx, vy) per pixel: the float64 sums of the bilinear blend, corners in line-major order from 0, each weighing
    (line weight) * (sample weight), NaN corners skipped."""
    dirs = np.asarray(dirs, dtype=np.complex128)
    i0, i1, tl = bracket(windows_line, line)
    j0, j1, ts = bracket(windows_sample, sample)
    vx, vy = np.zeros((len(i0), len(j0))), np.zeros((len(i0), len(j0)))
    for ii, wl in ((i0, 1.0 - tl), (i1, tl)):
        for jj, ws in ((j0, 1.0 - ts), (j1, ts)):
            w = wl[:, None] * ws[None, :]
            d = dirs[np.ix_(ii, jj)]
            ok = ~(np.isnan(d.real) | np.isnan(d.imag))
            vx = np.where(ok, vx + w * np.where(ok, d.real, 0.0), vx)
            vy = np.where(ok, vy + w * np.where(ok, d.imag, 0.0), vy)
    return vx, vy


LONGDOUBLE_EPS = float(np.finfo(np.longdouble).eps)   # 2**-63 where long double is the x87 format


def ancillary_exact(dirs, windows_line, windows_sample, anc, line, sample):
    """The finish of `ancillary` in np.longdouble on the float64 sums of `blend_sums` (which are the rule, not an approximation:
    four corners in a stated order): hypot(vx, vy), hypot(a.re, a.im), the product and the quotient.  dict(real, imag
    (longdouble; meaningful on `blend` only), nan, fallback, blend: the three classes of pixels, which cover the raster; vx, vy)."""
    anc = np.asarray(anc, dtype=np.complex128)
    vx, vy = blend_sums(dirs, windows_line, windows_sample, line, sample)
    nan = np.isnan(anc.real) | np.isnan(anc.imag)
    fallback = ~nan & (vx == 0) & (vy == 0)     # hypot(vx, vy) == 0 exactly there and nowhere else
    blend = ~nan & ~fallback
    lx, ly = vx.astype(np.longdouble), vy.astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        nv, m = np.hypot(lx, ly), np.hypot(anc.real.astype(np.longdouble), anc.imag.astype(np.longdouble))
        re, im = m * lx / nv, m * ly / nv
    assert (nan ^ fallback ^ blend).all() and not (nan & fallback).any()
    return dict(real=re, imag=im, nan=nan, fallback=fallback, blend=blend, vx=vx, vy=vy)


TINY_NORMAL = float(np.finfo(np.float64).tiny)


def ancillary_ulps(got, exact):
    """(worst error of the blend pixels' components in units of spacing(|exact|), worst absolute error of the components whose
    exact value is non-zero and below the smallest normal float64 in units of 2**-1074, their count, the count of all blend
    components).  A component whose exact value is 0 (its float64 sum is 0: every corner lies on the other axis; or |a| is 0) is
    not in those counts: it must be a zero of the sum's sign, which is asserted here.  m * (+-0.0) / |v| and 0 * v / |v| have no
    rounding, and a sum that starts from +0.0 never gives -0.0."""
    got = np.asarray(got)
    b = exact["blend"]
    worst, worst_tiny, n_tiny = 0.0, 0.0, 0
    for g, e, v in ((got.real[b], exact["real"][b], exact["vx"][b]), (got.imag[b], exact["imag"][b], exact["vy"][b])):
        zero = e == 0
        assert not np.signbit(v[v == 0]).any()
        assert (g[zero].view(np.int64) == np.copysign(0.0, v[zero]).view(np.int64)).all(), "an exact zero keeps the sum's sign"
        tiny = ~zero & (np.abs(e) < TINY_NORMAL)
        n_tiny += int(tiny.sum())
        if tiny.any():
            worst_tiny = float(np.maximum(worst_tiny, np.max(np.abs(g[tiny] - e[tiny])) / np.longdouble(2.0) ** -1074))   # (NaN propagates)
        rest = ~zero & ~tiny
        if rest.any():
            err = np.abs(g[rest].astype(np.longdouble) - e[rest])
            worst = float(np.maximum(worst, np.max(err / np.spacing(np.abs(e[rest]).astype(np.float64)))))
    return worst, worst_tiny, n_tiny, 2 * int(b.sum())


def ancillary(dirs, windows_line, windows_sample, anc, line, sample):
    """|a| v / |v| per pixel, v the bilinear blend of the resolved directions: corners in line-major order, each weighing
    (line weight) * (sample weight), NaN corners skipped; a where |v| == 0; NaN + NaN j where a has a NaN part."""
    anc = np.asarray(anc, dtype=np.complex128)
    vx, vy = blend_sums(dirs, windows_line, windows_sample, line, sample)
    nv, m = np.hypot(vx, vy), np.hypot(anc.real, anc.imag)
    out = anc.copy()
    go = nv != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out.real[go] = (m * vx / nv)[go]
        out.imag[go] = (m * vy / nv)[go]
    out[np.isnan(anc.real) | np.isnan(anc.imag)] = complex(np.nan, np.nan)
    return out
