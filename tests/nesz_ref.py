"""The noise flattening's log10 / exp10 pair (xsw_nesz.hpp: nesz_log10, nesz_exp10; float32 rasters: v_log_f32 / v_exp_f32) against
exact arithmetic.  TEST INFRASTRUCTURE ONLY; standard library and numpy.

The raster that isolates the pair: N lines x 3 samples, incidence 30, 35, 40 on every line, noise NaN but for column 1, which
holds one argument v per line.  Columns 0 and 2 have no valid noise (their mean is NaN), so every line fits the single point
(35, y), y = 10 log10(v): x0 = 35, the moments about it are n = 1, Sx = 0, Sy = y, Sxx = Sxy = 0, det = 0 exactly, and the
minimum-norm branch gives slope = y / 70, intercept = y / 2.  The three outputs of a line are

    out[s] = 10 ** (((x_s / 70 + 1 / 2) * y - 1) / 10),    x_s = 30, 35, 40

that is nesz_log10 once, a handful of plain float64 operations (`restate`, in the kernel's order), and nesz_exp10 at three
exponents.  `exact` evaluates the same expression of the stored v in `decimal` at PREC digits.

Bounds on the relative error of an output whose exact value is a normal number, from the source's own statements:
    float64 rasters   1e-15 * (1 + 0.2303 |y|) + r        the header's "~1e-15 relative" for each of the pair; an error e of
                                                          log10 is an error ln(10) / 10 * |y| * e of the output
    float32 rasters   2**-23 * (1 + 1.15 |t| + 0.345 |y|) + r
                                                          one ulp each for v_exp_f32 and v_log_f32 (ln(10) / 10 * 1.5 |y|: the
                                                          product with 3.0103f rounds too), and the float32 rounding of
                                                          t * log2(10) (ln(2) * 3.32 |t| / 2)
r is the error the plain float64 restatement (numpy's log10 and power) shows at that argument: what the operations between the
pair cost whatever the pair does."""
import decimal
import functools
from collections import namedtuple

import numpy as np

PREC = 90
_D = decimal.Context(prec=PREC, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
INC = (30.0, 35.0, 40.0)
SPECIALS = ("zero", "negative", "inf", "nan", "denormal")


def mantissas(dtype):
    t = np.dtype(dtype).type
    one, two, zero = t(1), t(2), t(0)
    r = np.sqrt(t(0.5))
    return [one, np.nextafter(one, zero), np.nextafter(one, two), r, np.nextafter(r, zero), np.nextafter(r, two), np.sqrt(two),
            t(0.75), t(0.9999), t(1.1), t(1.25), t(4.0) / t(3.0), t(1.4142)]


def exponents(dtype):
    if np.dtype(dtype) == np.float64:
        return sorted(set(range(-1020, 1021, 17)) | {-1022, -1, 0, 1, 1023})
    return sorted(set(range(-119, 120, 17)) | {-120, -1, 0, 1, 120})


@functools.lru_cache(maxsize=None)
def arguments(dtype):
    """(v, kinds): the finite normal arguments m * 2**k (each once), then the special lines -- 0, a negative value, +inf, NaN and
    denormals (as many as make len(v) % 4 == 3: the last workgroup of k_nesz_fit then holds three lines); kinds[i] is "normal" or
    the name of the special.  Read-only."""
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    with np.errstate(all="ignore"):
        v = np.array([np.ldexp(m, k) for m in mantissas(dtype) for k in exponents(dtype)], dtype=dtype)
    v = np.unique(v[np.isfinite(v) & (v >= fi.tiny)])
    rest = [0.0, -1.5, np.inf, np.nan, fi.smallest_subnormal * 3]
    kinds = ["normal"] * v.size + list(SPECIALS)
    k = 0
    while (v.size + len(rest)) % 4 != 3:
        rest.append(fi.tiny / 2 ** (k + 1) * 1.5)
        kinds.append("denormal")
        k += 1
    v = np.concatenate([v, np.array(rest, dtype=dtype)])
    v.setflags(write=False)
    return v, tuple(kinds)


def rasters(dtype):
    """(noise, inc) of the module docstring for `arguments(dtype)`."""
    v, _ = arguments(dtype)
    noise = np.full((v.size, 3), np.nan, dtype=dtype)
    noise[:, 1] = v
    inc = np.ascontiguousarray(np.broadcast_to(np.array(INC, dtype=dtype), (v.size, 3)))
    return noise, inc


def restate(v, log10=np.log10, exp10=lambda t: np.power(10.0, t)):
    """The kernels' float64 operations on one column of arguments, in their order (k_nesz_fit's minimum-norm branch, k_nesz_eval):
    [N, 3] float64.  A line whose y is not finite has nothing to fit: NaN."""
    v = np.asarray(v, dtype=np.float64)
    x = np.array(INC)
    with np.errstate(all="ignore"):
        y = 10.0 * log10(v)
        x0, xm, ym = 35.0, 0.0 / 1.0, y / 1.0
        slope = ym / (2.0 * (xm + x0))
        icpt = 0.5 * ym
        t = (x[None, :] * slope[:, None] + icpt[:, None] - 1.0) * 0.1
        out = exp10(t)
    out[~np.isfinite(y)] = np.nan
    return out


# the header's series in numpy (no fused multiply-add, a true division for the reciprocal: a port of the method, not of the bits)
LOG_COEF = tuple(1.0 / k for k in range(21, 1, -2))  # 1/21 ... 1/3
EXP_COEF = tuple(1.0 / f for f in (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0))


def series_log10(v, coef=LOG_COEF):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        plain = ~((v >= np.finfo(np.float64).tiny) & (v <= np.finfo(np.float64).max))
        m, e = np.frexp(np.where(plain, 1.0, v))
        low = m < 0.70710678118654752440
        m, e = np.where(low, m * 2.0, m), np.where(low, e - 1, e).astype(np.float64)
        z = (m - 1.0) / (m + 1.0)
        z2 = z * z
        p = np.full_like(z, coef[0])
        for c in coef[1:]:
            p = p * z2 + c
        lnm = 2.0 * z * z2 * p + 2.0 * z
        out = e * 0.30102999566361177 + (e * 3.694239077158931e-13 + lnm * 0.4342944819032518)
        return np.where(plain, np.log10(v), out)


def series_exp10(t, coef=EXP_COEF):
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        plain = ~(np.abs(t) < 300.0)
        ts = np.where(plain, 0.0, t)
        kf = np.rint(ts * 3.321928094887362)
        r = -kf * 3.694239077158931e-13 + (-kf * 0.30102999566361177 + ts)
        g = r * 2.302585092994046
        p = np.full_like(g, coef[0])
        for c in coef[1:]:
            p = p * g + c
        return np.where(plain, np.power(10.0, t), np.ldexp(p, kf.astype(np.int64)))


Exact = namedtuple("Exact", "hi lo y t")  # the exact output as hi + lo (float64 pair; hi inf / 0 outside float64), y and t as float64


@functools.lru_cache(maxsize=None)
def exact(dtype):
    """The exact outputs for the normal and denormal lines of `arguments(dtype)` (NaN on the lines that have nothing to fit)."""
    v, kinds = arguments(dtype)
    n = v.size
    hi, lo, ys, ts = (np.full((n, 3), np.nan) for _ in range(4))
    D = decimal.Decimal
    tenth, half = D(1) / D(10), D(1) / D(2)
    fmax = D(float(np.finfo(np.float64).max))
    for i in range(n):
        if kinds[i] not in ("normal", "denormal"):
            continue
        y = _D.multiply(D(10), _D.log10(D(float(v[i]))))
        for s, x in enumerate(INC):
            a = _D.add(_D.divide(D(x), D(70)), half)
            t = _D.subtract(_D.multiply(_D.multiply(a, y), tenth), tenth)
            E = _D.power(D(10), t)
            ys[i, s], ts[i, s] = float(y), float(t)
            if E > fmax:
                hi[i, s], lo[i, s] = np.inf, 0.0
            else:
                h = float(E)
                hi[i, s], lo[i, s] = h, (float(_D.subtract(E, D(h))) if h != 0.0 else 0.0)
    for a in (hi, lo, ys, ts):
        a.setflags(write=False)
    return Exact(hi, lo, ys, ts)


def rel_error(got, ex):
    """|got - exact| / exact where the exact value is a normal float64 (elsewhere NaN)."""
    tiny = np.finfo(np.float64).tiny
    with np.errstate(all="ignore"):
        normal = np.isfinite(ex.hi) & (ex.hi >= tiny)
        return np.where(normal, np.abs(((got - ex.hi) - ex.lo) / ex.hi), np.nan)


@functools.lru_cache(maxsize=None)
def restatement_error(dtype):
    """r of the bounds: the relative error of the plain float64 restatement at every output."""
    out = rel_error(restate(arguments(dtype)[0].astype(np.float64)), exact(dtype))
    out.setflags(write=False)
    return out


def bound(dtype):
    """The bound on the relative error of every output, [N, 3] (module docstring)."""
    ex, r = exact(dtype), restatement_error(dtype)
    if np.dtype(dtype) == np.float64:
        return 1e-15 * (1.0 + 0.2303 * np.abs(ex.y)) + r
    return 2.0 ** -23 * (1.0 + 1.15 * np.abs(ex.t) + 0.345 * np.abs(ex.y)) + r


def compared(dtype):
    """The outputs that are held to the bound: the exact value is a normal number of float64 -- and, for float32 rasters, of
    float32, the format v_exp_f32 returns."""
    ex = exact(dtype)
    fi = np.finfo(np.float64 if np.dtype(dtype) == np.float64 else np.float32)
    with np.errstate(all="ignore"):
        return np.isfinite(ex.hi) & (ex.hi >= float(fi.tiny)) & (ex.hi <= float(fi.max))


def worst_ratio(got, dtype):
    """(largest error / bound over the compared outputs, its (line, sample), number of compared outputs)."""
    with np.errstate(all="ignore"):
        ratio = np.where(compared(dtype), rel_error(got, exact(dtype)) / bound(dtype), 0.0)
    assert not np.isnan(ratio).any(), "a compared output is NaN"
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(k) for k in at), int(compared(dtype).sum())


def check_lines(got, dtype, what):
    """The structure every route must give: a NaN line for 0, a negative value, +inf and NaN; no NaN anywhere else."""
    _, kinds = arguments(dtype)
    nan_line = np.array([k in ("zero", "negative", "inf", "nan") for k in kinds])
    assert got.dtype == np.float64 and got.shape == (len(kinds), 3), what
    assert np.isnan(got[nan_line]).all(), f"{what}: a line with nothing to fit is not NaN"
    bad = np.flatnonzero(np.isnan(got[~nan_line]).any(axis=1))
    assert bad.size == 0, f"{what}: NaN on lines {np.flatnonzero(~nan_line)[bad][:8].tolist()} ({[kinds[k] for k in np.flatnonzero(~nan_line)[bad][:8]]})"
