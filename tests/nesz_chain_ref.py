"""The whole noise flattening (csrc/xsw_nesz.hpp: k_nesz_colsum, k_nesz_colmean, k_nesz_center, k_nesz_fit, k_nesz_eval) against a
high-precision evaluation of the same operation.  TEST INFRASTRUCTURE ONLY; standard library and numpy.

`reference`   the operation in np.longdouble (64-bit significand, asserted below), from the stored input values: column nan-means
              of noise and incidence, NaN noise filled with the column mean, y = 10 log10, the samples whose y is finite fitted
              by a line about their own mean abscissa, out = 10 ** ((x * slope + icpt - 1) / 10) at every column.  Branches:
              nothing fitted -> NaN line; every fitted abscissa equal -> numpy's minimum-norm answer slope = ym / (2 x),
              icpt = ym / 2; a NaN abscissa among the fitted samples -> NaN line (the kernel's documented behaviour; numpy
              raises there); a column whose incidence mean is NaN is NaN in every line.  For float32 rasters the fill value is
              the column mean rounded once to float32, as k_nesz_fit's take() has it; everything else is exact.
`restate`     float64 numpy in the order the kernels state: column sums from +0.0 over a block's lines in ascending order, the
              blocks added in ascending order (nesz_blocks as tests/test_host_lutplan.py restates it); x0 from 1024 strided
              partials, an xor butterfly 32..1 per wave, the waves in ascending order; the fit's five moments over 256 threads,
              groups of V adjacent samples with stride 256, then the tail samples, a butterfly per wave, four waves in
              ascending order; the closed form and its det test as written; np.log10 and 10.0 ** t for the pair.  The
              library is built without contraction of a * b + c, so the restatement differs from the device in the pair alone.
              `mutate=` selects one wrong variant (MUTANTS).
`bound`       the relative bound per pixel.  The fitted value at column s is a linear form of the line's y,
              yhat(x_s) = sum_i h_i(x_s) y_i with h_i(x_s) = 1 / n + (x_s - xbar)(x_i - xbar) / Sxx, so an error e_i of y_i moves
              it by at most max|e_i| * sum_i |h_i(x_s)| <= max|e_i| * kappa_l(s),
                  kappa_l(s) = 1 + |x_s - xbar| kappa1_l,    kappa1_l = sum_i |x_i - xbar| / Sxx
              (triangle inequality; O(n + S) per line).  kappa1 is infinite on minimum-norm lines: kappa = 1 there.  With
              |e_i| <= e * |y_i| <= e * Ymax_l this is the pair's own bound of tests/nesz_ref.py with |y| replaced by
              kappa_l(s) * Ymax_l:
                  float64 rasters   1e-15 * (1 + 0.2303 kappa Ymax) + F * max(R_l, 2**-52)
                  float32 rasters   2**-23 * (1 + 1.15 |t| + 0.345 kappa Ymax) + F * max(R_l, 2**-52)
                  both plus 2**-52 * D * 0.2303 |x_s - xbar| * 2 |m| (Ymax + |m slope|) / var,  m = xbar - x0
              The last term is the closed form's own: the kernel takes its moments about x0, the mean of ALL column abscissae,
              not about the line's own mean xbar.  With a_i = x_i - x0 (mean m, variance var over the fitted samples) it forms
              det = n Sxx - Sx^2 = n^2 (var + m^2) - n^2 m^2 and n Sxy - Sx Sy = n^2 (cov + m ybar) - n^2 m ybar: a relative
              error D 2**-52 of each product leaves cov / var = slope with an absolute error of D 2**-52 * 2 (|m ybar| + m^2
              |slope|) / var, which the evaluation carries |x_s - xbar| away from the line's centre; |ybar| <= Ymax; ln(10) / 10
              = 0.2303 turns dB into a relative error.  D = 3 + (additions along a moment's longest chain) / 2: half an ulp
              for each of a thread's trips, the six butterfly steps and the waves, 1.5 ulp for the products.  On an ordinary
              line m^2 << var and the term is a fraction of the first one; on a line that fits two adjacent samples far from
              the raster's centre (m^2 / var ~ 1e5) it is the whole error, 1e-9, and the restatement shows it on the CPU (the
              other terms alone are exceeded 16 times there).
              R_l is the largest relative error of `restate` against `reference` on line l: what the float64 sums and the
              closed form cost whatever the pair does -- measured against the reference, never against the device.  F = 4
              covers the later roundings that move when the kernel's log10 differs from numpy's within its stated 1e-15."""
import concurrent.futures
import functools
from collections import namedtuple

import numpy as np

from test_host_plan import source_define

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no 64-bit significand here: the reference would be no better than the kernel"

F = 4.0
MUTANTS = {1: "the tail lines of every colsum block are skipped (beyond the block's last full group of four)",
           2: "counts include NaN pixels",
           3: "the last sample of an odd-length line is left out of the fit",
           4: "only the first stride of the fit loop runs (groups q >= threads are ignored)",
           5: "the fill uses the mean of the pair's other sample (s ^ 1)",
           6: "the last wave's partial of the fit is not added",
           7: "k_nesz_eval's odd last column takes the previous column's abscissa"}


@functools.lru_cache(maxsize=None)
def constants():
    """(XSW_NESZ_LINES, XSW_NESZ_THREADS, XSW_NESZ_F32_GROUP, XSW_NESZ_EV) read from the kernel source."""
    return tuple(source_define(n) for n in ("XSW_NESZ_LINES", "XSW_NESZ_THREADS", "XSW_NESZ_F32_GROUP", "XSW_NESZ_EV"))


def ceil_div(a, b):
    return -(-a // b)


def nesz_blocks(lines, samples):
    """csrc/xsw_lutplan.hpp: nesz_blocks, as tests/test_host_lutplan.py::test_nesz_block_rule restates it: (nb, lpb, lines of the
    last block)."""
    gx = (samples + 255) // 256
    nb = (256 * 16 + gx - 1) // gx
    nb = max(1, min(min(nb, (lines + 7) // 8), 65535))
    lpb = ceil_div(lines, nb)
    nb = ceil_div(lines, lpb)
    return nb, lpb, lines - (nb - 1) * lpb


def eval_grid(lines, samples, ev):
    """The write pass's grid: strip_grid(lines, ceil(samples / XSW_NESZ_EV)) as tests/test_host_plan.py restates it:
    (gx, gy, lines per block, lines of the last block)."""
    gx = (samples + 256 * ev - 1) // (256 * ev)
    gy = max(1, min((256 * 16 + gx - 1) // gx, min(lines, 65535)))
    rpb = ceil_div(lines, gy)
    gy = ceil_div(lines, rpb)
    return gx, gy, rpb, lines - (gy - 1) * rpb


# ---------------------------------------------------------------------------------------------------------------- reference
Ref = namedtuple("Ref", "out t x n ymax kappa1 xbar minnorm slope var")
# out [L, S] longdouble (NaN where the operation gives NaN); t [L, S] float64, the exact exponent (yhat - 1) / 10; x [S] the column
# abscissae (longdouble); per line: n fitted samples, ymax = max |y_i| over them (0 where none), kappa1 (inf on minimum-norm
# lines, NaN on NaN lines), xbar, minnorm (bool), slope and var = Sxx / n (float64; NaN off the regular lines)


def _colmean_ld(a):
    lines, samples = a.shape
    s, c = np.zeros(samples, LD), np.zeros(samples, np.int64)
    for l in range(lines):
        ok = ~np.isnan(a[l])
        s += np.where(ok, a[l], 0).astype(LD)
        c += ok
    with np.errstate(all="ignore"):
        return np.where(c > 0, s / np.maximum(c, 1).astype(LD), LD(np.nan))


def reference(noise, inc, chunk=16):
    noise, inc = np.asarray(noise), np.asarray(inc)
    assert noise.ndim == 2 and noise.shape == inc.shape and noise.dtype == inc.dtype and noise.dtype in (np.float32, np.float64)
    lines, samples = noise.shape
    nan = LD(np.nan)
    mean, x = _colmean_ld(noise), _colmean_ld(inc)
    fill = mean.astype(np.float32).astype(LD) if noise.dtype == np.float32 else mean
    out = np.full((lines, samples), nan, LD)
    t_out = np.full((lines, samples), np.nan)
    n_l, ymax = np.zeros(lines, np.int64), np.zeros(lines)
    kappa1, xbar_l, minnorm = np.full(lines, np.nan), np.full(lines, np.nan), np.zeros(lines, bool)
    slope_l, var_l = np.full(lines, np.nan), np.full(lines, np.nan)
    xnan = np.isnan(x)

    def some_lines(a):  # lines a .. a + chunk: disjoint slices of the results
        v = noise[a:a + chunk].astype(LD)
        v = np.where(np.isnan(v), fill[None, :], v)
        with np.errstate(all="ignore"):
            y = LD(10) * np.log10(v)
        ok = np.isfinite(y)
        n = ok.sum(axis=1)
        n_l[a:a + chunk] = n
        y0 = np.where(ok, y, 0)
        ymax[a:a + chunk] = np.abs(y0).max(axis=1).astype(np.float64)
        poisoned = (ok & xnan[None, :]).any(axis=1)
        for j in np.flatnonzero((n > 0) & ~poisoned):
            m = ok[j]
            xf, yf = x[m], y[j][m]
            nn = LD(int(n[j]))
            xb, yb = xf.sum() / nn, yf.sum() / nn
            if xf.max() == xf.min():
                minnorm[a + j], kappa1[a + j], xbar_l[a + j] = True, np.inf, float(xf[0])
                yhat = x * (yb / (LD(2) * xf[0])) + yb / LD(2)
            else:
                dx = xf - xb
                sxx = (dx * dx).sum()
                slope = (dx * (yf - yb)).sum() / sxx
                kappa1[a + j], xbar_l[a + j] = float(np.abs(dx).sum() / sxx), float(xb)
                slope_l[a + j], var_l[a + j] = float(slope), float(sxx / nn)
                yhat = yb + slope * (x - xb)  # == x * slope + icpt, icpt = yb - slope * xb
            t = (yhat - LD(1)) / LD(10)
            with np.errstate(all="ignore"):
                out[a + j] = np.power(LD(10), t)
            t_out[a + j] = t.astype(np.float64)

    starts = range(0, lines, chunk)
    if lines * samples > 1 << 20:  # log10l and powl dominate and run without the interpreter lock
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(some_lines, starts))
    else:
        for a in starts:
            some_lines(a)
    for arr in (out, t_out, x, n_l, ymax, kappa1, xbar_l, minnorm, slope_l, var_l):
        arr.setflags(write=False)
    return Ref(out, t_out, x, n_l, ymax, kappa1, xbar_l, minnorm, slope_l, var_l)


def kappa(ref):
    """kappa_l(s), [L, S] float64: 1 on minimum-norm lines (and wherever kappa1 is not finite)."""
    k1 = np.where(np.isfinite(ref.kappa1), ref.kappa1, 0.0)
    with np.errstate(invalid="ignore"):
        dist = np.abs(ref.x.astype(np.float64)[None, :] - np.where(np.isfinite(ref.xbar), ref.xbar, 0.0)[:, None])
    return 1.0 + np.where(np.isfinite(dist), dist, 0.0) * k1[:, None]


def centring(ref):
    """What the closed form about x0 costs, as a relative error of the output in units of 2**-52, [L, S] (module docstring):
    D * 0.2303 * |x_s - xbar| * 2 |m| (Ymax + |m slope|) / var, m = xbar - x0; 0 off the regular lines."""
    _R, T, _G, _EV = constants()
    samples = ref.x.size
    groups = samples // 2  # V = 2 for both raster types
    D = 3.0 + (2 * ceil_div(groups, T) + (samples - 2 * groups) + 6 + T // 64) / 2.0
    xf = ref.x.astype(np.float64)
    x0 = float(np.mean(xf[np.isfinite(xf)])) if np.isfinite(xf).any() else 0.0
    reg = np.isfinite(ref.slope) & (ref.var > 0)
    with np.errstate(all="ignore"):
        m = np.abs(ref.xbar - x0)
        per_line = np.where(reg, 2.0 * m * (ref.ymax + m * np.abs(ref.slope)) / ref.var, 0.0)
        dist = np.abs(xf[None, :] - np.where(reg, ref.xbar, 0.0)[:, None])
    return D * 0.2303 * np.where(np.isfinite(dist), dist, 0.0) * per_line[:, None]


def rel_error(got, ref):
    """|got - reference| / reference in longdouble, as float64; NaN where the reference is NaN."""
    with np.errstate(all="ignore"):
        return np.abs((np.asarray(got).astype(LD) - ref.out) / ref.out).astype(np.float64)


def line_error(rst_out, ref):
    """R_l: the largest relative error of the restatement on every line (0 on a NaN line)."""
    e = rel_error(rst_out, ref)
    return np.where(np.isnan(ref.out), 0.0, e).max(axis=1)


def bound(ref, dtype, R=None):
    """The relative bound of every pixel, [L, S] float64 (module docstring).  R: `line_error` of the restatement; None leaves the
    R term out (what the CPU test holds the restatement itself to, with the float32 fill and numpy's pair: the float64 row)."""
    ky = kappa(ref) * ref.ymax[:, None]
    if np.dtype(dtype) == np.float64:
        b = 1e-15 * (1.0 + 0.2303 * ky)
    else:
        b = 2.0 ** -23 * (1.0 + 1.15 * np.abs(np.where(np.isnan(ref.t), 0.0, ref.t)) + 0.345 * ky)
    b = b + 2.0 ** -52 * centring(ref)
    if R is not None:
        b = b + F * np.maximum(np.asarray(R, dtype=np.float64), 2.0 ** -52)[:, None]
    return b


def worst_ratio(got, ref, bnd):
    """(largest error / bound over EVERY pixel where the reference is finite, its (line, sample), pixels compared, the error
    there).  NaN
    positions are the caller's to compare first: a NaN of `got` at a compared pixel gives an infinite ratio."""
    finite = np.isfinite(ref.out)
    if not finite.any():
        return 0.0, (0, 0), 0, 0.0
    e = rel_error(got, ref)
    ratio = np.where(finite, np.where(np.isnan(e), np.inf, e) / bnd, 0.0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), (int(at[0]), int(at[1])), int(finite.sum()), float(e[at])


# ---------------------------------------------------------------------------------------------------------------- restatement
Restated = namedtuple("Restated", "out mean x x0 slope icpt n regular launch")
# out [L, S] float64; mean, x [S]: the column means; x0; per line slope, icpt, n (fitted samples), regular (the det test passed);
# launch: what the restated launch says (dict)
_LANE = np.arange(64)


def _butterfly(v):
    """wave_sum_d on the last axis (64 lanes): v += shfl_xor(v, off), off = 32 .. 1; lane 0's value."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ off]
    return v[..., 0]


def _colmeans(a, nb, lpb, mutate):
    lines, samples = a.shape
    tot, cnt = np.zeros(samples), np.zeros(samples, np.int64)
    for b in range(nb):
        l0, l1 = b * lpb, min(lines, (b + 1) * lpb)
        if mutate == 1:
            l1 = l0 + (l1 - l0) // 4 * 4
        acc, c = np.zeros(samples), np.zeros(samples, np.int64)
        for l in range(l0, l1):
            v = a[l].astype(np.float64)
            ok = ~np.isnan(v)
            with np.errstate(invalid="ignore"):  # inf - inf cannot occur here; inf + x is quiet
                acc = np.where(ok, acc + np.where(ok, v, 0.0), acc)
            c += 1 if mutate == 2 else ok
        tot = tot + acc
        cnt += c
    with np.errstate(all="ignore"):
        return np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan)


def _thread_order(samples, V, T, mutate):
    """idx [T, depth]: the samples a thread of k_nesz_fit takes, in its order (-1: none)."""
    groups = samples // V
    if mutate == 4:
        groups_run = min(groups, T)
    else:
        groups_run = groups
    trips = ceil_div(groups_run, T) if groups_run else 0
    tail = np.arange(groups * V, samples)
    if mutate == 3 and samples % 2 == 1:
        tail = tail[:-1]
    tail_depth = ceil_div(tail.size, T) if tail.size else 0
    idx = np.full((T, trips * V + tail_depth), -1, np.int64)
    s = np.arange(groups_run * V)
    q = s // V
    idx[q % T, (q // T) * V + s % V] = s
    k = np.arange(tail.size)
    idx[k % T, trips * V + k // T] = tail
    return idx


def restate(noise, inc, mutate=None):
    noise, inc = np.asarray(noise), np.asarray(inc)
    assert mutate is None or mutate in MUTANTS
    lines, samples = noise.shape
    R, T, G32, EV = constants()
    f32 = noise.dtype == np.float32
    V = G32 if f32 else 2
    nb, lpb, last = nesz_blocks(lines, samples)
    # k_nesz_colsum + k_nesz_colmean
    mean, x = _colmeans(noise, nb, lpb, mutate), _colmeans(inc, nb, lpb, mutate)
    # k_nesz_center: 1024 threads, strided
    CT = 1024
    trips_c = ceil_div(samples, CT)
    xp = np.full(trips_c * CT, np.nan)
    xp[:samples] = x
    xp = xp.reshape(trips_c, CT)
    s, c = np.zeros(CT), np.zeros(CT)
    for k in range(trips_c):
        fin = np.isfinite(xp[k])
        s = np.where(fin, s + np.where(fin, xp[k], 0.0), s)
        c = np.where(fin, c + 1.0, c)
    ws, wc = _butterfly(s.reshape(CT // 64, 64)), _butterfly(c.reshape(CT // 64, 64))
    ts = tc = 0.0
    for w in range(CT // 64):
        ts, tc = ts + ws[w], tc + wc[w]
    x0 = float(ts / tc) if tc > 0.0 else 0.0
    # k_nesz_fit
    col = np.arange(samples)
    other = np.where((col ^ 1) < samples, col ^ 1, col) if mutate == 5 else col
    m_fill = mean.astype(np.float32).astype(np.float64) if f32 else mean
    v = noise.astype(np.float64)
    v = np.where(np.isnan(v), m_fill[other][None, :], v)
    with np.errstate(all="ignore"):
        y = 10.0 * np.log10(v)
    ok = np.isfinite(y)
    xc = x - x0
    idx = _thread_order(samples, V, T, mutate)
    mom = [np.zeros((lines, T)) for _ in range(5)]  # n, sx, sy, sxx, sxy
    for p in range(idx.shape[1]):
        si = idx[:, p]
        have = si >= 0
        sj = np.where(have, si, 0)
        m = ok[:, sj] & have[None, :]
        xs_, ys_ = np.broadcast_to(xc[sj][None, :], m.shape), np.where(m, y[:, sj], 0.0)
        with np.errstate(invalid="ignore"):
            terms = (1.0, xs_, ys_, xs_ * xs_, xs_ * ys_)
            mom = [np.where(m, acc + term, acc) for acc, term in zip(mom, terms)]
    NW = T // 64
    waves = [_butterfly(a.reshape(lines, NW, 64)) for a in mom]  # [L, NW] each
    tot = [np.zeros(lines) for _ in range(5)]
    for w in range(NW - 1 if mutate == 6 else NW):
        tot = [a + b[:, w] for a, b in zip(tot, waves)]
    nn, ssx, ssy, ssxx, ssxy = tot
    with np.errstate(all="ignore"):
        det = nn * ssxx - ssx * ssx
        xm, ym = ssx / nn, ssy / nn
        regular = det > 1e-24 * (nn * ssxx + ssx * ssx + 1e-300)
        slope_r = (nn * ssxy - ssx * ssy) / det
        icpt_r = ym - slope_r * (xm + x0)
        slope = np.where(nn == 0.0, np.nan, np.where(regular, slope_r, ym / (2.0 * (xm + x0))))
        icpt = np.where(nn == 0.0, np.nan, np.where(regular, icpt_r, 0.5 * ym))
        # k_nesz_eval
        xe = x.copy()
        if mutate == 7 and samples % 2 == 1 and samples > 1:
            xe[samples - 1] = x[samples - 2]
        t = (xe[None, :] * slope[:, None] + icpt[:, None] - 1.0) * 0.1
        out = 10.0 ** t
    groups = samples // V
    with_sample = min(T, groups) if groups else min(T, samples - groups * V)
    launch = {"blocks": (nb, lpb, last), "fit_threads": with_sample, "fit_waves": ceil_div(with_sample, 64), "fit_trips": ceil_div(groups, T),
              "fit_tail": samples - groups * V, "center_trips": trips_c, "fit_groups_of_lines": ceil_div(lines, R), "lines_mod": lines % R,
              "eval_grid": eval_grid(lines, samples, EV), "V": V}
    return Restated(out, mean, x, x0, slope, icpt, nn.astype(np.int64), regular & (nn > 0), launch)
