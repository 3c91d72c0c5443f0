"""CPU restatement of xsarsea.gradients (Koch 2004) with numpy, scipy and pandas: the test oracle of xsarsea_amd.gradients.

Written from the reference's semantics (src/xsarsea/gradients.py), with the behaviour its xarray / cv2 calls contribute
stated explicitly (neither package is installed here):
  - R2: scipy convolve2d(B4, "symm") / convolve2d(ones, B4), xarray coarsen(2 x 2, trim).mean() = NaN-skipping mean,
    convolve2d(B2, "symm") / convolve2d(ones, B2)
  - cv2.Scharr(CV_64F): BORDER_REFLECT_101, separable row filter then column filter, every tap multiplying
  - cv2.resize(INTER_AREA) at an integer factor: the f x f box mean (float64 sums in row-major order, times 1 / f^2, back to the
    input's dtype)
  - rolling(center=True).construct: rows i - w//2 .. i - w//2 + w - 1, NaN outside the raster
  - .sel(method="nearest"): pandas get_indexer(method="nearest")
  - gradient_histogram as written, except that bin n_angles folds onto bin 0 (the reference raises IndexError there)
Test infrastructure only: the product never imports it.
"""
import warnings

import numpy as np
import pandas as pd
from scipy import signal

B2 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], float) * 1 / 16
B4 = signal.convolve(B2, B2)


def angles_bins(n_angles=72):
    b = np.linspace(-np.pi / 2, np.pi / 2, n_angles + 1)
    return (b[1:] + b[:-1]) / 2


def conv_symm(image, kernel):
    out = signal.convolve2d(image, kernel, mode="same", boundary="symm")
    num = signal.convolve2d(np.ones_like(out), kernel, mode="same", boundary="symm")
    return out / num


def coarsen_mean(a, f=2):
    """xarray coarsen({line: f, sample: f}, boundary="trim").mean(): float / complex -> NaN-skipping mean."""
    L, S = a.shape[0] // f, a.shape[1] // f
    blocks = a[:L * f, :S * f].reshape(L, f, S, f)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(blocks, axis=(1, 3))


def coarsen_coords(c, f):
    c = np.asarray(c)
    n = (len(c) // f) * f
    return c[:n].reshape(-1, f).mean(axis=1)


def R2(image):
    x = conv_symm(np.asarray(image), B4)
    x = coarsen_mean(x, 2)
    return conv_symm(x, B2)


def area(sigma0, f):
    """cv2.resize(..., INTER_AREA) at integer factor f: box mean, trimmed, the input's dtype."""
    if f == 1:
        return sigma0
    L, S = sigma0.shape[0] // f, sigma0.shape[1] // f
    b = sigma0[:L * f, :S * f].reshape(L, f, S, f).astype(np.float64)
    s = np.zeros((L, S))
    for i in range(f):
        for j in range(f):
            s = s + b[:, i, :, j]
    return (s * (1.0 / (f * f))).astype(sigma0.dtype)


def scharr(a):
    """(dx, dy) of cv2.Scharr(a, CV_64F, 1, 0) / (0, 1) with BORDER_REFLECT_101 (numpy's "reflect")."""
    p = np.pad(np.asarray(a, np.float64), 1, mode="reflect")
    hx = -1.0 * p[:, :-2] + 0.0 * p[:, 1:-1] + 1.0 * p[:, 2:]
    hy = 3.0 * p[:, :-2] + 10.0 * p[:, 1:-1] + 3.0 * p[:, 2:]
    dx = 3.0 * hx[:-2] + 10.0 * hx[1:-1] + 3.0 * hx[2:]
    dy = -1.0 * hy[:-2] + 0.0 * hy[1:-1] + 1.0 * hy[2:]
    return dx, dy


def local_gradients(ampl):
    """(G2, G3, c) of local_gradients: G2 = sqrt(R2(grad**2)), G3 = R2(|grad**2|), c = |R2(grad**2)| / (G3 + 1e-5), 0 above 1
    or NaN."""
    dx, dy = scharr(ampl)
    grad = dx + 1j * dy
    grad12 = grad ** 2
    grad2 = R2(grad12)
    grad3 = R2(np.abs(grad12))
    with np.errstate(invalid="ignore"):
        c = np.abs(grad2) / (grad3 + 0.00001)
        c = np.where(c <= 1, c, 0.0)
    return np.sqrt(grad2), grad3, c


def gradient_histogram(g2, c, angles_bins, fold=True):
    """The reference's gradient_histogram; fold: bin len(angles_bins) goes to bin 0 (the port's deviation).  Returns
    (grads, used_ratio, ambiguous_weight): the last is the part of grads from pixels whose angle lies within 1e-9 rad of a bin
    edge (their bin may differ by one between two correct float64 evaluations of the angle)."""
    count = g2.size
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        angle = np.angle(g2)
        angles_step = angles_bins[1] - angles_bins[0]
        angles_start = angles_bins[0]
        k_all = np.round((angle - angles_start) / angles_step)
        grads = np.zeros_like(angles_bins, dtype=np.float64)
        abs_g2 = np.abs(g2)
        mask = ~np.isnan(abs_g2) & (abs_g2 > 0)
        abs_g2 = abs_g2[mask]
        c = c[mask]
        g2 = g2[mask]
        k_all = k_all[mask]
        angle = angle[mask]
        r = abs_g2 / (abs_g2 + np.median(abs_g2))
        grads_all = r * c
        mask = ~np.isnan(k_all) & ~np.isnan(grads_all)
        grads_all = grads_all[mask]
        k_all = k_all[mask].astype(np.int64)
        angle = angle[mask]
    if fold:
        k_all[k_all == len(angles_bins)] = 0
    np.add.at(grads, k_all, grads_all)
    u = (angle - angles_start) / angles_step
    edge_dist = np.abs(u - (np.floor(u) + 0.5)) * angles_step
    amb = float(grads_all[edge_dist < 1e-9].sum())
    return grads, g2.size / count, amb


def window_pixels(window_size, line, sample):
    return int(np.mean(tuple(window_size / np.unique(np.diff(ax))[0] for ax in [line, sample])))


def nearest(index, target):
    return pd.Index(np.asarray(index)).get_indexer(np.asarray(target), method="nearest")


def rolling_window(a, i, j, w):
    """xarray rolling({line: w, sample: w}, center=True).construct(...) at (i, j): NaN outside the raster."""
    out = np.full((w, w), np.nan, dtype=a.dtype) if np.iscomplexobj(a) else np.full((w, w), np.nan)
    r0, c0 = i - w // 2, j - w // 2
    ra, rb, ca, cb = max(r0, 0), min(r0 + w, a.shape[0]), max(c0, 0), min(c0 + w, a.shape[1])
    if rb > ra and cb > ca:
        out[ra - r0:rb - r0, ca - c0:cb - c0] = a[ra:rb, ca:cb]
    return out


def lg_of(sigma0, line, sample, factor=1):
    """(G2, c, lg_line, lg_sample, resampled line, resampled sample) of one (pol, factor) raster."""
    s = area(sigma0, factor)
    if factor > 1:
        line, sample = coarsen_coords(line, factor), coarsen_coords(sample, factor)
    ampl = np.sqrt(R2(s))
    g2, _g3, c = local_gradients(ampl)
    return g2, c, coarsen_coords(coarsen_coords(line, 2), 2), coarsen_coords(coarsen_coords(sample, 2), 2), line, sample


def histogram(sigma0, line, sample, windows_sizes=(1600,), downscales_factors=(1,), window_step=1, windows_at=None,
              n_angles=72):
    """Gradients(sigma0 (2-D), ...).histogram restated: (weight [df, ws, line, sample, angles], used_ratio, ambiguous
    [df, ws, line, sample] (weight of the near-edge pixels, already divided by w*w), windows_at)."""
    bins = angles_bins(n_angles)
    fields = [lg_of(sigma0, line, sample, f) for f in downscales_factors]
    if windows_at is None:
        _, _, _, _, l0, s0 = fields[0]
        step = int(window_pixels(windows_sizes[0], l0, s0) * window_step)
        windows_at = {"line": l0[::step], "sample": s0[::step]}
    wl, ws_ = np.asarray(windows_at["line"]), np.asarray(windows_at["sample"])
    W = np.zeros((len(downscales_factors), len(windows_sizes), len(wl), len(ws_), n_angles))
    R = np.zeros(W.shape[:-1])
    A = np.zeros(W.shape[:-1])
    for a, (g2, c, lgl, lgs, _, _) in enumerate(fields):
        rows, cols = nearest(lgl, wl), nearest(lgs, ws_)
        for b, wsz in enumerate(windows_sizes):
            w = window_pixels(wsz, lgl, lgs)
            for i, r in enumerate(rows):
                for j, q in enumerate(cols):
                    h, u, amb = gradient_histogram(rolling_window(g2, r, q, w), rolling_window(c, r, q, w), bins)
                    W[a, b, i, j] = h / (w * w)
                    R[a, b, i, j] = 0.0 if np.isnan(u) else u
                    A[a, b, i, j] = amb / (w * w)
    return W, R, A, windows_at


def circ_smooth(hist):
    """circ_smooth along the last axis: wrap-pad 17, scipy.signal.convolve(mode="same") with Bx, Bx2, Bx4, Bx8, unpad."""
    Bs = [np.array(k, float) / 4 for k in ([1, 2, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 2, 0, 0, 0, 1],
                                           [1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1])]
    pad = max(len(B) for B in Bs)
    h = np.asarray(hist, float)
    x = np.concatenate([h[..., -pad:], h, h[..., :pad]], axis=-1)
    for B in Bs:
        x = np.apply_along_axis(lambda v: signal.convolve(v, B, mode="same"), -1, x)
    return x[..., pad:-pad]


def streak_scene(shape, thetas, rng, wavelength=12.0, speckle=0.05, land=None):
    """sigma0 with stripes whose gradient direction is theta (rad, anticlockwise from the sample axis) in each quadrant of the
    scene (thetas: 4 angles: top-left, top-right, bottom-left, bottom-right), multiplicative speckle, NaN land patches."""
    L, S = shape
    y, x = np.mgrid[0:L, 0:S].astype(np.float64)
    out = np.empty(shape)
    for k, th in enumerate(thetas):
        ys = slice(0, L // 2) if k < 2 else slice(L // 2, L)
        xs = slice(0, S // 2) if k % 2 == 0 else slice(S // 2, S)
        phase = (x[ys, xs] * np.cos(th) + y[ys, xs] * np.sin(th)) * 2 * np.pi / wavelength
        out[ys, xs] = 0.1 * (1 + 0.3 * np.sin(phase))
    out *= rng.gamma(1 / speckle ** 2, speckle ** 2, shape) if speckle else 1.0
    if land is not None:
        out[land] = np.nan
    return out
