"""CPU restatement of xsarsea.gradients.filtering_parameters (reference: src/xsarsea/gradients.py:758-825, Mean :724-755, smoothing
:675-686) with numpy and scipy: the test oracle of xsarsea_amd.gradients.filtering_parameters / Mean / smoothing.

R2, local_gradients and the NaN-skipping coarsen come from tests/gradients_ref.py.  What the reference's xarray calls contribute is
stated explicitly (xarray and cv2 are not installed here); scipy's own convolve2d and ndimage.zoom are called as the reference
calls them.  `zoom_linear` restates ndimage.zoom(order=1) in numpy, so that a crop of a large raster can be zoomed at its global
coordinates (scipy's mapping depends on the whole raster's shape).  Lines :822-823 of the reference (F[F < 0.0015] = 0 when F has
image_ori's shape) cannot run for a non-empty raster, F having half the shape, and are not restated.
Test infrastructure only: the product never imports it.
"""
import numpy as np
from scipy import ndimage, signal

from gradients_ref import B2, B4, R2, coarsen_coords, coarsen_mean, conv_symm, local_gradients  # noqa: F401

B22 = np.array([[1, 0, 2, 0, 1], [0, 0, 0, 0, 0], [2, 0, 4, 0, 2], [0, 0, 0, 0, 0], [1, 0, 2, 0, 1]], float) * 1 / 16
B42 = signal.convolve(B22, B22)

COEFFS = ((-50, 2.75), (-5000, 3), (-2.5, 4), (-10, 6.3))


def Mean(image):
    """convolve2d(B4, "symm") / convolve2d(ones, B4), then convolve2d(B42, "symm") / convolve2d(ones, B4) (sic: B4)."""
    image = np.asarray(image)
    x = conv_symm(image, B4)
    out = signal.convolve2d(x, B42, mode="same", boundary="symm")
    num = signal.convolve2d(np.ones_like(out), B4, mode="same", boundary="symm")
    return out / num


def smoothing(image):
    return conv_symm(np.asarray(image), B2)


def zoom_axis(n_in, n_out, out_index=None):
    """One axis of ndimage.zoom(order=1, mode="constant", grid_mode=False): (first tap, second tap, weight 0, weight 1, inside)
    of the output indices (all of them by default).  Output o reads the coordinate o * (n_in - 1) / (n_out - 1); the taps are
    floor and floor + 1 with weights 1 - t and 1 - (1 - t), t the fractional part.  The second tap of the last output lies past
    the array: scipy mirrors it to n_in - 2 (0 for a one-element axis), and it multiplies with its weight of 0.  A coordinate
    beyond n_in - 1 is outside the array (the output is cval = 0)."""
    o = np.arange(n_out) if out_index is None else np.asarray(out_index)
    z = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    cc = o.astype(np.float64) * z
    fl = np.floor(cc)
    inside = cc <= n_in - 1
    i0 = np.where(inside, fl, 0).astype(np.int64)
    i1 = np.where(i0 + 1 < n_in, i0 + 1, n_in - 2 if n_in > 1 else 0)
    w0 = 1.0 - (cc - fl)
    w1 = 1.0 - w0
    return i0, i1, w0, w1, inside


def zoom_linear(a, out_shape, rows=None, cols=None, origin=(0, 0), in_shape=None):
    """ndimage.zoom(full, (out_shape[0] / n0, out_shape[1] / n1), order=1) at the output rows / cols (all by default).  `a` is the
    full input, or its crop starting at `origin` of a full input of `in_shape` (every tap must then fall inside the crop).
    scipy's order of the four taps: ((a00 wy0) wx0 + (a01 wy0) wx1) + (a10 wy1) wx0 + (a11 wy1) wx1."""
    a = np.asarray(a, dtype=np.float64)
    n0, n1 = a.shape if in_shape is None else in_shape
    y0, y1, wy0, wy1, iny = zoom_axis(n0, out_shape[0], rows)
    x0, x1, wx0, wx1, inx = zoom_axis(n1, out_shape[1], cols)
    y0, y1, x0, x1 = y0 - origin[0], y1 - origin[0], x0 - origin[1], x1 - origin[1]
    for idx, n in ((y0, a.shape[0]), (y1, a.shape[0]), (x0, a.shape[1]), (x1, a.shape[1])):
        assert idx.min() >= 0 and idx.max() < n, "a tap falls outside the crop"
    wy0, wy1 = wy0[:, None], wy1[:, None]
    with np.errstate(invalid="ignore"):
        out = a[np.ix_(y0, x0)] * wy0 * wx0
        out = out + a[np.ix_(y0, x1)] * wy0 * wx1
        out = out + a[np.ix_(y1, x0)] * wy1 * wx0
        out = out + a[np.ix_(y1, x1)] * wy1 * wx1
    return np.where(iny[:, None] & inx[None, :], out, 0.0)


def terms(image_ori):
    """The rasters filtering_parameters combines: r2, G3, c, J, J1, G4 (half resolution) and q4 = smoothing(coarsen(r2))."""
    with np.errstate(invalid="ignore"):
        image = np.sqrt(np.asarray(image_ori))  # in the input's dtype; negative -> NaN
    r2 = R2(image)
    _g2, G3, c = local_gradients(image)
    return dict(r2=r2, G3=G3, c=c, J=Mean(r2), J1=Mean(r2 ** 2), G4=Mean(G3), q4=smoothing(coarsen_mean(r2, 2)))


def combine(t, Z):
    """(f1, f2, f3, f4, F, d, J1) from `terms` and Z = zoom(q4) on r2's grid."""
    with np.errstate(invalid="ignore", divide="ignore"):
        J, J1 = t["J"], t["J1"]
        d = J1 - J ** 2
        P = [np.sqrt(d) / (J + 0.00001), (t["r2"] - Z) ** 2 / ((J ** 2) + 0.00001), t["G3"] / (t["G4"] + 0.00001), np.sqrt(t["c"])]
        f = [np.clip(a * p + b, 0, 1) for (a, b), p in zip(COEFFS, P)]
        F = np.sqrt(1 / 4.0 * (f[0] ** 2 + f[1] ** 2 + f[2] ** 2 + f[3] ** 2))
    return f[0], f[1], f[2], f[3], F, d, J1


def filtering_parameters(image_ori):
    """(f1, f2, f3, f4, F, d, J1): the five rasters of the reference, then d = J1 - J**2 (whose sign decides f1's NaN) and J1."""
    t = terms(image_ori)
    r2, q4 = t["r2"], t["q4"]
    # the reference's own expression: an axis below 4 pixels leaves q4 empty and the zoom factor divides by zero
    Z = ndimage.zoom(q4, (r2.shape[0] / q4.shape[0], r2.shape[1] / q4.shape[1]), order=1)
    return combine(t, Z)


def rain_scene(shape, dtype, seed, gamma=20, land=True):
    """The sigma0 scene of tests/test_gpu_gradients.py (structure, gamma speckle of the given shape parameter, NaN land patches)
    with six Gaussian blobs multiplied in (amplitude x1.5 .. x4, radius 4 .. 20 px): rain cells and ships."""
    rng = np.random.default_rng(seed)
    L, S = shape
    y, x = np.mgrid[0:L, 0:S].astype(np.float64)
    s0 = 0.05 * (1.2 + np.sin(x / 23.0 + 0.4 * np.cos(y / 41.0)) * np.cos(y / 17.0)) * rng.gamma(gamma, 1 / gamma, shape)
    for amp, rad in zip(np.linspace(1.5, 4.0, 6), rng.permutation(np.linspace(4.0, 20.0, 6))):
        cy, cx = rng.uniform(0.1, 0.9) * L, rng.uniform(0.1, 0.9) * S
        s0 *= 1 + (amp - 1) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * rad ** 2))
    if land:
        s0[: L // 5, S - S // 6:] = np.nan
        s0[(y - 0.6 * L) ** 2 + (x - 0.3 * S) ** 2 < (0.08 * min(L, S)) ** 2] = np.nan
        s0[L // 2, S // 3] = np.nan
    return s0.astype(dtype)


# every (shape, dtype, seed, gamma) scene the GPU tests compare on; tests/test_filtering_cpu.py asserts `conditions` on each
GPU_SCENES = [(shape, dtype, seed, gamma) for shape, seed, gamma in (((203, 317), 21, 20), ((402, 515), 22, 100))
              for dtype in (np.float32, np.float64)]
FULL_TILE = ((2000, 2000), np.float32, 24, 20)


def full_tile():
    """The 2000 x 2000 scene the 20000 x 20000 GPU raster tiles 10 x 10: FULL_TILE rolled by half its side, which moves the land
    off the tile's corners (the corners of the full raster are compared)."""
    shape, dtype, seed, gamma = FULL_TILE
    return np.roll(rain_scene(shape, dtype, seed, gamma), (shape[0] // 2, shape[1] // 2), axis=(0, 1))


def conditions(f1, f2, f3, f4, F, d, J1):
    """The three conditions that keep a comparison on this scene honest: (share of ill-conditioned pixels among the finite
    ones, where d <= 1e-9 J1 and the sign of d is rounding noise; the smallest share over f1..f4 of finite pixels inside the
    ramp 0 < f < 1; the share of finite outputs).  Required: <= 0.001, >= 0.05, >= 0.8."""
    fin = np.isfinite(J1)
    ill = fin & (d <= 1e-9 * J1)
    ramps = []
    for f in (f1, f2, f3, f4):
        m = np.isfinite(f)
        ramps.append(((f[m] > 0) & (f[m] < 1)).mean())
    finite = np.mean([np.isfinite(f).mean() for f in (f1, f2, f3, f4, F)])
    return ill.sum() / max(fin.sum(), 1), min(ramps), finite, ramps
