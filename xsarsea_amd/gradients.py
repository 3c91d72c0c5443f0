"""Wind-streak direction histograms (Koch 2004) on the GPU: port of `xsarsea.gradients` (reference: src/xsarsea/gradients.py).

    sigma0 -> [f x f box mean] -> ampl = sqrt(R2(sigma0)) -> local_gradients(ampl) -> per-window gradient_histogram

and the rain / heterogeneity mask of the same module, `filtering_parameters(sigma0)` -> (f1, f2, f3, f4, F) in [0, 1] on the
half-resolution grid, with its helpers `Mean` and `smoothing`.  `Gradients(..., min_F=, mask=)` applies it (and / or a user's
mask on the sigma0 grid) to the histograms: a masked-out pixel of the local-gradients grid behaves exactly as a NaN G2 (`keep_mask`,
`gradient_histogram(..., keep=)`); the reference computes F and stops there, so this step is this package's own.

`Gradients(sigma0, windows_sizes, downscales_factors, window_step).histogram` is the notebook's entry point; `Gradients2D` is the
mono-pol, single-window-size class it stacks.  The raster passes and the per-window histograms run in HIP kernels
(csrc/xsw_gradients.hip, include/xsw.h: xsw_grad_*); window geometry is host arithmetic that copies the reference's expressions.

Containers (neither xarray nor cv2 is needed): `sigma0` is a 2-D (line, sample) -- or 3-D (pol, line, sample) for `Gradients` --
numpy array, a device tensor, or any object with `.values` and `.line` / `.sample` coordinates (an xarray.DataArray).  Coordinates
come from the object, else from the `line=` / `sample=` keywords, else np.arange.  Numpy in gives numpy out; a device tensor in gives
device tensors out, computed asynchronously on the caller's current stream.

One deliberate deviation: a pixel whose G2 is a negative real with +0 imaginary part has angle +pi/2, bin index n_angles; the
reference's np.add.at raises IndexError there, this port folds it onto bin 0 (pi/2 == -pi/2 modulo pi).  See DESIGN.md.
"""
import numpy as np

from . import _device, _lib
from ._raster import _as_u8, _Call, _coord_values, _is_tensor, _Raster, _u8_kind, _unwrap

__all__ = ["Gradients", "Gradients2D", "GradientsHistogram", "local_gradients", "R2", "gradient_histogram", "circ_smooth",
           "angles_bins", "filtering_parameters", "Mean", "smoothing", "keep_mask"]


def angles_bins(n_angles=72):
    """Bin centres: the midpoints of linspace(-pi/2, pi/2, n_angles + 1) (gradients.py:93-97)."""
    b = np.linspace(-np.pi / 2, np.pi / 2, n_angles + 1)
    return (b[1:] + b[:-1]) / 2


# ------------------------------------------------------------------------------------------------------ host geometry
def coarsen_coords(coords, factor):
    """Coordinates of a factor-f reduction with the remainder trimmed: the means of the groups (xarray coarsen(...).mean(),
    Gradients._sigma0_resample.compute_coords)."""
    coords = np.asarray(coords)
    n = (len(coords) // factor) * factor
    return coords[:n].reshape(-1, factor).mean(axis=1)


def window_pixels(window_size, line, sample):
    """Window size in pixels of a grid: int(mean(window_size / smallest coordinate step)) over both axes (gradients.py:146-150,
    :169-177)."""
    return int(np.mean(tuple(window_size / np.unique(np.diff(np.asarray(ax)))[0] for ax in (line, sample))))


def nearest_indexer(index, target):
    """pandas.Index(index).get_indexer(target, method="nearest") for an ascending index: the nearest position, a tie going to the
    larger coordinate (gradients.py:198, `.sel(..., method="nearest")`)."""
    index, target = np.asarray(index), np.asarray(target)
    right = np.searchsorted(index, target, side="left")        # first index >= target ('backfill'), len: none
    left = np.searchsorted(index, target, side="right") - 1    # last index <= target ('pad'), -1: none
    right_m = np.where(right == len(index), -1, right)
    left_dist = np.abs(index[left] - target)
    right_dist = np.abs(index[right_m] - target)
    return np.where((left_dist < right_dist) | (right_m == -1), left, right_m)


# ------------------------------------------------------------------------------------------------------ device calls
def _area(values, factor):
    """f x f box mean of a 2-D raster, the input's dtype (float32 / float64) kept (xsw_grad_area)."""
    call = _Call(values)
    x = call.prep(values)
    L, S = x.shape
    out = call.empty((L // factor, S // factor), np.float32 if call.xsw_dtype(x) == _lib.XSW_F32 else np.float64)
    call.launch("grad_area_raw", L, S, factor, call.xsw_dtype(x), call.mem, x, out)
    return out


def _r2(values, take_sqrt):
    call = _Call(values)
    x = call.prep(values)
    if x.ndim != 2:
        raise ValueError("R2 needs a 2-D raster")
    L, S = x.shape
    if L < 2 or S < 2:
        raise ValueError("R2 needs at least 2 x 2 pixels")
    out = call.empty((L // 2, S // 2), np.float64)
    call.launch("grad_r2_raw", L, S, call.xsw_dtype(x), call.mem, take_sqrt, x, out)
    return out


def _local(ampl):
    call = _Call(ampl)
    x = call.prep(ampl, np.float64)
    if x.ndim != 2:
        raise ValueError("local_gradients needs a 2-D raster")
    L, S = x.shape
    if L < 2 or S < 2:
        raise ValueError("local_gradients needs at least 2 x 2 pixels")
    shape = (L // 2, S // 2)
    g2, g3, c = call.empty(shape, np.complex128), call.empty(shape, np.float64), call.empty(shape, np.float64)
    call.launch("grad_local_raw", L, S, call.mem, x, g2, g3, c)
    return g2, g3, c


def _checked_keep(keep, g2):
    """keep (or None) after the host checks: a bool / uint8 array of g2's shape."""
    if keep is not None:
        if tuple(keep.shape) != tuple(np.shape(g2)):
            raise ValueError(f"keep {tuple(keep.shape)} must have g2's shape {tuple(np.shape(g2))}")
        if _u8_kind(keep) != "u8":
            raise TypeError(f"keep must be bool or uint8, not {keep.dtype}")
    return keep


def _hist(g2, c, window, rows, cols, n_angles, bins=None, normalise=True, keep=None):
    """Bin sums [rows, cols, n_angles] (divided by the window's pixel count with `normalise`, as an IEEE division on the device
    whatever the route) and used ratios [rows, cols] of the windows centred at (rows[a], cols[b]).  keep: bool / uint8 array of
    g2's shape, 0 = the pixel behaves as a NaN g2 (xsw_grad_hist_masked); None: the unmasked kernel."""
    call = _Call(g2, c, _checked_keep(keep, g2))
    g2, c = call.prep(g2, np.complex128), call.prep(c, np.float64)
    L, S = g2.shape
    if c.shape != g2.shape:
        raise ValueError("g2 and c must have one shape")
    wl, ws = (window, window) if np.isscalar(window) else window
    bins = angles_bins(n_angles) if bins is None else np.asarray(bins, dtype=np.float64)
    rows = call.prep(np.asarray(rows, dtype=np.int32), np.int32)
    cols = call.prep(np.asarray(cols, dtype=np.int32), np.int32)
    nr, nc = rows.shape[0], cols.shape[0]
    weight, ratio = call.empty((nr, nc, len(bins)), np.float64), call.empty((nr, nc), np.float64)
    if nr and nc:
        masked = () if keep is None else (_as_u8(call, keep),)
        call.launch("grad_hist_raw" if keep is None else "grad_hist_masked_raw", L, S, call.mem, g2, c, *masked, wl, ws, nr, rows, nc, cols,
                    len(bins), bins[0], bins[1] - bins[0], normalise, weight, ratio)
    return weight, ratio


# --------------------------------------------------------------------------------------------------- public functions
def R2(image):
    """Reduce a 2-D real raster by a factor 2 with no moire effect (gradients.py:689-722): B4 smoothing ("symm" border),
    NaN-skipping 2 x 2 mean (the remainder trimmed), B2 smoothing.  float64 (lines // 2, samples // 2), same container kind as
    `image` (numpy or device tensor); the coarse coordinates are `coarsen_coords(coords, 2)`."""
    values = _Raster(image).values
    return _r2(values, False)


class LocalGradients:
    """local_gradients' result (the reference's Dataset of G2, G3, c): attribute or item access."""

    def __init__(self, G2, G3, c, line=None, sample=None):
        self.G2, self.G3, self.c, self.line, self.sample = G2, G3, c, line, sample

    def __getitem__(self, name):
        return getattr(self, name)


def local_gradients(image, line=None, sample=None):
    """Local gradients of a 2-D amplitude raster (gradients.py:588-634): G2 = sqrt(R2(grad**2)) (complex128; its angle is the
    gradient direction in [-pi/2, pi/2]), G3 = R2(|grad**2|), c = |R2(grad**2)| / (G3 + 1e-5) set to 0 above 1 or where NaN,
    grad = Scharr_x + 1j * Scharr_y.  All on the (lines // 2, samples // 2) grid, whose coordinates are the means of pairs."""
    r = _Raster(image, line, sample)
    g2, g3, c = _local(r.values)
    return LocalGradients(g2, g3, c, coarsen_coords(r.line, 2), coarsen_coords(r.sample, 2))


# ------------------------------------------------------------------------------------- rain / heterogeneity mask
def _same_shape_filter(image, fn_name):
    """Mean / smoothing: a 2-D raster through one same-shape float64 kernel."""
    call = _Call(image)
    x = call.prep(image, np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{fn_name} needs a non-empty 2-D raster")
    L, S = x.shape
    out = call.empty((L, S), np.float64)
    if fn_name == "Mean":
        call.launch("grad_mean_raw", L, S, call.mem, x, out)
    else:
        call.launch("grad_smooth_raw", L, S, call.mem, False, x, out)
    return out


def Mean(image):
    """Local mean operator (gradients.py:724-755): B4 smoothing then B42 (B4 dilated by 2, 9 x 9), both with the "symm"
    border.  B42's zero taps multiply as in scipy's sum: one NaN makes its 9 x 9 footprint NaN.  float64, the input's shape
    and container kind."""
    return _same_shape_filter(_Raster(image).values, "Mean")


def smoothing(image):
    """3 x 3 B2 smoothing with the "symm" border (gradients.py:675-686).  float64, the input's shape and container kind."""
    return _same_shape_filter(_Raster(image).values, "smoothing")


class FilteringParameters(tuple):
    """filtering_parameters' result: the reference's 5-tuple (f1, f2, f3, f4, F), which also carries the coordinates of
    the half-resolution grid as `.line` / `.sample` and the rasters by name."""

    def __new__(cls, f1, f2, f3, f4, F, line=None, sample=None):
        self = super().__new__(cls, (f1, f2, f3, f4, F))
        self.f1, self.f2, self.f3, self.f4, self.F, self.line, self.sample = f1, f2, f3, f4, F, line, sample
        return self


def filtering_parameters(image_ori, line=None, sample=None):
    """Koch filters of a 2-D sigma0 raster (gradients.py:758-825): (f1, f2, f3, f4, F), each float64 in [0, 1] (NaN where the
    input's NaN reaches) on the (lines // 2, samples // 2) grid; 0 flags heterogeneous sigma0 (rain cells, ships, land edges,
    fronts).  With ampl = sqrt(sigma0) (in the input's dtype), r2 = R2(ampl) and G3, c of local_gradients(ampl):
    f1 from the local standard deviation over mean of r2, f2 from r2 minus its quarter-resolution smoothing zoomed back
    (scipy.ndimage.zoom, order 1), f3 from G3 / Mean(G3), f4 from sqrt(c), F = sqrt(mean(f_i**2)).  sqrt(sigma0) is taken
    inside the kernels; no full-resolution temporary is made.  Needs at least 4 x 4 pixels (ValueError below that: the
    quarter-resolution raster would be empty)."""
    r = _Raster(image_ori, line, sample)
    L, S = r.values.shape
    if L < 4 or S < 4:  # the reference divides by the empty quarter-resolution raster's axis length there
        raise ValueError(f"filtering_parameters needs at least 4 x 4 pixels, not {L} x {S}")
    call = _Call(r.values)
    x = call.prep(r.values)
    L2, S2 = L // 2, S // 2
    dt = call.xsw_dtype(x)
    r2, g3, c = (call.empty((L2, S2), np.float64) for _ in range(3))
    q4 = call.empty((L2 // 2, S2 // 2), np.float64)
    out = call.empty((5, L2, S2), np.float64)
    call.launch("grad_r2_sqrt_raw", L, S, dt, call.mem, x, r2)
    call.launch("grad_local_sqrt_raw", L, S, dt, call.mem, x, None, g3, c)
    call.launch("grad_smooth_raw", L2, S2, call.mem, True, r2, q4)
    call.launch("grad_filter_raw", L2, S2, call.mem, r2, g3, c, q4, out)
    return FilteringParameters(out[0], out[1], out[2], out[3], out[4], coarsen_coords(r.line, 2), coarsen_coords(r.sample, 2))


def keep_mask(values, threshold=None, block=2, and_with=None):
    """Reduce a 2-D raster to a uint8 keep mask by block x block blocks, the remainder trimmed: out[i, j] = 1 iff every input of
    the block is usable (xsw_grad_keep_f64 / xsw_grad_keep_u8).  Floating `values` (widened to float64) need `threshold`: usable
    iff x >= threshold, an IEEE comparison, so NaN is never usable.  bool / uint8 `values` take no threshold: usable iff
    non-zero.  `and_with`: a bool / uint8 mask on the OUTPUT grid, AND-ed in.  The result, (lines // block, samples // block), is
    of the input's container kind: numpy, or a device tensor computed on the caller's current stream.

    block = 2 takes `filtering_parameters(sigma0).F` to the local-gradients grid of the same sigma0; block = 4 f takes a mask on
    the sigma0 grid to the local-gradients grid at downscale factor f.  For a threshold on F see `Gradients`' `min_F`: F sits on
    plateaus, choose the threshold between them."""
    values = _unwrap(values)
    if not _is_tensor(values):
        values = np.asarray(values)
    if len(values.shape) != 2:
        raise ValueError(f"keep_mask needs a 2-D raster, not {len(values.shape)}-D")
    kind = _u8_kind(values)
    if kind == "float" and threshold is None:
        raise ValueError("a floating raster needs a threshold (usable iff x >= threshold)")
    if kind == "u8" and threshold is not None:
        raise ValueError("a bool / uint8 raster takes no threshold (usable iff non-zero)")
    if threshold is not None and np.isnan(float(threshold)):
        raise ValueError("the threshold is NaN")
    block = int(block)
    if block < 1:
        raise ValueError(f"block must be at least 1, not {block}")
    L, S = (int(v) for v in values.shape)
    Lo, So = L // block, S // block
    if Lo < 1 or So < 1:
        raise ValueError(f"a {L} x {S} raster has no {block} x {block} block")
    if and_with is not None:
        if tuple(and_with.shape) != (Lo, So):
            raise ValueError(f"and_with {tuple(and_with.shape)} must be on the output grid ({Lo}, {So})")
        if _u8_kind(and_with) != "u8":
            raise TypeError(f"and_with must be bool or uint8, not {and_with.dtype}")
    call = _Call(values, and_with)
    x = call.prep(values, np.float64) if kind == "float" else _as_u8(call, values)
    aw = None if and_with is None else _as_u8(call, and_with)
    out = call.empty((Lo, So), np.uint8)
    thr = None if kind == "u8" else float(threshold)
    call.launch("grad_keep_raw", L, S, call.mem, x, thr, block, aw, out)
    return out


def _check_bins(call, g2, c, bins, keep=None):
    """IndexError, as the reference's np.add.at raises it, when a pixel that would be summed falls outside numpy's index range
    -n .. n - 1 (bin n is the documented fold onto bin 0).  Only a g2 that is not a principal square root can do that (G2 from
    local_gradients never does).  Pixels masked out by `keep` are not summed and cannot raise.  Device input: one synchronising
    check."""
    n, start, step = len(bins), float(bins[0]), float(bins[1] - bins[0])
    if call.device:
        t = call.torch
        a, cc = g2.abs(), call.prep(c, np.float64)
        k = t.round((t.angle(g2) - start) / step)  # round half to even, as numpy's
        bad = t.isfinite(a) & (a > 0) & ~t.isnan(cc) & ((k > n) | (k < -n))
        if keep is not None:
            bad &= _as_u8(call, keep) != 0
        first = int(k[bad][0].item()) if bool(bad.any()) else None
    else:
        a, cc = np.abs(g2), np.asarray(c, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            k = np.round((np.angle(g2) - start) / step)
            bad = np.isfinite(a) & (a > 0) & ~np.isnan(cc) & ((k > n) | (k < -n))
        if keep is not None:
            bad &= _as_u8(call, keep) != 0
        first = int(k[bad][0]) if bad.any() else None
    if first is not None:
        raise IndexError(f"index {first} is out of bounds for axis 0 with size {n}")


def gradient_histogram(g2, c, angles_bins, keep=None):
    """Direction histogram of ONE box (gradients.py:828-879): (bin sums [len(angles_bins)], used ratio).  Each pixel whose |g2|
    is not NaN and > 0 adds |g2| / (|g2| + median|g2|) * c into bin rint((angle(g2) - angles_bins[0]) / step).  Bin
    len(angles_bins) (angle +pi/2) is folded onto bin 0 where the reference raises IndexError; any other index outside
    numpy's range raises IndexError as the reference does.  keep (bool / uint8, g2's shape; this package's own): a pixel whose
    keep is 0 behaves exactly as if its g2 were NaN -- not kept, outside the median, in no bin, not counted in the used ratio's
    numerator (the denominator stays g2.size)."""
    if len(np.shape(g2)) != 2:
        raise ValueError("g2 must be 2-D")
    if np.shape(c) != tuple(np.shape(g2)):
        raise ValueError("g2 and c must have one shape")
    call = _Call(g2, c, _checked_keep(keep, g2))
    g2 = call.prep(g2, np.complex128)
    _check_bins(call, g2, c, np.asarray(angles_bins, dtype=np.float64), keep)
    L, S = g2.shape
    weight, ratio = _hist(g2, c, (L, S), [L // 2], [S // 2], len(angles_bins), angles_bins, normalise=False, keep=keep)
    return weight[0, 0], ratio[0, 0]


_SMOOTHERS = [np.array(k, float) / 4 for k in ([1, 2, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 2, 0, 0, 0, 1],
                                              [1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1])]


def circ_smooth(hist, axis=-1):
    """Smooth histograms along their angles axis with Bx, Bx2, Bx4, Bx8 in that order, circularly (gradients.py:882-923: the
    reference pads 17 bins by wrapping, more than the cumulative reach of 15, so its result is exactly circular).  numpy in
    gives numpy out, a device tensor gives a device tensor (torch ops, the caller's stream)."""
    if _is_tensor(hist):
        import torch
        x = _device.as_tensor(hist, _device.device_of(hist)).double()
        roll, zeros = torch.roll, torch.zeros_like
    else:
        x = np.asarray(hist, dtype=np.float64)
        roll, zeros = np.roll, np.zeros_like
    for B in _SMOOTHERS:
        h = len(B) // 2
        out = zeros(x)
        for j, b in enumerate(B):  # out[i] = sum_j B[j] * x[i + j - h]
            out = out + float(b) * roll(x, h - j, axis)
        x = out
    return x


# ------------------------------------------------------------------------------------------------------------ classes
class GradientsHistogram:
    """Result of `.histogram` (the reference's xarray.Dataset, field and axis names kept):
    weight [pol?, downscale_factor, window_size, line, sample, angles] (Gradients) or [line, sample, angles] (Gradients2D),
    used_ratio without the angles axis, and the coordinate vectors.  `pol` is present only when the input had it."""

    def __init__(self, weight, used_ratio, angles, line, sample, dims, **coords):
        self.weight, self.used_ratio, self.angles, self.line, self.sample, self.dims = weight, used_ratio, angles, line, sample, dims
        self.window_size = coords.get("window_size")
        self.downscale_factor = coords.get("downscale_factor")
        self.pol = coords.get("pol")

    def __getitem__(self, name):
        return getattr(self, name)


class _Field:
    """One (pol, downscale factor) raster and its lazily computed local gradients, shared by the window sizes.

    Device intermediates are computed on the stream current at their first use; an event recorded there after the launches
    makes the stream current at any later use wait for them (on the device: the host does not block), so the cached
    tensors stay ordered when `.histogram` is called again from another stream.

    mask (on the ORIGINAL sigma0 grid, non-zero = usable) and min_F (threshold on this field's own filtering_parameters F) give
    the field's keep mask on its local-gradients grid, cached and ordered like the local gradients."""

    def __init__(self, values, line, sample, factor=1, mask=None, min_F=None):
        self._src, self.factor = values, factor
        self._mask, self._min_F = _checked_mask(mask, values), _checked_min_F(min_F)
        self._keep = None
        self._keep_ev = None
        self.line = coarsen_coords(line, factor) if factor > 1 else np.asarray(line)
        self.sample = coarsen_coords(sample, factor) if factor > 1 else np.asarray(sample)
        self._values = values if factor == 1 else None
        self._values_ev = None
        self._lg = None
        self._lg_ev = None

    @staticmethod
    def _produced(t):
        """Event on the current stream of t's device, after what has been queued there (None for host arrays)."""
        if not _is_tensor(t):
            return None
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
        return ev

    @staticmethod
    def _consume(ev, t):
        if ev is not None:
            import torch
            torch.cuda.current_stream(t.device).wait_event(ev)

    @property
    def values(self):
        if self._values is None:
            self._values = _area(self._src, self.factor)
            self._values_ev = self._produced(self._values)
        else:
            self._consume(self._values_ev, self._values)
        return self._values

    @property
    def lg(self):
        """(G2, c, line, sample) of local_gradients(sqrt(R2(sigma0)))."""
        if self._lg is None:
            g2, _g3, c = _local(_r2(self.values, True))
            self._lg = (g2, c, coarsen_coords(coarsen_coords(self.line, 2), 2), coarsen_coords(coarsen_coords(self.sample, 2), 2))
            self._lg_ev = self._produced(g2)
        else:
            self._consume(self._lg_ev, self._lg[0])
        return self._lg

    @property
    def keep(self):
        """uint8 keep mask on the local-gradients grid (None without mask and min_F): the sigma0-grid mask reduced by
        4 f x 4 f blocks, AND F >= min_F reduced by 2 x 2, F = filtering_parameters of this field's own raster."""
        if self._mask is None and self._min_F is None:
            return None
        if self._keep is None:
            k = None
            if self._mask is not None:
                m = self._mask
                if _is_tensor(self._src) != _is_tensor(m):  # the mask follows sigma0's container kind
                    m = _device.as_tensor(m, _device.device_of(self._src)) if _is_tensor(self._src) else m.cpu().numpy()
                k = keep_mask(m, block=4 * self.factor)
            if self._min_F is not None:
                k = keep_mask(filtering_parameters(self.values).F, threshold=self._min_F, block=2, and_with=k)
            self._keep = k
            self._keep_ev = self._produced(k)
        else:
            self._consume(self._keep_ev, self._keep)
        return self._keep


def _checked_mask(mask, values):
    """The user's mask as an array of sigma0's (line, sample) shape, or ValueError / TypeError: host checks only."""
    if mask is None:
        return None
    if not _is_tensor(mask):
        mask = np.asarray(_unwrap(mask))
    if tuple(mask.shape) != tuple(values.shape[-2:]):
        raise ValueError(f"mask {tuple(mask.shape)} must have sigma0's (line, sample) shape {tuple(values.shape[-2:])}")
    if _u8_kind(mask) != "u8":
        raise TypeError(f"mask must be bool or uint8 (non-zero = usable), not {mask.dtype}")
    return mask


def _checked_min_F(min_F):
    if min_F is None:
        return None
    min_F = float(min_F)
    if np.isnan(min_F):
        raise ValueError("min_F is NaN")
    return min_F


class Gradients2D:
    """Direction histograms of a mono-pol (line, sample) sigma0 for one window size (gradients.py:45-205).

    window_size: in units of the coordinates (1600 = 16 km windows for 10 m coordinates, whatever sigma0's resolution);
    window_step: window stepping as a fraction of the window (1: no overlap); windows_at: dict(line=, sample=) of window centre
    coordinates.  window_step and windows_at are mutually exclusive.

    mask / min_F (this package's own; the reference computes `filtering_parameters` and applies it nowhere) remove pixels of the
    local-gradients grid from every window's histogram exactly as a NaN G2 would: they are not kept, stay out of the median of
    |G2|, add to no bin and do not count in used_ratio's numerator (the denominator stays w * w), so `Streaks.resolve(
    min_used_ratio=)` drops the windows they empty.  Their neighbours' gradients are untouched, unlike with NaN written into sigma0.
      mask:  bool / uint8 array on sigma0's (line, sample) grid, non-zero = usable (land, ice, an external rain flag); a pixel
             of the local-gradients grid is kept iff its whole 4 x 4 sigma0 block is usable.
      min_F: float; kept iff `filtering_parameters(sigma0).F >= min_F` on the pixel's whole 2 x 2 block of the half-resolution
             grid (NaN F: not kept).  There is no default.  Where the four filters saturate at 0 or 1, F takes exactly the
             plateau values 0.5, sqrt(1/2), sqrt(3/4) and 1, on many pixels; a threshold ON a plateau is decided by rounding.
             Choose min_F between plateaus (e.g. 0.3, 0.6, 0.7).
    Both given: AND.  ValueError for a mask of another shape, before any device call."""

    def __init__(self, sigma0, window_size=1600, window_step=None, windows_at=None, line=None, sample=None, mask=None, min_F=None):
        if window_step is not None and windows_at is not None:
            raise ValueError("window_step and window_at are mutually exclusive")
        if window_step is None and windows_at is None:
            window_step = 1
        if isinstance(sigma0, _Field):
            if mask is not None or min_F is not None:
                raise ValueError("a shared field carries its own mask / min_F")
            self._field = sigma0
        else:
            r = _Raster(sigma0, line, sample)
            self._field = _Field(r.values, r.line, r.sample, mask=mask, min_F=min_F)
        self.window_size = window_size
        self.n_angles = 72
        """Bin angles count, in the range [-pi/2, pi/2] (can be changed)"""
        self.window_step = window_step
        self._windows_at = windows_at

    @property
    def sigma0(self):
        return self._field.values

    @property
    def windows_at(self):
        """dict(line=, sample=) of window centre coordinates; by default sigma0's coordinates stepped by
        int(window pixels of sigma0 * window_step) (gradients.py:153-190).  Settable."""
        if self._windows_at is None and self.window_step is not None:
            step = int(window_pixels(self.window_size, self._field.line, self._field.sample) * self.window_step)
            self._windows_at = {"line": self._field.line[::step], "sample": self._field.sample[::step]}
        return self._windows_at

    @windows_at.setter
    def windows_at(self, windows_at):
        self._windows_at = windows_at

    def _weights(self):
        """(weight [line, sample, angles] divided by the window's pixel count, used_ratio [line, sample], centre coordinates)."""
        at = self.windows_at
        at_line, at_sample = _coord_values(at["line"]), _coord_values(at["sample"])
        g2, c, lg_line, lg_sample = self._field.lg
        w = window_pixels(self.window_size, lg_line, lg_sample)
        if w < 1:
            raise ValueError(f"window_size {self.window_size} is smaller than one pixel of the local-gradients grid")
        rows, cols = nearest_indexer(lg_line, at_line), nearest_indexer(lg_sample, at_sample)
        weight, ratio = _hist(g2, c, w, rows, cols, self.n_angles, keep=self._field.keep)
        return weight, ratio, at_line, at_sample

    @property
    def histogram(self):
        """Direction histograms of every window: weight [line, sample, angles] (divided by the window's pixel count), used_ratio
        [line, sample]; line / sample are the window centres (`windows_at`)."""
        weight, ratio, at_line, at_sample = self._weights()
        return GradientsHistogram(weight, ratio, angles_bins(self.n_angles), at_line, at_sample, ("line", "sample", "angles"))


class Gradients:
    """Direction histograms at several window sizes and resolutions (gradients.py:248-367).

    sigma0: (line, sample) or (pol, line, sample); windows_sizes: window sizes in coordinate units; downscales_factors: integer
    box-mean reductions of sigma0 (cv2 INTER_AREA); window_step: stepping of the FIRST (pol, factor, size) combination, whose
    window centres every other combination uses.

    mask / min_F: as in `Gradients2D`.  mask lies on the INPUT sigma0 grid (line, sample), one for all pols, and is reduced by
    4 f x 4 f blocks for the field of downscale factor f; min_F thresholds the F of each (pol, factor) field's OWN raster (the
    box-averaged sigma0 for f > 1), reduced by 2 x 2.  Each field computes its keep mask once, for all its window sizes.
    Choose min_F between F's plateaus 0.5, sqrt(1/2), sqrt(3/4), 1 (e.g. 0.3, 0.6, 0.7)."""

    def __init__(self, sigma0, windows_sizes=[1600], downscales_factors=[1], window_step=1, line=None, sample=None, pol=None,
                 mask=None, min_F=None):
        r = _Raster(sigma0, line, sample, pol, allow_pol=True)
        self._drop_pol = not r.has_pol
        self.windows_sizes, self.downscales_factors = list(windows_sizes), list(downscales_factors)
        self.pol = r.pol
        planes = [r.values] if self._drop_pol else [r.values[p] for p in range(r.values.shape[0])]
        self.gradients_list = []
        for plane in planes:
            for df in self.downscales_factors:
                field = _Field(plane, r.line, r.sample, int(df), mask=mask, min_F=min_F)
                for ws in self.windows_sizes:
                    self.gradients_list.append(Gradients2D(field, window_size=ws))
        # the 1st gradient defines windows_at from window_step for all the others (StackedGradients, :208-245)
        self.gradients_list[0].window_step = window_step
        for g in self.gradients_list[1:]:
            g.windows_at = self.gradients_list[0].windows_at

    @property
    def histogram(self):
        """weight [pol?, downscale_factor, window_size, line, sample, angles], used_ratio without angles, and the coordinates."""
        parts = [g._weights() for g in self.gradients_list]
        weight, ratio = [p[0] for p in parts], [p[1] for p in parts]
        lead = ([] if self._drop_pol else [len(self.pol)]) + [len(self.downscales_factors), len(self.windows_sizes)]
        if _is_tensor(weight[0]):
            import torch
            W, R = torch.stack(weight), torch.stack(ratio)
        else:
            W, R = np.stack(weight), np.stack(ratio)
        W = W.reshape(tuple(lead) + tuple(weight[0].shape))
        R = R.reshape(tuple(lead) + tuple(ratio[0].shape))
        dims = ("downscale_factor", "window_size", "line", "sample", "angles")
        coords = dict(window_size=np.asarray(self.windows_sizes), downscale_factor=np.asarray(self.downscales_factors))
        if not self._drop_pol:
            dims = ("pol",) + dims
            coords["pol"] = self.pol
        g0 = self.gradients_list[0]
        return GradientsHistogram(W, R, angles_bins(g0.n_angles), parts[0][2], parts[0][3], dims, **coords)
