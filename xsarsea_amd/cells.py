"""Wind product cells: block statistics of a raster on a product grid, computed on the device -- the way out of HBM.

    cells = wind_cells(wind, cell=(100, 100), tie_points=TiePoints(...))     # 1 km cells from 10 m pixels
    cells = invert_copol_codes(...).cells((100, 100), tie_points=...)       # the same from the 4-byte codes, nothing expanded
    sig   = raster_cells(sigma0, (100, 100))                                # count, mean, std of a real raster

The inversion chain leaves a full-resolution complex raster (or its grid codes) in device memory; what a user wants of it is
almost always the wind on a product grid -- a few kilobytes.  The raster `[L, S]` is tiled from pixel (0, 0) by cells of
`cl x cs` pixels (`ceil(L / cl)` by `ceil(S / cs)` cells, the last one of an axis clipped); per cell one HIP pass
(csrc/xsw_cells.hip; include/xsw.h: xsw_wind_cells, xsw_raster_cells) gives the valid count, the vector mean wind, the scalar
mean speed, its scatter and the steadiness, and with tie points the centre's longitude / latitude and the east / north components.
Every sum is float64 in one stated order (include/xsw.h), so the results do not depend on the launch and equal the numpy
restatement tests/cells_ref.py bit for bit.  Only `WindCells.direction` calls a trigonometric function (the container's own
`arctan2`, on the cell grid): it is the one value not pinned to the bit.

Containers as in `ancillary`: numpy in gives numpy out (through host buffers, synchronous); a device tensor in gives device
tensors out, computed asynchronously on torch's current stream.  Every host check precedes any device call.
"""
import operator

import numpy as np

from . import _lib
from ._raster import _Call, _as_u8, _coord_values, _is_tensor, _small, _unwrap
from .ancillary import TiePoints, _raster_axis
from .streaks import bracket

__all__ = ["WindCells", "RasterCells", "wind_cells", "raster_cells"]


class WindCells:
    """Result of `wind_cells` / `CopolCodes.cells`, one `[nLc, nSc]` array each (numpy, or torch tensors for a device source):
    count (int32, the valid pixels), wind (complex128, the vector mean in antenna convention), wspd (the scalar mean of |wind|),
    wspd_std (its sample standard deviation, NaN below two pixels), steadiness (|vector mean| / scalar mean, NaN where wspd is
    0); line, sample: the cells' centre coordinates (numpy: (first + last) / 2 of the cell's pixels); longitude, latitude (the
    tie points' continuous longitude, not wrapped), u, v (east / north components, "blowing to", m/s): None without tie
    points.  A cell without a valid pixel is NaN with count 0: mask on `count`."""

    def __init__(self, count, wind, wspd, wspd_std, steadiness, line, sample, longitude=None, latitude=None, u=None, v=None):
        self.count, self.wind, self.wspd, self.wspd_std, self.steadiness = count, wind, wspd, wspd_std, steadiness
        self.line, self.sample = line, sample
        self.longitude, self.latitude, self.u, self.v = longitude, latitude, u, v

    def __getitem__(self, name):
        return getattr(self, name)

    @property
    def direction(self):
        """The meteorological direction the wind comes FROM, degrees clockwise from north: (270 - degrees(arctan2(v, u))) % 360,
        with the container's own arctan2 (numpy's or torch's) on the cell grid -- the one value of this class that is not
        pinned to the bit.  None without tie points."""
        if self.u is None:
            return None
        if _is_tensor(self.u):
            import torch
            return torch.remainder(270.0 - torch.rad2deg(torch.atan2(self.v, self.u)), 360.0)
        return (270.0 - np.degrees(np.arctan2(self.v, self.u))) % 360.0


class RasterCells:
    """Result of `raster_cells`: count (int32), mean, std (sample standard deviation, NaN below two pixels) per cell, and the
    cells' centre coordinates line, sample (numpy)."""

    def __init__(self, count, mean, std, line, sample):
        self.count, self.mean, self.std, self.line, self.sample = count, mean, std, line, sample

    def __getitem__(self, name):
        return getattr(self, name)


def _cell_shape(cell):
    try:
        cl, cs = cell
    except (TypeError, ValueError):
        raise ValueError(f"cell must be (cell_lines, cell_samples), not {cell!r}") from None
    try:
        cl, cs = operator.index(cl), operator.index(cs)
    except TypeError:
        raise TypeError(f"cell entries must be integers, not {cell!r}") from None
    if cl < 1 or cs < 1 or cl > 0x7fffffff or cs > 0x7fffffff:
        raise ValueError(f"cell entries must be 1 or more (and fit int32), not {(cl, cs)}")
    return cl, cs


def _source(a, what, dtypes):
    """The raster as the call reads it (a device tensor, or a numpy array) and its dtype's name, after the rank and dtype checks."""
    a = _unwrap(a)
    a = a if _is_tensor(a) else np.asarray(a)
    name = str(a.dtype).replace("torch.", "")
    if name not in dtypes:
        raise TypeError(f"{what} must be {' or '.join(dtypes)}, not {name}")
    if len(tuple(a.shape)) != 2:
        raise ValueError(f"{what} must be a 2-D raster [line, sample], not of shape {tuple(a.shape)}")
    return a, name


def _keep(keep, src, what):
    if keep is None:
        return None
    keep = _unwrap(keep)
    keep = keep if _is_tensor(keep) else np.asarray(keep)
    if _is_tensor(keep) != _is_tensor(src):
        raise ValueError(f"keep is a {'device' if _is_tensor(keep) else 'host'} array but {what} is a "
                         f"{'device' if _is_tensor(src) else 'host'} one: one container kind per call")
    if str(keep.dtype).replace("torch.", "") not in ("bool", "uint8"):
        raise TypeError(f"keep must be bool or uint8, not {keep.dtype}")
    if tuple(keep.shape) != tuple(src.shape):
        raise ValueError(f"keep has shape {tuple(keep.shape)}, {what} has shape {tuple(src.shape)}")
    return keep


def _centres(coords, n, step, what):
    """The cells' centre coordinates on an axis of n pixels: (coord[first] + coord[last]) / 2 of each cell's pixels."""
    c = np.arange(n, dtype=np.float64) if coords is None else np.asarray(_coord_values(coords), dtype=np.float64)
    if c.shape != (n,):
        raise ValueError(f"{what} coordinates of shape {c.shape} do not match the raster's {n} {what}s")
    if not np.isfinite(c).all():
        raise ValueError(f"{what} coordinates hold a NaN or an infinity")
    first = np.arange(0, n, step)
    last = np.minimum(first + step, n) - 1
    return (c[first] + c[last]) / 2 if n else np.empty(0)


def _plan(src, what, cell, tie_points, line, sample, keep):
    """Every host check of a call: (cl, cs), keep, the centre coordinates and, with tie points, their brackets."""
    cl, cs = _cell_shape(cell)
    keep = _keep(keep, src, what)
    if tie_points is not None and not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    L, S = (int(v) for v in src.shape)
    cline, csample = _centres(line, L, cl, "line"), _centres(sample, S, cs, "sample")
    brackets = None
    if tie_points is not None:
        cline, csample = _raster_axis(cline, tie_points.line, "line"), _raster_axis(csample, tie_points.sample, "sample")
        brackets = bracket(tie_points.line, cline) + bracket(tie_points.sample, csample)
    return cl, cs, keep, cline, csample, brackets


def _wind_cells(src, kind, what, cell, tie_points, line, sample, keep, lut=None):
    cl, cs, keep, cline, csample, brackets = _plan(src, what, cell, tie_points, line, sample, keep)
    L, S = (int(v) for v in src.shape)
    shape = (len(cline), len(csample))

    # the device from here on
    call = _Call(src)
    if call.device:
        from . import _device
        src = _device.as_tensor(src, call.dev).contiguous()
    else:
        src = np.ascontiguousarray(src)
    outs = [call.empty(shape, dt) for dt in (np.int32, np.complex128, np.float64, np.float64, np.float64)]
    geo = [call.empty(shape, np.float64) for _ in range(4)] if tie_points is not None else [None] * 4
    if L * S:
        keep = None if keep is None else _as_u8(call, keep)
        ties = [0, 0] + [None] * 8
        if tie_points is not None:
            lf, lt, sf, st = brackets
            ties = [len(tie_points.line), len(tie_points.sample)]
            ties += [_small(call, a, np.float64) for a in (tie_points.longitude, tie_points.latitude, tie_points.cos_heading, tie_points.sin_heading)]
            ties += [_small(call, lf, np.int32), _small(call, lt, np.float64), _small(call, sf, np.int32), _small(call, st, np.float64)]
        args = (L, S, call.mem, kind, src, keep, cl, cs, *ties, *outs, *geo)
        if lut is None:
            call.launch("wind_cells_raw", *args)
        else:  # codes: the context must hold their LUT when the kernel reads `sol`
            from .windspeed import _engine
            is_array = lambda a: hasattr(a, "data_ptr") or isinstance(a, np.ndarray)

            def run(ctx, mem):
                with ctx.lock:
                    _engine.ensure_luts(ctx, lut, None)
                    ctx.wind_cells_raw(*[call.ptr(a) if is_array(a) else a for a in args])
            call.run(run, [a for a in args if is_array(a)])
    return WindCells(*outs, cline, csample, *geo)


def wind_cells(wind, cell, *, tie_points=None, line=None, sample=None, keep=None):
    """`WindCells` of a complex wind raster on the product grid of `cell = (cell_lines, cell_samples)` pixels per cell.

    wind: complex128 or complex64 `[L, S]`, antenna convention, numpy or a device tensor: what `invert_from_model`,
    `CopolCodes.wind()` or `.dual()` return.  A pixel counts iff neither of its parts is NaN and, with `keep` (bool / uint8
    `[L, S]` in the raster's container kind), its keep byte is non-zero.  line / sample: the raster's coordinate vectors
    (default np.arange); the cells' centres are the means of their first and last pixel's coordinates.  tie_points: the
    scene's `TiePoints`; every centre must lie inside their span (geolocation is not extrapolated).  With them the result
    carries longitude, latitude, u, v (and `.direction`).

    Every sum is float64 in the order include/xsw.h states (complex64 parts are widened first); tests/cells_ref.py restates the
    call in numpy bit for bit.  ValueError / TypeError for a cell entry that is not an integer >= 1, a wrong rank or dtype, a
    `keep` of another shape or container kind, `tie_points` that is not a `TiePoints`, centres outside the tie span -- all before
    any device call."""
    src, name = _source(wind, "wind", ("complex128", "complex64"))
    return _wind_cells(src, _lib.CELLS_C128 if name == "complex128" else _lib.CELLS_C64, "wind", cell, tie_points, line, sample, keep)


def codes_cells(codes, lut_co, cell, *, tie_points=None, line=None, sample=None, keep=None):
    """`wind_cells` from co-pol grid codes `[L, S]` (uint32 numpy, or an int32 / uint32 device tensor) of the LUT `lut_co`
    (`CopolCodes.cells` calls this): 4 B per pixel are read and nothing is expanded; bit for bit `wind_cells` of the complex128
    expansion."""
    src, _ = _source(codes, "codes", ("uint32", "int32"))
    if not _is_tensor(src):
        src = src.view(np.uint32)
    return _wind_cells(src, _lib.CELLS_CODES, "codes", cell, tie_points, line, sample, keep, lut=lut_co)


def raster_cells(x, cell, *, keep=None, line=None, sample=None):
    """`RasterCells` (count, mean, std per cell) of a float32 / float64 raster `[L, S]`, numpy or a device tensor, on the product
    grid of `cell = (cell_lines, cell_samples)`: linear sigma0 before an inversion at product resolution, the incidence,
    `InversionCost.J`, `wspd_std`...  A pixel counts iff it is not NaN and, with `keep`, its keep byte is non-zero.  Sums,
    containers and refusals as `wind_cells`."""
    src, name = _source(x, "x", ("float32", "float64"))
    cl, cs, keep, cline, csample, _ = _plan(src, "x", cell, None, line, sample, keep)
    L, S = (int(v) for v in src.shape)

    # the device from here on
    call = _Call(src)
    src = call.prep(src)
    outs = [call.empty((len(cline), len(csample)), dt) for dt in (np.int32, np.float64, np.float64)]
    if L * S:
        call.launch("raster_cells_raw", L, S, call.mem, call.xsw_dtype(src), src, None if keep is None else _as_u8(call, keep), cl, cs, *outs)
    return RasterCells(*outs, cline, csample)
