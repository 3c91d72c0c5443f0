"""Wind on a regular longitude / latitude grid: order-free binning in fixed point, computed on the device.

    g = wind_grid(wind, TiePoints(...), lon=(lon0, dlon, n_lon), lat=(lat0, dlat, n_lat))    # a map of one scene
    g = invert_copol_codes(...).grid(tie_points, lon=..., lat=...)                            # the same from the 4-byte codes
    wind_grid(other_wind, other_tie_points, lon=..., lat=..., into=g)                         # a mosaic: a second scene added
    g += g_of_another_rank                                                                    # per-rank or per-tile sums merged

Every valid pixel is geolocated from the scene's tie points (the arithmetic of `ancillary_from_model`, per pixel), rotated to its
east / north components with its own heading, and adds five 64-bit integers to the bin it falls into: 1, u, v and |wind| in
units of 2**-24 m/s, |wind|**2 in units of 2**-16 (include/xsw.h: xsw_wind_grid; csrc/xsw_cells.hip: k_wind_grid).  Integer sums
have no order, so the launch, the kernel's pre-aggregation, a split of the scene into row tiles, the order of scenes and the
number of devices change no bit: `WindGrid.merge` of per-rank `sums` is exact, and it is the form a multi-GPU reduction takes.
The means follow on the small grid in the container's own float64 (`WindGrid.u`, ...): numpy and torch give the same bits, and
tests/grid_ref.py restates the whole call in numpy.  Only `WindGrid.direction` calls a trigonometric function.

Containers as in `cells`: numpy in gives numpy out (through host buffers, synchronous); a device tensor in gives device tensors
out, computed asynchronously on torch's current stream.  Every host check precedes any device call.
"""
import math
import operator
import os

import numpy as np

from . import _lib
from ._raster import _Call, _as_u8, _coord_values, _is_tensor, _small
from .ancillary import UNIFORM_TOLERANCE, TiePoints, _raster_axis
from .cells import _keep, _source
from .streaks import bracket

__all__ = ["WindGrid", "wind_grid", "codes_grid"]

PLANES = ("n", "Su", "Sv", "Ss", "Sq")  # the order of `WindGrid.sums`
Q24, Q16 = 2.0 ** -24, 2.0 ** -16       # what one unit of Su / Sv / Ss and of Sq is worth


def _axis_spec(spec, what, signed):
    """(edge of bin 0, step, bins) of one grid axis, checked."""
    try:
        first, step, n = spec
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be ({what}0, d{what}, n_{what}), not {spec!r}") from None
    try:
        n = operator.index(n)
    except TypeError:
        raise TypeError(f"n_{what} must be an integer, not {n!r}") from None
    try:
        first, step = float(first), float(step)
    except (TypeError, ValueError):
        raise TypeError(f"{what}0 and d{what} must be numbers, not {spec!r}") from None
    if not (math.isfinite(first) and math.isfinite(step)):
        raise ValueError(f"{what}0 and d{what} must be finite, not {(first, step)}")
    if step == 0.0 or (step < 0.0 and not signed):
        raise ValueError(f"d{what} must be {'non-zero' if signed else 'positive'}, not {step}")
    if n < 1 or n > 0x7fffffff:
        raise ValueError(f"n_{what} must be 1 or more (and fit int32), not {n}")
    return first, step, n


class GridSpec:
    """The grid of a `WindGrid`: bin (j, i) covers [lon0 + i dlon, lon0 + (i + 1) dlon) and the latitudes from lat0 + j dlat to
    lat0 + (j + 1) dlat; lon0 / lat0 are the EDGES of bin 0.  dlon > 0; dlat signed (a descending axis: dlat < 0).  The longitude
    axis is periodic iff n_lon * dlon is 360 within 1e-3 * dlon, the rule of `ancillary_from_model`."""

    def __init__(self, lon, lat):
        self.lon0, self.dlon, self.n_lon = _axis_spec(lon, "lon", signed=False)
        self.lat0, self.dlat, self.n_lat = _axis_spec(lat, "lat", signed=True)
        if self.n_lon * self.n_lat > 0x7fffffff:
            raise ValueError(f"n_lon * n_lat = {self.n_lon * self.n_lat} bins do not fit int32")
        self.periodic = abs(self.n_lon * self.dlon - 360.0) <= UNIFORM_TOLERANCE * self.dlon

    def key(self):
        return self.lon0, self.dlon, self.n_lon, self.lat0, self.dlat, self.n_lat

    def __eq__(self, other):
        return isinstance(other, GridSpec) and self.key() == other.key()

    def __repr__(self):
        return f"GridSpec(lon={self.key()[:3]}, lat={self.key()[3:]})"

    @property
    def shape(self):
        return self.n_lat, self.n_lon


class WindGrid:
    """Result of `wind_grid` / `codes_grid` / `CopolCodes.grid`.  `sums`: int64 `[5, n_lat, n_lon]` (numpy, or a torch tensor for
    a device source), the planes n, Su, Sv, Ss, Sq; `spec`: the `GridSpec`.  What follows from the sums is computed on first use
    in the container's own float64, in the order include/xsw.h states, and again after the sums changed through `into=` or
    `merge`: count (int64), u, v (east / north, "blowing to", m/s), wspd (the scalar mean), wspd_std (sample standard deviation,
    NaN below two pixels), steadiness (|vector mean| / scalar mean).  A bin without a pixel is NaN with count 0.  longitude
    [n_lon], latitude [n_lat]: the bin centres (numpy).  A bin is exact up to 2**30 pixels over everything accumulated."""

    def __init__(self, sums, spec):
        if not isinstance(spec, GridSpec):
            raise TypeError("spec must be a GridSpec")
        if tuple(sums.shape) != (5,) + spec.shape or str(sums.dtype).replace("torch.", "") != "int64":
            raise ValueError(f"sums must be int64 [5, n_lat, n_lon] = {(5,) + spec.shape}, not {sums.dtype} {tuple(sums.shape)}")
        self.sums, self.spec = sums, spec
        self._finished = None

    def __getitem__(self, name):
        return getattr(self, name)

    @property
    def on_device(self):
        return _is_tensor(self.sums)

    @property
    def longitude(self):
        return self.spec.lon0 + (np.arange(self.spec.n_lon) + 0.5) * self.spec.dlon

    @property
    def latitude(self):
        return self.spec.lat0 + (np.arange(self.spec.n_lat) + 0.5) * self.spec.dlat

    def _finish(self):
        """u, v, wspd, wspd_std, steadiness from the sums: `*`, `/`, `-` and sqrt alone, one operation per step."""
        if self._finished is None:
            if self.on_device:
                import torch
                f64, sqrt, where = (lambda a: a.to(torch.float64)), torch.sqrt, torch.where
                # (filled on the device: a tensor made from a host scalar would wait for the stream)
                nan, zero = (torch.full((), v, dtype=torch.float64, device=self.sums.device) for v in (float("nan"), 0.0))
                n, su, sv, ss, sq = self.sums.unbind(0)
                ctx = None
            else:
                f64, sqrt, where, nan, zero = (lambda a: a.astype(np.float64)), np.sqrt, np.where, np.nan, 0.0
                n, su, sv, ss, sq = self.sums
                ctx = np.errstate(invalid="ignore", divide="ignore")
                ctx.__enter__()
            try:
                nd = f64(n)
                u, v, wspd = (f64(su) / nd) * Q24, (f64(sv) / nd) * Q24, (f64(ss) / nd) * Q24
                s1, s2 = f64(ss) * Q24, f64(sq) * Q16
                var = (s2 - (s1 * s1) / nd) / (nd - 1.0)
                std = where(n < 2, nan, sqrt(where(var < 0.0, zero, var)))
                steadiness = sqrt(u * u + v * v) / wspd
            finally:
                if ctx is not None:
                    ctx.__exit__(None, None, None)
            self._finished = dict(u=u, v=v, wspd=wspd, wspd_std=std, steadiness=steadiness)
        return self._finished

    count = property(lambda self: self.sums[0])
    u = property(lambda self: self._finish()["u"])
    v = property(lambda self: self._finish()["v"])
    wspd = property(lambda self: self._finish()["wspd"])
    wspd_std = property(lambda self: self._finish()["wspd_std"])
    steadiness = property(lambda self: self._finish()["steadiness"])

    @property
    def direction(self):
        """The meteorological direction the wind comes FROM, degrees clockwise from north, as `WindCells.direction`: the one
        value of this class that is not pinned to the bit."""
        if self.on_device:
            import torch
            return torch.remainder(270.0 - torch.rad2deg(torch.atan2(self.v, self.u)), 360.0)
        return (270.0 - np.degrees(np.arctan2(self.v, self.u))) % 360.0

    def _same_grid(self, other, what):
        if not isinstance(other, WindGrid):
            raise TypeError(f"{what} must be a WindGrid, not {type(other).__name__}")
        if other.spec != self.spec:
            raise ValueError(f"{what} lies on {other.spec}, not on {self.spec}: sums of different grids cannot be added")
        if other.on_device != self.on_device:
            raise ValueError(f"{what} holds {'device' if other.on_device else 'host'} sums, this grid {'device' if self.on_device else 'host'} ones: "
                             "one container kind")

    def merge(self, other):
        """Add another grid's `sums` (the same `spec`, the same container kind; else ValueError) into this one's and return
        self.  Exact: the form in which ranks, row tiles or scenes are combined."""
        self._same_grid(other, "the other grid")
        if self.on_device:
            self.sums += other.sums.to(self.sums.device)
        else:
            self.sums += other.sums
        self._finished = None
        return self

    __iadd__ = merge


def _grid_path():
    v = os.environ.get("XSW_GRID_PATH")
    if v is not None and v not in ("direct", "lds"):
        raise ValueError(f"XSW_GRID_PATH must be direct or lds, not {v!r}")


def _pixel_axis(coords, n, tie, what):
    c = np.arange(n, dtype=np.float64) if coords is None else np.asarray(_coord_values(coords), dtype=np.float64)
    if c.shape != (n,):
        raise ValueError(f"{what} coordinates of shape {c.shape} do not match the raster's {n} {what}s")
    return _raster_axis(c, tie, what)


def _wind_grid(src, kind, what, tie_points, lon, lat, line, sample, keep, into, lut=None):
    # every host check
    keep = _keep(keep, src, what)
    if not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    L, S = (int(v) for v in src.shape)
    line, sample = _pixel_axis(line, L, tie_points.line, "line"), _pixel_axis(sample, S, tie_points.sample, "sample")
    spec = GridSpec(lon, lat)
    _grid_path()
    if into is not None:
        if not isinstance(into, WindGrid):
            raise TypeError(f"into must be a WindGrid, not {type(into).__name__}")
        if into.spec != spec:
            raise ValueError(f"into lies on {into.spec}, the call asks for {spec}")
        if into.on_device != _is_tensor(src):
            raise ValueError(f"into holds {'device' if into.on_device else 'host'} sums but {what} is a {'device' if _is_tensor(src) else 'host'} array: "
                             "one container kind per call")
    lf, lt = bracket(tie_points.line, line)
    sf, st = bracket(tie_points.sample, sample)

    # the device from here on
    call = _Call(src)
    if call.device:
        from . import _device
        src = _device.as_tensor(src, call.dev).contiguous()
    else:
        src = np.ascontiguousarray(src)
    if into is None:
        sums = call.empty((5,) + spec.shape, np.int64)
        if call.device:
            sums.zero_()  # on the current stream, as the launch is
        else:
            sums.fill(0)
        out = WindGrid(sums, spec)
    else:
        out, sums = into, into.sums
        if call.device:
            sums = _device.as_tensor(sums, call.dev)
        if not (sums.is_contiguous() if call.device else sums.flags.c_contiguous):
            raise ValueError("into.sums must be contiguous")
    if L * S:
        keep = None if keep is None else _as_u8(call, keep)
        tables = [_small(call, a, np.float64) for a in (tie_points.longitude, tie_points.latitude, tie_points.cos_heading, tie_points.sin_heading)]
        tables += [_small(call, lf, np.int32), _small(call, lt, np.float64), _small(call, sf, np.int32), _small(call, st, np.float64)]
        args = (L, S, call.mem, kind, src, keep, len(tie_points.line), len(tie_points.sample), *tables, spec.lon0, spec.dlon, spec.n_lon,
                int(spec.periodic), spec.lat0, spec.dlat, spec.n_lat, sums)
        if lut is None:
            call.launch("wind_grid_raw", *args)
        else:  # codes: the context must hold their LUT when the kernel reads `sol`
            from .windspeed import _engine
            is_array = lambda a: hasattr(a, "data_ptr") or isinstance(a, np.ndarray)

            def run(ctx, mem):
                with ctx.lock:
                    _engine.ensure_luts(ctx, lut, None)
                    ctx.wind_grid_raw(*[call.ptr(a) if is_array(a) else a for a in args])
            call.run(run, [a for a in args if is_array(a)])
        out._finished = None
    return out


def wind_grid(wind, tie_points, *, lon, lat, line=None, sample=None, keep=None, into=None):
    """`WindGrid` of a complex wind raster on the grid lon = (lon0, dlon, n_lon), lat = (lat0, dlat, n_lat).

    wind: complex128 or complex64 `[L, S]`, antenna convention, numpy or a device tensor.  tie_points: the scene's `TiePoints`
    (required: every pixel is geolocated).  line / sample: the raster's coordinate vectors (default np.arange; a row tile passes
    its own lines); every coordinate lies inside the tie points' span.  lon0 / lat0 are the edges of bin 0, dlon > 0, dlat is
    signed; the longitude axis is periodic iff n_lon * dlon is 360 (`GridSpec`), otherwise pixels outside the grid are dropped,
    the upper edge being outside.  A pixel counts iff neither part is NaN, its keep byte (bool / uint8 `[L, S]` in the raster's
    container kind) is non-zero, its heading is defined and its speed is below 256 m/s.

    into: a `WindGrid` of the same grid and container kind, whose `sums` the call adds to (and which it returns): a mosaic of
    scenes, or a scene in row tiles.  Any order gives the same bits.  Without it the sums start at zero.

    ValueError / TypeError for a wrong rank, dtype or container kind, a `keep` of another shape, `tie_points` that is not a
    `TiePoints`, coordinates outside the tie span, a bad grid entry, an `into` of another grid, an XSW_GRID_PATH other than
    `direct` or `lds` -- all before any device call."""
    src, name = _source(wind, "wind", ("complex128", "complex64"))
    return _wind_grid(src, _lib.CELLS_C128 if name == "complex128" else _lib.CELLS_C64, "wind", tie_points, lon, lat, line, sample, keep, into)


def codes_grid(codes, lut_co, tie_points, *, lon, lat, line=None, sample=None, keep=None, into=None):
    """`wind_grid` from co-pol grid codes `[L, S]` (uint32 numpy, or an int32 / uint32 device tensor) of the LUT `lut_co`
    (`CopolCodes.grid` calls this): 4 B per pixel are read and nothing is expanded; bit for bit `wind_grid` of the complex128
    expansion."""
    src, _ = _source(codes, "codes", ("uint32", "int32"))
    if not _is_tensor(src):
        src = src.view(np.uint32)
    return _wind_grid(src, _lib.CELLS_CODES, "codes", tie_points, lon, lat, line, sample, keep, into, lut=lut_co)
