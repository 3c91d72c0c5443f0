"""sigma0, NESZ, incidence and a validity mask from a product's digital numbers, computed on the device.

    cal = calibrate_dn(dn, AnnotationGrid(line, sample, sigma0_lut), noise_range=..., noise_azimuth=..., incidence=...)
    invert_from_model(cal.incidence, cal.sigma0, ...)          # device tensors, as every other call here takes them

A GRD product holds 2-byte digital numbers per pixel and a few kilobytes of annotation: the sigma0 calibration vectors, the noise
vectors, the geolocation grid with the incidence angle.  Expanded on the host they are four float32 rasters that cross the link;
here the digital numbers cross it as they are and one HIP kernel (csrc/xsw_calibrate.hip, include/xsw.h: xsw_calibrate) applies
xsar's arithmetic -- sigma0_raw = DN**2 / A**2, nesz = N / A**2, sigma0 = sigma0_raw - nesz, A and N bilinear between the
annotation nodes -- in one streaming pass.  Reading product files is the caller's: the vectors come from xsar or any other reader.

Containers as in `ancillary`: numpy in and no `device=` gives numpy out (through host buffers, synchronous); a device `dn`, or
`device=`, gives device tensors, computed asynchronously on torch's current stream.  Every host check precedes any device call.
"""
import numpy as np

from . import _lib
from ._raster import _Call, _coord_values, _is_tensor, _small, _unwrap
from .ancillary import _axis, _raster_axis
from .streaks import bracket

__all__ = ["AnnotationGrid", "Calibrated", "raster_from_grid", "calibrate_dn"]


class AnnotationGrid:
    """A tensor-product annotation table: `line[nl]`, `sample[ns]` (strictly ascending, not necessarily uniform, one node or more
    each) and `values` [nl, ns], float64 and finite, else ValueError.  Host arrays, or objects with `.values`.  Nodes may lie
    outside the raster (Sentinel-1 calibration vectors start at negative lines); between nodes the table is bilinear, and it is
    never extrapolated.  Two nodes at neighbouring integer coordinates (s, s + 1) state a jump exactly: pixel s reads the first
    alone, pixel s + 1 the second.  This is how the sub-swath boundary of a GRD azimuth-noise block is given."""

    def __init__(self, line, sample, values):
        self.line, self.sample = _axis(line, "annotation line"), _axis(sample, "annotation sample")
        for a, what in ((self.line, "line"), (self.sample, "sample")):
            if len(a) > 1 and not (np.diff(a) > 0).all():
                raise ValueError(f"annotation {what} coordinates must be strictly ascending")
        v = np.asarray(_coord_values(values), dtype=np.float64)
        if v.shape != self.shape:
            raise ValueError(f"annotation values must be [line, sample] = {self.shape}, not {v.shape}")
        if not np.isfinite(v).all():
            raise ValueError("annotation values hold a NaN or an infinity")
        self.values = np.array(v, order="C")  # the grid's own copy

    @property
    def shape(self):
        return len(self.line), len(self.sample)


class Calibrated:
    """Result of `calibrate_dn`: sigma0, nesz, incidence (`dtype`) and valid (uint8) `[L, S]`; an output that was not asked for
    is None.  Attribute or item access."""

    def __init__(self, sigma0, nesz, incidence, valid):
        self.sigma0, self.nesz, self.incidence, self.valid = sigma0, nesz, incidence, valid

    def __getitem__(self, name):
        return getattr(self, name)


def _grid(g, what, required=False):
    if g is None and not required:
        return None
    if not isinstance(g, AnnotationGrid):
        raise TypeError(f"{what} must be an AnnotationGrid, not {type(g).__name__}")
    return g


def _out_dtype(dtype):
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt is None or dt.name not in ("float32", "float64"):
        raise ValueError(f"dtype must be float32 or float64, not {dtype!r}")
    return dt.type


def _raster_coords(shape, line, sample):
    """(line, sample) coordinate vectors from shape=(L, S) or line= and sample=: exactly one of the two forms."""
    coords = line is not None or sample is not None
    if coords == (shape is not None):
        raise ValueError("give the raster as shape=(L, S) or as line= and sample=: exactly one of the two forms")
    if coords and (line is None or sample is None):
        raise ValueError("line= and sample= go together")
    if shape is not None:
        if len(tuple(shape)) != 2 or min(int(v) for v in shape) < 0:
            raise ValueError(f"shape must be (L, S), not {shape}")
        line, sample = np.arange(int(shape[0])), np.arange(int(shape[1]))
    return line, sample


def _device(device):
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a GPU, not {dev}")
    return dev


def _table(call, g, line, sample):
    """xsw_table of grid `g` for the raster's coordinates: (n_lines, n_samples, values, line_first, line_t, sample_first, sample_t)."""
    lf, lt = bracket(g.line, line)
    sf, st = bracket(g.sample, sample)
    return (len(g.line), len(g.sample), _small(call, g.values, np.float64), _small(call, lf, np.int32), _small(call, lt, np.float64),
            _small(call, sf, np.int32), _small(call, st, np.float64))


def _launch(call, L, S, dn_kind, out_dtype, dn, tables, fill, outs):
    """xsw_calibrate on the call's context; every array handed in is recorded on the launch stream."""
    arrays = [a for a in [dn, *outs] if a is not None] + [a for t in tables if t is not None for a in t[2:]]
    ptr = lambda a: None if a is None else call.ptr(a)
    raw = [None if t is None else t[:2] + tuple(ptr(a) for a in t[2:]) for t in tables]
    call.run(lambda ctx, mem: ctx.calibrate_raw(L, S, mem, dn_kind, _lib.XSW_F32 if out_dtype is np.float32 else _lib.XSW_F64, ptr(dn), *raw, fill,
                                                *[ptr(o) for o in outs]), arrays)


def raster_from_grid(grid, *, shape=None, line=None, sample=None, dtype="float32", device=None):
    """An `AnnotationGrid` at every pixel of a raster `[L, S]`: the incidence angle, the elevation angle, the ground heading.

    The raster's coordinate vectors are `line` / `sample`, or np.arange of `shape=(L, S)`: exactly one of the two forms; every
    coordinate lies inside the grid's span (no extrapolation), else ValueError.  Per pixel the four nodes around it are blended
    (`streaks.bracket` per axis) as wl0 * (ws0 * f00 + ws1 * f01) + wl1 * (ws0 * f10 + ws1 * f11) in float64 and rounded once to
    `dtype` (float32 or float64).  Returns numpy when `device` is None (host buffers, synchronous), otherwise a device tensor,
    computed asynchronously on torch's current stream."""
    grid = _grid(grid, "grid", required=True)
    out_dtype = _out_dtype(dtype)
    line, sample = _raster_coords(shape, line, sample)
    line, sample = _raster_axis(line, grid.line, "line"), _raster_axis(sample, grid.sample, "sample")
    L, S = len(line), len(sample)
    dev = _device(device) if device is not None else None

    # the device from here on
    if dev is not None:
        import torch
        out = torch.empty((L, S), dtype=getattr(torch, np.dtype(out_dtype).name), device=dev)
        call = _Call(out)
    else:
        call = _Call()
        out = call.empty((L, S), out_dtype)
    if L * S:
        _launch(call, L, S, _lib.DN_U16, out_dtype, None, [None, None, None, _table(call, grid, line, sample)], None, [None, None, out, None])
    return out


def _dn_kind(dn):
    """(the array, 'uint16' or 'float32') of the digital numbers; TypeError for any other type."""
    dn = _unwrap(dn)
    if not _is_tensor(dn):
        dn = np.asarray(dn)
    name = str(dn.dtype).replace("torch.", "")
    if name not in (("uint16", "int16", "float32") if _is_tensor(dn) else ("uint16", "float32")):
        raise TypeError("dn must be numpy uint16 or float32, or a device tensor of uint16, int16 (read as unsigned) or float32, "
                        f"not {'a device tensor of ' if _is_tensor(dn) else ''}{name}")
    if len(tuple(dn.shape)) != 2:
        raise ValueError(f"dn must be [L, S], not of shape {tuple(dn.shape)}")
    return dn, "float32" if name == "float32" else "uint16"


def calibrate_dn(dn, sigma0_lut, *, noise_range=None, noise_azimuth=None, incidence=None, line=None, sample=None, fill=0, dtype="float32",
                 nesz=True, valid=False, device=None):
    """`Calibrated(sigma0, nesz, incidence, valid)` of the digital numbers `dn` `[L, S]`.

    dn: numpy uint16 or float32, or a device tensor of torch.uint16, torch.int16 (reinterpreted as unsigned) or torch.float32;
    anything else is a TypeError.  sigma0_lut: the sigma0 calibration LUT A, an `AnnotationGrid` with values > 0.  noise_range /
    noise_azimuth: the noise LUT's range and azimuth factors (values >= 0); incidence: the incidence angle on the geolocation
    grid.  line / sample: the raster's coordinate vectors (default np.arange); every coordinate lies inside every grid's span.

    Per pixel, every operation float64 and rounded once: A, Nr, Na, inc bilinear on their own grids (`raster_from_grid`);
    N = Nr * Na (one alone when only one is given, 0.0 when neither); d = dn, q = d * d, g = 1 / (A * A); nesz = N * g,
    sigma0 = (q - N) * g; where dn == fill (fill=None: never; float32 dn: compared in float32) sigma0 is NaN, nesz and incidence
    are still written; valid (uint8, usable as `keep=`) is 1 iff the pixel is not fill and sigma0 > 0; the float outputs are
    rounded once to `dtype` (float32 or float64).  include/xsw.h (xsw_calibrate) fixes the order; tests/calibrate_ref.py restates
    it in numpy, bit for bit.  nesz=False / valid=True choose the outputs; incidence is written iff its grid is given.

    Returns numpy rasters when `dn` is numpy and `device` is None (host buffers, synchronous); otherwise device tensors on
    `device` (or dn's device), computed asynchronously on torch's current stream: a numpy `dn` is uploaded through page-locked
    staging as its own 2 bytes per pixel."""
    # every host check
    dn, kind = _dn_kind(dn)
    lut = _grid(sigma0_lut, "sigma0_lut", required=True)
    nr, na, inc = _grid(noise_range, "noise_range"), _grid(noise_azimuth, "noise_azimuth"), _grid(incidence, "incidence")
    if not (lut.values > 0).all():
        raise ValueError("sigma0_lut values must be positive")
    for g, what in ((nr, "noise_range"), (na, "noise_azimuth")):
        if g is not None and not (g.values >= 0).all():
            raise ValueError(f"{what} values must not be negative")
    out_dtype = _out_dtype(dtype)
    L, S = (int(v) for v in dn.shape)
    grids = [lut, nr, na, inc]
    axes = []
    for coords, n, what in ((line, L, "line"), (sample, S, "sample")):
        c = np.arange(n, dtype=np.float64) if coords is None else np.asarray(_coord_values(coords), dtype=np.float64)
        if c.shape != (n,):
            raise ValueError(f"{what} coordinates of shape {c.shape} do not match the raster's {n} {what}s")
        for g in grids:
            if g is not None:
                _raster_axis(c, getattr(g, what), what)
        axes.append(c)
    line, sample = axes
    if fill is not None:
        if isinstance(fill, (bool, np.bool_)) or not np.isscalar(fill) or not np.isreal(fill):
            raise TypeError(f"fill must be a number or None, not {fill!r}")
        if kind == "uint16" and not (0 <= fill <= 65535 and float(fill).is_integer()):
            raise ValueError(f"the fill value of uint16 digital numbers must be a whole number in 0 .. 65535, not {fill!r}")
        fill = float(fill)
    dev = _device(device) if device is not None else None

    # the device from here on
    if _is_tensor(dn) or dev is not None:
        import torch
        from . import _device as device_arrays
        if _is_tensor(dn):
            dn = device_arrays.as_tensor(dn, dev if dev is not None else device_arrays.device_of(dn)).contiguous()
        else:  # its own bytes through page-locked staging (int16 carries the uint16 bits)
            host = np.ascontiguousarray(dn)
            dn = torch.from_numpy(host.view(np.int16) if kind == "uint16" else host).pin_memory().to(dev, non_blocking=True)
    else:
        dn = np.ascontiguousarray(dn)
    call = _Call(dn)
    outs = [call.empty((L, S), out_dtype), call.empty((L, S), out_dtype) if nesz else None,
            call.empty((L, S), out_dtype) if inc is not None else None, call.empty((L, S), np.uint8) if valid else None]
    if L * S:
        tables = [None if g is None else _table(call, g, line, sample) for g in grids]
        _launch(call, L, S, _lib.DN_F32 if kind == "float32" else _lib.DN_U16, out_dtype, dn, tables, fill, outs)
    return Calibrated(*outs)
