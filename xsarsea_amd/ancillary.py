"""The inversion's a-priori wind raster from a coarse model grid, computed on the device.

    ancillary_from_model(U10, V10, model_lon, model_lat, TiePoints(...), shape=sigma0.shape) -> invert_from_model / Streaks.resolve

Every entry of the inversion chain takes the a-priori wind as a full-resolution complex128 raster in antenna convention.  The
reference's notebook docs/examples/windspeed_retrieval_L1.ipynb builds it by hand, per pixel, from model rasters resampled
elsewhere:

    direction = (90 - rad2deg(arctan2(V10, U10)) + 180) % 360
    wind      = sqrt(U10**2 + V10**2) * exp(1j * dir_meteo_to_sample(direction, ground_heading))

`ancillary_from_model` computes the same raster from what carries the information: the model's `U10` / `V10` on their own regular
longitude / latitude grid (a few hundred nodes under a scene) and the scene's geolocation on its tie-point grid (`TiePoints`).
Only these kilobytes cross the link; one HIP kernel (csrc/xsw_ancillary.hip, include/xsw.h: xsw_ancillary_model) interpolates
both and writes the 16 B per pixel once, in the closed form -(u + 1j v) * (cos h + 1j sin h) of the three lines above.  Brackets,
the longitude continuity step, the uniformity rule and the heading's cosine / sine tables are host arithmetic on the small grids;
every host check runs before any device call.

Containers as in `streaks`: numpy in and no `device=` gives numpy out (through host buffers, synchronous); a device tensor among
the model fields, or `device=`, gives a device tensor, computed asynchronously on the caller's current stream.
"""
import numpy as np

from ._raster import _Call, _coord_values, _is_tensor, _small, _unwrap
from .streaks import bracket

__all__ = ["TiePoints", "ancillary_from_model", "UNIFORM_TOLERANCE"]

UNIFORM_TOLERANCE = 1e-3  # of a step: how far a model node may lie from first + k * step


def _axis(v, what):
    a = np.asarray(_coord_values(v), dtype=np.float64)
    if a.ndim != 1 or len(a) < 1:
        raise ValueError(f"{what} must be a non-empty vector, not of shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds a NaN or an infinity")
    return a


def _continuous(lon):
    """lon - 360 * K with the whole turns K that leave no neighbours more than 180 apart: K accumulates round(difference / 360)
    of the raw neighbours, down the first column and then along every line."""
    turns = lambda a: np.cumsum(np.round(np.diff(a, axis=-1, prepend=a[..., :1]) / 360.0), axis=-1)
    out = lon - 360.0 * (turns(lon[:, 0])[:, None] + turns(lon))
    if (np.abs(np.diff(out, axis=0)) > 180.0).any():
        raise ValueError("the tie longitudes cannot be made continuous: neighbouring lines differ by more than 180 degrees")
    return out


class TiePoints:
    """The scene's geolocation on its tie-point grid: `line[nl]`, `sample[ns]` (strictly ascending, not necessarily uniform, one
    point or more each) and `longitude`, `latitude`, `ground_heading` [nl, ns] in degrees; the heading is the azimuth of the line
    axis from north, as in `dir_meteo_to_sample`.  Host arrays, or objects with `.values`.  A longitude grid that crosses the
    antimeridian is made continuous (whole multiples of 360 added, so that no neighbours differ by more than 180); a NaN
    anywhere raises ValueError.  `cos_heading` / `sin_heading` are the tables the kernel blends instead of the angle."""

    def __init__(self, line, sample, longitude, latitude, ground_heading):
        self.line, self.sample = _axis(line, "tie-point line"), _axis(sample, "tie-point sample")
        for a, what in ((self.line, "line"), (self.sample, "sample")):
            if len(a) > 1 and not (np.diff(a) > 0).all():
                raise ValueError(f"tie-point {what} coordinates must be strictly ascending")
        shape = (len(self.line), len(self.sample))
        grids = []
        for v, what in ((longitude, "longitude"), (latitude, "latitude"), (ground_heading, "ground_heading")):
            a = np.asarray(_coord_values(v), dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"tie-point {what} must be [line, sample] = {shape}, not {a.shape}")
            if not np.isfinite(a).all():
                raise ValueError(f"tie-point {what} holds a NaN or an infinity")
            grids.append(a)
        self.longitude, self.latitude, self.ground_heading = _continuous(grids[0]), grids[1], grids[2]
        h = np.deg2rad(self.ground_heading)
        self.cos_heading, self.sin_heading = np.cos(h), np.sin(h)

    @property
    def shape(self):
        return len(self.line), len(self.sample)


def _uniform_axis(v, what):
    """(first, step, n, last) of a uniform axis of two nodes or more: step = (last - first) / (n - 1), and every node within
    UNIFORM_TOLERANCE * |step| of first + k * step.  A real irregularity (a Gaussian grid) is refused, not silently bent."""
    a = _axis(v, what)
    n = len(a)
    if n < 2:
        raise ValueError(f"{what} needs two nodes or more")
    step = (a[-1] - a[0]) / (n - 1)
    if step == 0.0 or not np.isfinite(step):
        raise ValueError(f"{what} has no extent")
    off = np.abs(a - (a[0] + np.arange(n) * step))
    if not (off <= UNIFORM_TOLERANCE * abs(step)).all():
        k = int(np.argmax(off))
        raise ValueError(f"{what} is not uniform: node {k} lies {off[k] / abs(step):.3g} of a step from first + k * step "
                         f"(at most {UNIFORM_TOLERANCE:g}); non-uniform model grids are not supported")
    return float(a[0]), float(step), n, float(a[-1])


def _raster_axis(coords, tie, what):
    c = np.asarray(_coord_values(coords), dtype=np.float64)
    if c.ndim != 1:
        raise ValueError(f"raster {what} coordinates must be a vector, not of shape {c.shape}")
    if not np.isfinite(c).all():
        raise ValueError(f"raster {what} coordinates hold a NaN or an infinity")
    if len(c) and (c.min() < tie[0] or c.max() > tie[-1]):
        raise ValueError(f"raster {what} coordinates {c.min():g} .. {c.max():g} leave the tie points' span {tie[0]:g} .. {tie[-1]:g}: "
                         "geolocation is not extrapolated")
    if len(tie) == 1 and len(c) > 1:
        raise ValueError(f"a single tie-point {what} serves a raster of that one {what} only")
    return c


def _field_meta(a, what):
    shape = tuple(a.shape)
    name = str(a.dtype).replace("torch.", "")
    if len(shape) != 2:
        raise ValueError(f"{what} must be [n_lat, n_lon], not of shape {shape}")
    if name not in ("float32", "float64"):
        raise ValueError(f"{what} must be float32 or float64, not {name}")
    return shape, name


def ancillary_from_model(model_u, model_v, model_lon, model_lat, tie_points, line=None, sample=None, shape=None, device=None):
    """The a-priori wind raster of the inversion (complex128 [L, S], antenna convention) from a model wind on its own grid.

    model_u / model_v: [n_lat, n_lon], float32 or float64 (the same for both; the arithmetic is float64), the eastward /
    northward components of the wind ("blowing to"); numpy, or already device tensors.  model_lon[n_lon] ascending,
    model_lat[n_lat] ascending or descending (a descending axis gives what the flipped grid gives, bit for bit), two nodes or more
    each and uniform: with step = (last - first) / (n - 1) every node
    lies within 1e-3 * |step| of first + k * step, else ValueError.  The longitude axis is periodic iff n_lon * step is 360 within
    the same rule.  tie_points: the scene's `TiePoints`.  The raster's coordinate vectors are `line` / `sample`, or np.arange of
    `shape=(L, S)`: exactly one of the two forms; every coordinate lies inside the tie points' span (geolocation is not
    extrapolated), else ValueError.

    Per pixel: longitude, latitude, cos and sin of the heading bilinear between the four tie points around it (`streaks.bracket`
    per axis), the heading vector renormalised by one hypot (NaN where the headings cancel); u, v bilinear over the model cell's
    four nodes in plain arithmetic (a NaN node makes the pixel NaN, also at weight 0); out = -(u + 1j v) * (cos h + 1j sin h): the
    GMF's "from" sense, with heading 0 a wind blowing to the east gives -speed.  Outside a regional grid the pixel is NaN + NaN j
    (the last node is inside); a periodic longitude axis wraps.  include/xsw.h (xsw_ancillary_model) fixes the operation order;
    tests/ancillary_model_ref.py restates it in numpy, bit for bit.

    Returns numpy when `device` is None and neither field is a device tensor (host buffers, synchronous); otherwise a device
    tensor on `device` (or the fields' device), computed asynchronously on torch's current stream."""
    if not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    coords = line is not None or sample is not None
    if coords == (shape is not None):
        raise ValueError("give the raster as shape=(L, S) or as line= and sample=: exactly one of the two forms")
    if coords and (line is None or sample is None):
        raise ValueError("line= and sample= go together")
    if shape is not None:
        if len(tuple(shape)) != 2 or min(int(v) for v in shape) < 0:
            raise ValueError(f"shape must be (L, S), not {shape}")
        line, sample = np.arange(int(shape[0])), np.arange(int(shape[1]))
    line, sample = _raster_axis(line, tie_points.line, "line"), _raster_axis(sample, tie_points.sample, "sample")
    u, v = _unwrap(model_u), _unwrap(model_v)
    u, v = (a if _is_tensor(a) else np.asarray(a) for a in (u, v))
    (ushape, udtype), (vshape, vdtype) = _field_meta(u, "model_u"), _field_meta(v, "model_v")
    if ushape != vshape or udtype != vdtype:
        raise ValueError(f"model_u {ushape} {udtype} and model_v {vshape} {vdtype} must have one shape and one dtype")
    lon0, dlon, n_lon, _ = _uniform_axis(model_lon, "model_lon")
    lat0, dlat, n_lat, lat_last = _uniform_axis(model_lat, "model_lat")
    if dlon < 0:
        raise ValueError("model_lon must ascend")
    if ushape != (n_lat, n_lon):
        raise ValueError(f"model_u / model_v {ushape} do not match the axes [n_lat, n_lon] = ({n_lat}, {n_lon})")
    periodic = abs(n_lon * dlon - 360.0) <= UNIFORM_TOLERANCE * abs(dlon)
    lf, lt = bracket(tie_points.line, line)
    sf, st = bracket(tie_points.sample, sample)
    L, S = len(line), len(sample)

    # the device from here on
    if device is not None or _is_tensor(u) or _is_tensor(v):
        import torch
        from . import _device
        dev = torch.device(device) if device is not None else _device.device_of(u, v)
        if dev.type != "cuda":
            raise ValueError(f"device must be a GPU, not {dev}")
        up = lambda a: _device.as_tensor(a, dev) if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)
        u, v = up(u), up(v)
    call = _Call(u, v)
    if dlat < 0:  # a descending latitude axis is the ascending one read backwards: the same bits as the flipped grid gives
        lat0, dlat = lat_last, -dlat
        u, v = (a.flip(0) if call.device else a[::-1] for a in (u, v))
    u, v = call.prep(u), call.prep(v)
    out = call.empty((L, S), np.complex128)
    if L * S:
        tables = [_small(call, a, np.float64) for a in (tie_points.longitude, tie_points.latitude, tie_points.cos_heading, tie_points.sin_heading)]
        lf, lt, sf, st = _small(call, lf, np.int32), _small(call, lt, np.float64), _small(call, sf, np.int32), _small(call, st, np.float64)
        call.launch("ancillary_model_raw", L, S, call.mem, call.xsw_dtype(u), u, v, n_lat, n_lon, lon0, dlon, int(periodic), lat0, dlat,
                    len(tie_points.line), len(tie_points.sample), *tables, lf, lt, sf, st, out)
    return out
