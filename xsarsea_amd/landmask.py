"""The sea / land keep mask of a scene from coastline polygons, computed on the device.

    land_mask(Coastline(rings), TiePoints(...), shape=sigma0.shape, and_with=calibrated.valid) -> keep= / mask= / and_with=

Every product call takes a `keep=` / `mask=` / `and_with=` byte raster; `calibrate_dn` makes one from fill values and
`filtering_parameters` one from heterogeneity.  This module makes the one that comes from geography.  What carries the information
is a few thousand coastline edges and the scene's `TiePoints`: kilobytes.  One HIP kernel (csrc/xsw_landmask.hip, include/xsw.h:
xsw_land_mask) finds every pixel's longitude and latitude with the arithmetic of `ancillary_from_model` and decides land or water
by the even-odd rule over the edges, 1 B per pixel written once.

The rule is stated in include/xsw.h in a form with no division and no library call (half-open in latitude, with the two
longitude-range clauses "an edge wholly west never counts, one wholly east always does" as part of the definition), so
tests/landmask_ref.py restates it in numpy and the GPU tests ask for equal bytes.

Host side (numpy, no device needed: `plan`): the whole turns that bring the coastline to the scene's continuous longitudes, the
edges that cannot matter dropped, the rest sorted into latitude bands.  A band decides which edges a pixel is tested against,
never what an edge answers.

Containers as in `ancillary`: no `device=` and no device `and_with` gives numpy out (through host buffers, synchronous); otherwise
a device tensor, computed asynchronously on the caller's current stream.
"""
import os

import numpy as np

from ._raster import _Call, _as_u8, _is_tensor, _small, _unwrap
from .ancillary import TiePoints, _raster_axis
from .streaks import bracket

__all__ = ["Coastline", "LandPlan", "land_mask", "plan", "SPAN_MARGIN", "MIN_BAND_HEIGHT", "EDGES_PER_BAND", "MAX_BANDS"]

SPAN_MARGIN = 1e-9       # degrees by which the tie nodes' longitude / latitude span is widened before anything is dropped
MIN_BAND_HEIGHT = 0.005  # degrees: no band is thinner (about 550 m)
EDGES_PER_BAND = 16      # n_bands is the edge count over this ...
MAX_BANDS = 65536        # ... and at most this


def _rings_of(obj):
    """Every ring ([n, 2] sequences) of a ring list or of an object with `__geo_interface__`, exterior and interior alike."""
    geo = getattr(obj, "__geo_interface__", None)
    if geo is None and isinstance(obj, dict) and "type" in obj:
        geo = obj
    if geo is None:
        if isinstance(obj, np.ndarray) and obj.ndim == 2:
            return [obj]
        out = []
        for item in obj:
            if hasattr(item, "__geo_interface__") or (isinstance(item, dict) and "type" in item):
                out += _rings_of(item)
            else:
                out.append(item)
        return out
    kind = geo.get("type")
    if kind == "Polygon":
        return list(geo["coordinates"])
    if kind == "MultiPolygon":
        return [ring for poly in geo["coordinates"] for ring in poly]
    if kind == "GeometryCollection":
        return [ring for g in geo["geometries"] for ring in _rings_of(g)]
    if kind == "Feature":
        return _rings_of(geo["geometry"]) if geo.get("geometry") is not None else []
    if kind == "FeatureCollection":
        return [ring for f in geo["features"] for ring in _rings_of(f)]
    raise ValueError(f"a coastline is made of Polygon, MultiPolygon, GeometryCollection, Feature or FeatureCollection objects, not {kind!r}")


def _ring(ring, k):
    """The continuous, open vertex list [n, 2] of ring k: the repeated closing vertex dropped, longitudes made continuous by
    whole turns accumulated along the ring (round(difference / 360) of the raw neighbours, as `TiePoints` does along a line)."""
    a = np.asarray(ring, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError(f"ring {k} must be [n, 2] (longitude, latitude), not of shape {a.shape}")
    a = a[:, :2]
    if not np.isfinite(a).all():
        raise ValueError(f"ring {k} holds a NaN or an infinity")
    if len(a) > 1 and (a[0] == a[-1]).all():
        a = a[:-1]
    if len(a) < 3:
        raise ValueError(f"ring {k} has fewer than 3 vertices")
    lon = a[:, 0] - 360.0 * np.cumsum(np.round(np.diff(a[:, 0], prepend=a[:1, 0]) / 360.0))
    return np.stack([lon, a[:, 1]], axis=1)


class Coastline:
    """Coastline polygons as the edges the even-odd rule counts.

    rings: an iterable of rings, each `[n, 2]` (longitude, latitude) in degrees, and / or of objects with `__geo_interface__`
    (`Polygon`, `MultiPolygon`, `GeometryCollection`, `Feature`, `FeatureCollection`; duck-typed, nothing is imported); one such
    object alone passes too.  Exterior and interior rings are taken alike: a lake in an island in a lake comes out right by
    parity.  Per ring a repeated closing vertex is dropped and an open ring is closed; fewer than 3 vertices, a NaN or an infinity
    raise ValueError; a jump of more than 180 degrees between consecutive vertices is made continuous (whole turns accumulated
    along the ring), so a ring across the antimeridian may be given wrapped.  A longitude extent above 360 raises ValueError
    (exactly 360, a global file, is fine).

    edges: float64 `[E, 4]` = x1, y1, x2, y2; edges with y1 == y2 (zero-length ones among them) are dropped, because by the
    statement they never count.  n_rings; bbox = (lon_min, lat_min, lon_max, lat_max) of all vertices (None without rings)."""

    def __init__(self, rings):
        rings = [_ring(r, k) for k, r in enumerate(_rings_of(rings))]
        self.n_rings = len(rings)
        if rings:
            pts = np.concatenate(rings)
            self.bbox = (float(pts[:, 0].min()), float(pts[:, 1].min()), float(pts[:, 0].max()), float(pts[:, 1].max()))
            if self.bbox[2] - self.bbox[0] > 360.0:
                raise ValueError(f"the coastline spans {self.bbox[2] - self.bbox[0]:g} degrees of longitude: more than 360")
            e = np.concatenate([np.concatenate([r, np.roll(r, -1, axis=0)], axis=1) for r in rings])
            self.edges = np.ascontiguousarray(e[e[:, 1] != e[:, 3]])
        else:
            self.bbox = None
            self.edges = np.empty((0, 4))


class LandPlan:
    """What one call hands to the kernel: `edges` [E, 4] (the turn copies that can reach the scene, less the edges that cannot
    matter), and the bands `band_start` [n_bands + 1], `band_edges` (int32 CSR: the edges of band b are
    band_edges[band_start[b]:band_start[b + 1]], by descending xmax) of height `h` from `lat0`.  `turns`: the whole turns copied;
    `span` = (lon_min, lon_max, lat_min, lat_max) of the scene as widened."""

    def __init__(self, edges, band_start, band_edges, lat0, h, turns, span):
        self.edges, self.band_start, self.band_edges, self.lat0, self.h, self.turns, self.span = edges, band_start, band_edges, lat0, h, turns, span

    @property
    def n_bands(self):
        return len(self.band_start) - 1

    @property
    def mean_band_edges(self):
        """Edges listed per band, averaged over the bands: at most this many edges are tested per pixel of an evenly spread
        scene (the walk stops at the first edge west of the pixel)."""
        return len(self.band_edges) / self.n_bands

    def band_of(self, lat):
        """The kernel's band index of a latitude: clamp(floor((lat - lat0) / h), 0, n_bands - 1)."""
        return np.clip(np.floor((np.asarray(lat, dtype=np.float64) - self.lat0) / self.h), 0, self.n_bands - 1).astype(np.int64)


def _forced_bands():
    v = os.environ.get("XSW_LAND_BANDS")
    if v is None:
        return None
    try:
        n = int(v)
    except ValueError:
        n = 0
    if not 1 <= n <= MAX_BANDS:
        raise ValueError(f"XSW_LAND_BANDS must be a whole number in 1 .. {MAX_BANDS}, not {v!r}")
    return n


def _land_path():
    v = os.environ.get("XSW_LAND_PATH")
    if v is not None and v not in ("direct", "bands"):
        raise ValueError(f"XSW_LAND_PATH must be direct or bands, not {v!r}")
    return v or "bands"


def plan(coastline, tie_points, n_bands=None):
    """The `LandPlan` of a coastline under a scene (numpy only).

    Span: the minimum and maximum of the tie nodes' continuous longitudes and of their latitudes, each widened by SPAN_MARGIN
    (1e-9 degrees).  A pixel's position is a blend of four nodes with weights t, 1 - t in [0, 1] on each axis, four products and
    three sums, each rounded once: it leaves the nodes' range by less than 4 ulp of the largest node magnitude (at most
    4 * 2**-52 * 720 < 7e-13 degrees for longitudes within two turns), which the margin covers a thousandfold.

    Turns: for every whole k with bbox.lon_min + 360 k <= span.lon_max and bbox.lon_max + 360 k >= span.lon_min the edges are
    copied with x + 360.0 * k (one rounded add per vertex); the mask is the parity over the union.  Whole rings are copied, so a
    copy that cannot reach the scene would add an even number of hits to every pixel: leaving it out is exact.

    Drops, both exact by the statement: an edge hits only pixels with min(y1, y2) <= py < max(y1, y2), so one whose latitude
    range misses the span never counts; one with xmax < span.lon_min is west of every pixel and never counts.

    Bands: n_bands bands of height h = (span.lat_max - span.lat_min) / n_bands from lat0 = span.lat_min.  The kernel's band index
    clamp(floor((lat - lat0) / h), 0, n_bands - 1) is monotone in lat, so the pixels an edge can hit lie in the bands from that of
    min(y1, y2) to that of max(y1, y2), computed here by the same expression; the edge is listed in those and in one more on
    either side.  Within a band the edges are ordered by descending xmax.
    n_bands: the argument, else XSW_LAND_BANDS (read at every call), else
    clamp(ceil(E / EDGES_PER_BAND), 1, min(MAX_BANDS, floor(extent / MIN_BAND_HEIGHT))) with E the edges kept and extent the
    span's latitude extent (1 when that gives none)."""
    if not isinstance(coastline, Coastline):
        raise TypeError("coastline must be a Coastline")
    if not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    forced = _forced_bands() if n_bands is None else int(n_bands)
    if forced is not None and not 1 <= forced <= MAX_BANDS:
        raise ValueError(f"n_bands must be in 1 .. {MAX_BANDS}, not {forced}")
    lon_a, lon_b = float(tie_points.longitude.min()) - SPAN_MARGIN, float(tie_points.longitude.max()) + SPAN_MARGIN
    lat_a, lat_b = float(tie_points.latitude.min()) - SPAN_MARGIN, float(tie_points.latitude.max()) + SPAN_MARGIN
    span = (lon_a, lon_b, lat_a, lat_b)
    edges, turns = np.empty((0, 4)), []
    if len(coastline.edges):
        x_min, _, x_max, _ = coastline.bbox
        turns = list(range(int(np.ceil((lon_a - x_max) / 360.0)), int(np.floor((lon_b - x_min) / 360.0)) + 1))
        if turns:
            edges = np.concatenate([coastline.edges + np.array([360.0 * k, 0.0, 360.0 * k, 0.0]) for k in turns])
    y_lo, y_hi = np.minimum(edges[:, 1], edges[:, 3]), np.maximum(edges[:, 1], edges[:, 3])
    keep = (y_hi >= lat_a) & (y_lo <= lat_b) & (np.maximum(edges[:, 0], edges[:, 2]) >= lon_a)
    edges, y_lo, y_hi = np.ascontiguousarray(edges[keep]), y_lo[keep], y_hi[keep]
    extent = lat_b - lat_a
    if forced is None:
        forced = int(min(max(-(-len(edges) // EDGES_PER_BAND), 1), min(MAX_BANDS, max(int(extent / MIN_BAND_HEIGHT), 1))))
    out = LandPlan(edges, np.zeros(forced + 1, np.int32), np.empty(0, np.int32), lat_a, extent / forced, turns, span)
    if len(edges):
        first, last = np.maximum(out.band_of(y_lo) - 1, 0), np.minimum(out.band_of(y_hi) + 1, forced - 1)
        count = last - first + 1
        edge = np.repeat(np.arange(len(edges)), count)
        band = np.repeat(first, count) + (np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count))
        order = np.lexsort((edge, -np.maximum(edges[edge, 0], edges[edge, 2]), band))  # by band, then descending xmax
        out.band_edges = edge[order].astype(np.int32)
        out.band_start = np.concatenate([[0], np.cumsum(np.bincount(band, minlength=forced))]).astype(np.int32)
    return out


def land_mask(coastline, tie_points, line=None, sample=None, shape=None, and_with=None, invert=False, device=None):
    """The sea / land keep mask of a scene: uint8 `[L, S]`, 1 = water (keep), 0 = land; `invert=True` swaps them.

    coastline: a `Coastline`.  tie_points: the scene's `TiePoints`.  The raster's coordinate vectors are `line` / `sample`, or
    np.arange of `shape=(L, S)`: exactly one of the two forms; every coordinate lies inside the tie points' span (geolocation is
    not extrapolated), else ValueError -- as for `ancillary_from_model`.  and_with: a bool / uint8 raster of the output's shape
    (numpy or a device tensor; non-zero counts as 1), AND-ed into the result after the inversion, so that `Calibrated.valid` folds
    in the same pass.

    Per pixel: longitude and latitude bilinear between the four tie points around it (the arithmetic of `ancillary_from_model`),
    then the parity of the edges hit, by the statement of include/xsw.h (xsw_land_mask); coastline longitudes are brought to the
    scene's continuous ones by whole turns (`plan`).  tests/landmask_ref.py restates the call in numpy, byte for byte.

    Environment, read at every call: XSW_LAND_PATH = direct | bands (default bands; `direct` tests every pixel against every
    edge), XSW_LAND_BANDS = n forces the number of latitude bands (1 .. 65536).  Neither changes a byte.

    Returns numpy when `device` is None and `and_with` is not a device tensor (host buffers, synchronous); otherwise a device
    tensor on `device` (or and_with's device), computed asynchronously on torch's current stream.  Every host check (TypeError /
    ValueError) runs before any device call."""
    if not isinstance(coastline, Coastline):
        raise TypeError("coastline must be a Coastline")
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
    L, S = len(line), len(sample)
    if and_with is not None:
        and_with = _unwrap(and_with)
        and_with = and_with if _is_tensor(and_with) else np.asarray(and_with)
        if str(and_with.dtype).replace("torch.", "") not in ("bool", "uint8"):
            raise TypeError(f"and_with must be bool or uint8, not {and_with.dtype}")
        if tuple(and_with.shape) != (L, S):
            raise ValueError(f"and_with has shape {tuple(and_with.shape)}, the mask has shape {(L, S)}")
    direct = _land_path() == "direct"
    p = plan(coastline, tie_points)
    lf, lt = bracket(tie_points.line, line)
    sf, st = bracket(tie_points.sample, sample)

    # the device from here on
    if device is not None or _is_tensor(and_with):
        import torch
        from . import _device
        dev = torch.device(device) if device is not None else _device.device_of(and_with)
        if dev.type != "cuda":
            raise ValueError(f"device must be a GPU, not {dev}")
        out = torch.empty((L, S), dtype=torch.uint8, device=dev)
        if and_with is not None and not _is_tensor(and_with):
            and_with = torch.from_numpy(np.ascontiguousarray(and_with)).pin_memory().to(dev, non_blocking=True)
        call = _Call(out)
    else:
        call = _Call()
        out = np.empty((L, S), np.uint8)
    if L * S:
        and_with = None if and_with is None else _as_u8(call, and_with)
        tables = [_small(call, a, np.float64) for a in (tie_points.longitude, tie_points.latitude)]
        tables += [_small(call, lf, np.int32), _small(call, lt, np.float64), _small(call, sf, np.int32), _small(call, st, np.float64)]
        n_edges, n_list = len(p.edges), len(p.band_edges)
        edges = _small(call, p.edges, np.float64) if n_edges else None
        bands = (0, None, 0, None)
        if not direct and n_list:
            bands = (p.n_bands, _small(call, p.band_start, np.int32), n_list, _small(call, p.band_edges, np.int32))
        call.launch("land_mask_raw", L, S, call.mem, len(tie_points.line), len(tie_points.sample), *tables, n_edges, edges, *bands,
                    p.lat0, p.h, and_with, int(bool(invert)), out)
    return out
