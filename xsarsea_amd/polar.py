"""Wind around a given centre: the storm-centred description of a cyclone scene, binned on the device.

    p = wind_polar(wind, TiePoints(...), centre=(lon, lat), radius=(dr_km, n_r), sectors=n_theta)
    p = invert_copol_codes(...).polar(tie_points, centre=..., radius=..., sectors=...)           # the same from the 4-byte codes
    wind_polar(lower_tile, tie_points, line=its_lines, centre=..., radius=..., sectors=..., into=p)   # a scene in row tiles
    p += p_of_another_rank                                                                        # per-rank sums merged
    p.ring_profile(), p.vmax_rmax(), p.wind_radii()                                               # profile, Vmax / Rmax, R34 / R50 / R64

Every valid pixel is geolocated from the scene's tie points, laid on a local chart around the centre (x east, y north, in km:
the equirectangular chart at the mid-latitude, without a trigonometric call), rotated to its east / north components with its
own heading and from there to the radial (outward) and tangential (positive counter-clockwise) components.  It falls into one of
`n_r` rings of width `dr_km` and one of `n_theta` sectors, counted clockwise from north, and adds five 64-bit integers to that bin
-- 1, |wind|, the radial and the tangential component in units of 2**-24 m/s, |wind|**2 in units of 2**-16 -- and raises a sixth,
the bin's largest |wind|, by an integer maximum (include/xsw.h: xsw_wind_polar; csrc/xsw_cells.hip: k_wind_polar).  Integer sums
and maxima have no order: as for `wind_grid`, the launch, the kernel's pre-aggregation, a split into row tiles and the number of
devices change no bit, and `WindPolar.merge` of per-rank `sums` is exact.  tests/polar_ref.py restates the whole call in numpy.

Containers as in `grid`: numpy in gives numpy out (through host buffers, synchronous); a device tensor in gives device tensors
out, computed asynchronously on torch's current stream.  Every host check precedes any device call.  The three helpers
(`ring_profile`, `vmax_rmax`, `wind_radii`) work on the host from the n_r x n_theta sums, a few kilobytes.
"""
import math
import operator

import numpy as np

from . import _lib
from ._raster import _Call, _as_u8, _is_tensor, _small
from .ancillary import TiePoints
from .cells import _keep, _source
from .grid import Q16, Q24, _grid_path, _pixel_axis
from .streaks import bracket

__all__ = ["PolarSpec", "WindPolar", "wind_polar", "codes_polar"]

PLANES = ("n", "Ss", "Sq", "Sr", "St", "Mx")  # the order of `WindPolar.sums`
MAX_SECTORS = 360                              # XSW_POLAR_MAX_SECTORS (csrc/xsw_cells.hip)
KT34, KT50, KT64 = 17.4911, 25.7222, 32.9244   # 34 / 50 / 64 kt in m/s


class PolarSpec:
    """The bins of a `WindPolar`: `n_r` rings of width `dr_km` around `centre = (lon, lat)` in degrees, ring k covering
    [k dr_km, (k + 1) dr_km); `n_theta` sectors per ring, clockwise from north, a multiple of 4 up to 360, so that the quadrants
    NE, SE, SW, NW are whole sectors.  The centre's longitude is kept as lon - 360 rint(lon / 360): -179.6 and 180.4 are one
    centre.  |lat| <= 89."""

    def __init__(self, centre, radius, sectors):
        try:
            lon, lat = centre
        except (TypeError, ValueError):
            raise ValueError(f"centre must be (lon, lat), not {centre!r}") from None
        try:
            lon, lat = float(lon), float(lat)
        except (TypeError, ValueError):
            raise TypeError(f"centre must be two numbers, not {centre!r}") from None
        if not (math.isfinite(lon) and math.isfinite(lat)):
            raise ValueError(f"centre must be two finite numbers, not {(lon, lat)}")
        if abs(lat) > 89.0:
            raise ValueError(f"the centre's latitude must lie within 89 degrees of the equator, not at {lat}")
        try:
            dr_km, n_r = radius
        except (TypeError, ValueError):
            raise ValueError(f"radius must be (dr_km, n_r), not {radius!r}") from None
        try:
            n_r, n_theta = operator.index(n_r), operator.index(sectors)
        except TypeError:
            raise TypeError(f"n_r and sectors must be integers, not {n_r!r} and {sectors!r}") from None
        try:
            dr_km = float(dr_km)
        except (TypeError, ValueError):
            raise TypeError(f"dr_km must be a number, not {dr_km!r}") from None
        if not (math.isfinite(dr_km) and dr_km > 0.0):
            raise ValueError(f"dr_km must be finite and positive, not {dr_km}")
        if n_r < 1:
            raise ValueError(f"n_r must be 1 or more, not {n_r}")
        if n_theta < 4 or n_theta % 4 != 0 or n_theta > MAX_SECTORS:
            raise ValueError(f"sectors must be a multiple of 4 from 4 to {MAX_SECTORS}, not {n_theta}")
        if n_r * n_theta > 0x7fffffff:
            raise ValueError(f"n_r * sectors = {n_r * n_theta} bins do not fit int32")
        self.lon_c, self.lat_c = lon - 360.0 * float(np.rint(lon / 360.0)), lat
        self.dr_km, self.n_r, self.n_theta = dr_km, n_r, n_theta

    def key(self):
        return self.lon_c, self.lat_c, self.dr_km, self.n_r, self.n_theta

    def __eq__(self, other):
        return isinstance(other, PolarSpec) and self.key() == other.key()

    def __repr__(self):
        return f"PolarSpec(centre={self.key()[:2]}, radius={self.key()[2:4]}, sectors={self.n_theta})"

    @property
    def shape(self):
        return self.n_r, self.n_theta

    def tables(self):
        """What the entry takes besides the spec itself: (cos, sin of the centre's latitude, sin and cos [n_theta / 4 + 1] of the
        sector borders j * 90 / (n_theta / 4) degrees of one quadrant)."""
        lat = np.deg2rad(np.float64(self.lat_c))
        borders = np.deg2rad(np.arange(self.n_theta // 4 + 1, dtype=np.float64) * (90.0 / (self.n_theta // 4)))
        return float(np.cos(lat)), float(np.sin(lat)), np.sin(borders), np.cos(borders)


def _finish_host(n, ss, sq, sr, st, mx):
    """dict(wspd, wspd_std, vr, vt, vmax) from numpy int64 sums of one shape: `WindPolar._finish` on the host."""
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = n.astype(np.float64)
        wspd, vr, vt = (ss.astype(np.float64) / nd) * Q24, (sr.astype(np.float64) / nd) * Q24, (st.astype(np.float64) / nd) * Q24
        s1, s2 = ss.astype(np.float64) * Q24, sq.astype(np.float64) * Q16
        var = (s2 - (s1 * s1) / nd) / (nd - 1.0)
        std = np.where(n < 2, np.nan, np.sqrt(np.where(var < 0.0, 0.0, var)))
        vmax = np.where(n == 0, np.nan, mx.astype(np.float64) * Q24)
    return dict(wspd=wspd, wspd_std=std, vr=vr, vt=vt, vmax=vmax)


class WindPolar:
    """Result of `wind_polar` / `codes_polar` / `CopolCodes.polar`.  `sums`: int64 `[6, n_r, n_theta]` (numpy, or a torch tensor
    for a device source), the planes n, Ss, Sq, Sr, St, Mx; `spec`: the `PolarSpec`.  What follows from the sums is computed on
    first use in the container's own float64, in the order include/xsw.h states, and again after the sums changed through
    `into=` or `merge`: count (int64), wspd (the scalar mean, m/s), wspd_std (sample standard deviation, NaN below two pixels),
    vr, vt (mean radial, outward, and tangential, counter-clockwise, components), vmax (the bin's largest speed).  A bin without
    a pixel is NaN with count 0.  radius [n_r] (km), bearing [n_theta] (degrees clockwise from north): the bin centres (numpy).
    A bin is exact up to 2**30 pixels over everything accumulated."""

    def __init__(self, sums, spec):
        if not isinstance(spec, PolarSpec):
            raise TypeError("spec must be a PolarSpec")
        if tuple(sums.shape) != (6,) + spec.shape or str(sums.dtype).replace("torch.", "") != "int64":
            raise ValueError(f"sums must be int64 [6, n_r, n_theta] = {(6,) + spec.shape}, not {sums.dtype} {tuple(sums.shape)}")
        self.sums, self.spec = sums, spec
        self._finished = None

    def __getitem__(self, name):
        return getattr(self, name)

    @property
    def on_device(self):
        return _is_tensor(self.sums)

    @property
    def radius(self):
        return (np.arange(self.spec.n_r) + 0.5) * self.spec.dr_km

    @property
    def bearing(self):
        return (np.arange(self.spec.n_theta) + 0.5) * (360.0 / self.spec.n_theta)

    def _finish(self):
        """wspd, wspd_std, vr, vt, vmax from the sums: `*`, `/`, `-` and sqrt alone, one operation per step."""
        if self._finished is None:
            if self.on_device:
                import torch
                f64 = lambda a: a.to(torch.float64)
                # (filled on the device: a tensor made from a host scalar would wait for the stream)
                nan, zero = (torch.full((), v, dtype=torch.float64, device=self.sums.device) for v in (float("nan"), 0.0))
                n, ss, sq, sr, st, mx = self.sums.unbind(0)
                nd = f64(n)
                wspd, vr, vt = (f64(ss) / nd) * Q24, (f64(sr) / nd) * Q24, (f64(st) / nd) * Q24
                s1, s2 = f64(ss) * Q24, f64(sq) * Q16
                var = (s2 - (s1 * s1) / nd) / (nd - 1.0)
                std = torch.where(n < 2, nan, torch.sqrt(torch.where(var < 0.0, zero, var)))
                vmax = torch.where(n == 0, nan, f64(mx) * Q24)
                self._finished = dict(wspd=wspd, wspd_std=std, vr=vr, vt=vt, vmax=vmax)
            else:
                self._finished = _finish_host(*self.sums)
        return self._finished

    count = property(lambda self: self.sums[0])
    wspd = property(lambda self: self._finish()["wspd"])
    wspd_std = property(lambda self: self._finish()["wspd_std"])
    vr = property(lambda self: self._finish()["vr"])
    vt = property(lambda self: self._finish()["vt"])
    vmax = property(lambda self: self._finish()["vmax"])

    @property
    def inflow_angle(self):
        """degrees(atan2(-vr, vt)): how far the mean wind of a bin points inwards of the tangent, positive for inflow into a
        counter-clockwise vortex.  The one value of this class that is not pinned to the bit."""
        if self.on_device:
            import torch
            return torch.rad2deg(torch.atan2(-self.vr, self.vt))
        return np.degrees(np.arctan2(-self.vr, self.vt))

    def _same_bins(self, other, what):
        if not isinstance(other, WindPolar):
            raise TypeError(f"{what} must be a WindPolar, not {type(other).__name__}")
        if other.spec != self.spec:
            raise ValueError(f"{what} lies on {other.spec}, not on {self.spec}: sums of different bins cannot be merged")
        if other.on_device != self.on_device:
            raise ValueError(f"{what} holds {'device' if other.on_device else 'host'} sums, this one {'device' if self.on_device else 'host'} ones: "
                             "one container kind")

    def merge(self, other):
        """Merge another result's `sums` (the same `spec`, the same container kind; else ValueError) into this one's and return
        self: planes 0-4 are added, plane 5 becomes the maximum.  Exact: the form in which ranks or row tiles are combined."""
        self._same_bins(other, "the other result")
        if self.on_device:
            import torch
            o = other.sums.to(self.sums.device)
            self.sums[:5] += o[:5]
            torch.maximum(self.sums[5], o[5], out=self.sums[5])
        else:
            self.sums[:5] += other.sums[:5]
            np.maximum(self.sums[5], other.sums[5], out=self.sums[5])
        self._finished = None
        return self

    __iadd__ = merge

    # ---- the storm-centred helpers: on the host, from the n_r x n_theta sums
    def host_sums(self):
        """`sums` as a numpy array.  For device sums this download of a few kilobytes is the one synchronisation of the
        helpers below."""
        return self.sums.cpu().numpy() if self.on_device else np.asarray(self.sums)

    def ring_profile(self, min_coverage=0.5):
        """The azimuthal profile: dict(radius, count, coverage, wspd, wspd_std, vr, vt, vmax), each `[n_r]` (numpy).  The integer
        sums of a ring's sectors are added (the largest speed: their maximum) and finished as a bin is; `coverage` is the share
        of the ring's sectors that hold a pixel, and a ring below `min_coverage` is NaN in every finished field.  Works on the
        host; for device sums the download of `sums` is its only synchronisation."""
        s = self.host_sums()
        ring = [s[k].sum(axis=1) for k in range(5)] + [s[5].max(axis=1)]
        coverage = (s[0] > 0).sum(axis=1) / float(self.spec.n_theta)
        out = dict(radius=self.radius, count=ring[0], coverage=coverage)
        for name, a in _finish_host(*ring).items():
            out[name] = np.where(coverage >= min_coverage, a, np.nan)
        return out

    def vmax_rmax(self, min_coverage=0.5):
        """(the largest pixel speed inside the rings, the largest ring-mean speed of `ring_profile(min_coverage)`, the centre
        radius of that ring in km); on ties the first ring; NaN where there is no pixel or no ring of that coverage.  Works on
        the host; for device sums the download of `sums` is its only synchronisation."""
        s = self.host_sums()
        pixel_max = float(s[5].max()) * Q24 if (s[0] > 0).any() else float("nan")
        wspd = self.ring_profile(min_coverage)["wspd"]
        if np.isnan(wspd).all():
            return pixel_max, float("nan"), float("nan")
        k = int(np.nanargmax(wspd))
        return pixel_max, float(wspd[k]), float(self.radius[k])

    def wind_radii(self, thresholds=(KT34, KT50, KT64), min_count=1):
        """float64 `[len(thresholds), 4]`: per threshold (m/s; the default is 34 / 50 / 64 kt) and quadrant NE, SE, SW, NW, the
        radius in km at which the quadrant's mean speed falls to the threshold.  Per quadrant and ring the integer sums of the
        quadrant's sectors give the mean m_k (rings of fewer than `min_count` pixels have none).  With k the largest ring of
        m_k >= T the radius is r_k + dr_km (m_k - T) / (m_k - m_(k+1)), r_k the ring's centre.  NaN if no ring reaches T; NaN if
        k is the last ring of `min_count` pixels or more, because the radius then lies beyond the coverage; NaN also where ring
        k + 1 has no mean.  Works on the host; for device sums the download of `sums` is its only synchronisation."""
        min_count = max(int(min_count), 1)
        s = self.host_sums()
        mq, dr = self.spec.n_theta // 4, self.spec.dr_km
        out = np.full((len(thresholds), 4), np.nan)
        r = self.radius
        for quadrant in range(4):
            n = s[0][:, quadrant * mq:(quadrant + 1) * mq].sum(axis=1)
            ss = s[1][:, quadrant * mq:(quadrant + 1) * mq].sum(axis=1)
            have = n >= min_count
            with np.errstate(invalid="ignore", divide="ignore"):
                mean = np.where(have, (ss.astype(np.float64) / n.astype(np.float64)) * Q24, np.nan)
            if not have.any():
                continue
            last = int(np.nonzero(have)[0][-1])
            for i, T in enumerate(thresholds):
                above = np.nonzero(have & (mean >= float(T)))[0]
                if not len(above) or above[-1] == last:
                    continue
                k = int(above[-1])
                out[i, quadrant] = r[k] + dr * (mean[k] - float(T)) / (mean[k] - mean[k + 1])   # NaN where ring k + 1 has no mean
        return out


def _wind_polar(src, kind, what, tie_points, centre, radius, sectors, line, sample, keep, into, lut=None):
    # every host check
    keep = _keep(keep, src, what)
    if not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    L, S = (int(v) for v in src.shape)
    line, sample = _pixel_axis(line, L, tie_points.line, "line"), _pixel_axis(sample, S, tie_points.sample, "sample")
    spec = PolarSpec(centre, radius, sectors)
    _grid_path()
    if into is not None:
        if not isinstance(into, WindPolar):
            raise TypeError(f"into must be a WindPolar, not {type(into).__name__}")
        if into.spec != spec:
            raise ValueError(f"into lies on {into.spec}, the call asks for {spec}")
        if into.on_device != _is_tensor(src):
            raise ValueError(f"into holds {'device' if into.on_device else 'host'} sums but {what} is a {'device' if _is_tensor(src) else 'host'} array: "
                             "one container kind per call")
    lf, lt = bracket(tie_points.line, line)
    sf, st = bracket(tie_points.sample, sample)
    cos_c, sin_c, border_sin, border_cos = spec.tables()

    # the device from here on
    call = _Call(src)
    if call.device:
        from . import _device
        src = _device.as_tensor(src, call.dev).contiguous()
    else:
        src = np.ascontiguousarray(src)
    if into is None:
        sums = call.empty((6,) + spec.shape, np.int64)
        if call.device:
            sums.zero_()  # on the current stream, as the launch is
        else:
            sums.fill(0)
        out = WindPolar(sums, spec)
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
        borders = [_small(call, border_sin, np.float64), _small(call, border_cos, np.float64)]
        args = (L, S, call.mem, kind, src, keep, len(tie_points.line), len(tie_points.sample), *tables, spec.lon_c, spec.lat_c, cos_c, sin_c,
                spec.dr_km, spec.n_r, spec.n_theta, *borders, sums)
        if lut is None:
            call.launch("wind_polar_raw", *args)
        else:  # codes: the context must hold their LUT when the kernel reads `sol`
            from .windspeed import _engine
            is_array = lambda a: hasattr(a, "data_ptr") or isinstance(a, np.ndarray)

            def run(ctx, mem):
                with ctx.lock:
                    _engine.ensure_luts(ctx, lut, None)
                    ctx.wind_polar_raw(*[call.ptr(a) if is_array(a) else a for a in args])
            call.run(run, [a for a in args if is_array(a)])
        out._finished = None
    return out


def wind_polar(wind, tie_points, *, centre, radius, sectors, line=None, sample=None, keep=None, into=None):
    """`WindPolar` of a complex wind raster around centre = (lon, lat), in rings radius = (dr_km, n_r) and `sectors` sectors.

    wind: complex128 or complex64 `[L, S]`, antenna convention, numpy or a device tensor.  tie_points: the scene's `TiePoints`
    (required: every pixel is geolocated).  line / sample: the raster's coordinate vectors (default np.arange; a row tile passes
    its own lines); every coordinate lies inside the tie points' span.  The centre is the caller's (a best track, a fix from the
    scene): it may lie outside the raster.  A pixel counts iff its distance on the chart is below n_r * dr_km, neither part is
    NaN, its keep byte (bool / uint8 `[L, S]` in the raster's container kind) is non-zero, its heading is defined and its speed
    is below 256 m/s.

    into: a `WindPolar` of the same `PolarSpec` and container kind, which the call accumulates into (and returns): a scene in
    row tiles.  Any order gives the same bits.  Without it the sums start at zero.

    ValueError / TypeError for a wrong rank, dtype or container kind, a `keep` of another shape, `tie_points` that is not a
    `TiePoints`, coordinates outside the tie span, a centre that is not two finite numbers or lies beyond 89 degrees of latitude,
    dr_km <= 0, sectors that are no multiple of 4 (or more than 360), an `into` of another spec, an XSW_GRID_PATH other than
    `direct` or `lds` -- all before any device call."""
    src, name = _source(wind, "wind", ("complex128", "complex64"))
    return _wind_polar(src, _lib.CELLS_C128 if name == "complex128" else _lib.CELLS_C64, "wind", tie_points, centre, radius, sectors, line, sample,
                       keep, into)


def codes_polar(codes, lut_co, tie_points, *, centre, radius, sectors, line=None, sample=None, keep=None, into=None):
    """`wind_polar` from co-pol grid codes `[L, S]` (uint32 numpy, or an int32 / uint32 device tensor) of the LUT `lut_co`
    (`CopolCodes.polar` calls this): 4 B per pixel are read and nothing is expanded; bit for bit `wind_polar` of the complex128
    expansion."""
    src, _ = _source(codes, "codes", ("uint32", "int32"))
    if not _is_tensor(src):
        src = src.view(np.uint32)
    return _wind_polar(src, _lib.CELLS_CODES, "codes", tie_points, centre, radius, sectors, line, sample, keep, into, lut=lut_co)
