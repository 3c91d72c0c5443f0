"""The cyclone centre from the wind field: annulus scores on a lattice of candidate centres, summed on the device in one pass.

    s = wind_centre_scores(wind, TiePoints(...), first_guess=(lon, lat), step_km=2.0, n=17, annulus=(10.0, 30.0))
    s = invert_copol_codes(...).centre_scores(tie_points, first_guess=..., step_km=..., n=..., annulus=...)   # from the 4-byte codes
    wind_centre_scores(lower_tile, tie_points, line=its_lines, ..., into=s)                         # a scene in row tiles
    s += s_of_another_rank                                                                          # per-rank sums merged
    fix = s.best("vt")                                                                              # the circulation centre
    fix = find_centre(wind, tie_points, annulus=(10.0, 30.0))                                       # coarse to fine

`wind_polar` describes a cyclone around a centre the caller supplies; this module finds that centre in the scene itself.  The
candidates are the nodes of an `n x n` lattice, `step_km` apart, on the local chart of `polar` laid around a first guess.  Every
valid pixel adds to EVERY candidate whose annulus `r_in_km <= r < r_out_km` it lies in the five integers it adds to a bin of
`wind_polar` -- 1, |wind|, the radial and the tangential component around that candidate in units of 2**-24 m/s, |wind|**2 in
units of 2**-16 (include/xsw.h: xsw_wind_centre; csrc/xsw_cells.hip: k_wind_centre).  Integer sums have no order: as for `wind_grid`
and `wind_polar`, the launch, the kernel's staging, a split into row tiles and the number of devices change no bit, and
`CentreScores.merge` of per-rank `sums` is exact.  tests/centre_ref.py restates the whole call in numpy.

`CentreScores.best` picks a candidate from the few kilobytes of sums, on the host: the largest mean tangential wind ("vt", the
circulation or "simplex" centre of airborne-radar practice, for an annulus at about the radius of maximum wind), the highest
annulus-mean speed ("wspd"), the calmest disc ("calm", for `annulus=(0, r_eye)`) or the most uniform speed ("steady").
`find_centre` repeats the search on ever finer lattices, each laid around the best node of the one before.

Containers as in `polar`: numpy in gives numpy out (through host buffers, synchronous); a device tensor in gives device sums,
computed asynchronously on torch's current stream.  Every host check precedes any device call.
"""
import math
import operator
import os

import numpy as np

from . import _lib
from ._raster import _Call, _as_u8, _is_tensor, _small
from .ancillary import TiePoints
from .cells import _keep, _source
from .grid import Q16, Q24, _pixel_axis
from .streaks import bracket

__all__ = ["CentreSpec", "CentreScores", "CentreFix", "wind_centre_scores", "codes_centre_scores", "find_centre", "codes_find_centre"]

PLANES = ("n", "Ss", "Sq", "Sr", "St")  # the order of `CentreScores.sums`: planes 0-4 of `WindPolar.sums`
MAX_N = 31                              # XSW_CENTRE_MAX_N (csrc/xsw_cells.hip)
CRITERIA = ("vt", "wspd", "calm", "steady")
R_KM, D2R = 6371.0088, 0.017453292519943295
KX = R_KM * D2R


class CentreSpec:
    """The candidates of a `CentreScores`: the nodes of an `n x n` lattice (`n` odd, 1 to 31), `step_km` apart, on the chart of
    `polar` around `first_guess = (lon, lat)` in degrees (|lat| <= 89; the longitude is kept as lon - 360 rint(lon / 360)), and
    the annulus `(r_in_km, r_out_km)`, 0 <= r_in_km < r_out_km, in which a pixel counts for a candidate.  Row i of the lattice
    runs south to north, column j west to east; node ((n - 1) / 2, (n - 1) / 2) is the first guess.  With n == 1 `step_km` is
    not read and is kept as 0."""

    def __init__(self, first_guess, step_km, n, annulus):
        try:
            lon, lat = first_guess
        except (TypeError, ValueError):
            raise ValueError(f"first_guess must be (lon, lat), not {first_guess!r}") from None
        try:
            lon, lat = float(lon), float(lat)
        except (TypeError, ValueError):
            raise TypeError(f"first_guess must be two numbers, not {first_guess!r}") from None
        if not (math.isfinite(lon) and math.isfinite(lat)):
            raise ValueError(f"first_guess must be two finite numbers, not {(lon, lat)}")
        if abs(lat) > 89.0:
            raise ValueError(f"the first guess's latitude must lie within 89 degrees of the equator, not at {lat}")
        try:
            n = operator.index(n)
        except TypeError:
            raise TypeError(f"n must be an integer, not {n!r}") from None
        if n < 1 or n > MAX_N or n % 2 != 1:
            raise ValueError(f"n must be odd, from 1 to {MAX_N}, not {n}")
        if n > 1:
            try:
                step_km = float(step_km)
            except (TypeError, ValueError):
                raise TypeError(f"step_km must be a number, not {step_km!r}") from None
            if not (math.isfinite(step_km) and step_km > 0.0):
                raise ValueError(f"step_km must be finite and positive, not {step_km}")
        else:
            step_km = 0.0
        try:
            r_in, r_out = annulus
        except (TypeError, ValueError):
            raise ValueError(f"annulus must be (r_in_km, r_out_km), not {annulus!r}") from None
        try:
            r_in, r_out = float(r_in), float(r_out)
        except (TypeError, ValueError):
            raise TypeError(f"annulus must be two numbers, not {annulus!r}") from None
        if not (math.isfinite(r_in) and math.isfinite(r_out) and 0.0 <= r_in < r_out):
            raise ValueError(f"annulus must be finite with 0 <= r_in_km < r_out_km, not {(r_in, r_out)}")
        self.lon_g, self.lat_g = lon - 360.0 * float(np.rint(lon / 360.0)), lat
        self.step_km, self.n, self.r_in_km, self.r_out_km = step_km, n, r_in, r_out

    def key(self):
        return self.lon_g, self.lat_g, self.step_km, self.n, self.r_in_km, self.r_out_km

    def __eq__(self, other):
        return isinstance(other, CentreSpec) and self.key() == other.key()

    def __repr__(self):
        return f"CentreSpec(first_guess={self.key()[:2]}, step_km={self.step_km}, n={self.n}, annulus={self.key()[4:]})"

    @property
    def shape(self):
        return self.n, self.n

    def tables(self):
        """What the entry takes besides the spec itself: (cos, sin of the first guess's latitude)."""
        lat = np.deg2rad(np.float64(self.lat_g))
        return float(np.cos(lat)), float(np.sin(lat))

    @property
    def x_km(self):
        """East offsets `[n]` of the lattice's columns on the chart: (j - (n - 1) / 2) * step_km, the kernel's expression."""
        return (np.arange(self.n) - (self.n - 1) // 2).astype(np.float64) * self.step_km

    y_km = x_km  # north offsets [n] of the lattice's rows: the same values

    def _lonlat(self):
        """The candidates through the inverse of the chart: dy = y / R, lat = lat_g + dy / D, m of the chart's step 3,
        lon = lon_g + x / (K m), wrapped to [-180, 180)."""
        cos_g, sin_g = self.tables()
        x, y = np.meshgrid(self.x_km, self.y_km)
        dy = y / R_KM
        h = 0.5 * dy
        lat = self.lat_g + dy / D2R
        m = (cos_g - sin_g * h) - (0.5 * cos_g) * (h * h)
        lon = self.lon_g + x / (KX * m)
        return lon - 360.0 * np.floor((lon + 180.0) / 360.0), lat

    longitude = property(lambda self: self._lonlat()[0], doc="Longitudes `[n, n]` of the candidates, degrees in [-180, 180).")
    latitude = property(lambda self: self._lonlat()[1], doc="Latitudes `[n, n]` of the candidates, degrees.")


class CentreFix:
    """What `CentreScores.best` and `find_centre` return: the chosen candidate's `lon`, `lat` (degrees), `x_km`, `y_km` (its
    offsets from the first guess on the chart), its lattice indices `i` (south to north), `j` (west to east), its `score` (the
    criterion's own value: rotation * vt, the mean speed, or its standard deviation) and `on_border` (True where i or j is 0 or
    n - 1: the lattice may have been too small).  NaN with i = j = -1 where no candidate was eligible.  `levels`: the fixes of
    `find_centre`'s lattices, coarse to fine (empty for `best`)."""
    __slots__ = ("lon", "lat", "x_km", "y_km", "i", "j", "score", "on_border", "levels")

    def __init__(self, lon, lat, x_km, y_km, i, j, score, on_border, levels=()):
        self.lon, self.lat, self.x_km, self.y_km, self.i, self.j = lon, lat, x_km, y_km, i, j
        self.score, self.on_border, self.levels = score, on_border, tuple(levels)

    @property
    def found(self):
        return self.i >= 0

    def __repr__(self):
        return (f"CentreFix(lon={self.lon}, lat={self.lat}, x_km={self.x_km}, y_km={self.y_km}, i={self.i}, j={self.j}, score={self.score}, "
                f"on_border={self.on_border})")


def _finish_host(n, ss, sq, sr, st):
    """dict(wspd, wspd_std, vr, vt) from numpy int64 sums of one shape, in include/xsw.h's finishing order."""
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = n.astype(np.float64)
        wspd, vr, vt = (ss.astype(np.float64) / nd) * Q24, (sr.astype(np.float64) / nd) * Q24, (st.astype(np.float64) / nd) * Q24
        s1, s2 = ss.astype(np.float64) * Q24, sq.astype(np.float64) * Q16
        var = (s2 - (s1 * s1) / nd) / (nd - 1.0)
        std = np.where(n < 2, np.nan, np.sqrt(np.where(var < 0.0, 0.0, var)))
    return dict(wspd=wspd, wspd_std=std, vr=vr, vt=vt)


class CentreScores:
    """Result of `wind_centre_scores` / `codes_centre_scores` / `CopolCodes.centre_scores`.  `sums`: int64 `[5, n, n]` (numpy, or
    a torch tensor for a device source), the planes n, Ss, Sq, Sr, St per candidate; `spec`: the `CentreSpec`.  What follows
    from the sums is computed on first use in the container's own float64, in the order include/xsw.h states, and again after
    the sums changed through `into=` or `merge`: count (int64), wspd (the annulus-mean speed, m/s), wspd_std (sample standard
    deviation, NaN below two pixels), vr, vt (mean radial, outward, and tangential, counter-clockwise, components around the
    candidate).  A candidate without a pixel is NaN with count 0.  A candidate is exact up to 2**30 pixels over everything
    accumulated."""

    def __init__(self, sums, spec):
        if not isinstance(spec, CentreSpec):
            raise TypeError("spec must be a CentreSpec")
        if tuple(sums.shape) != (5,) + spec.shape or str(sums.dtype).replace("torch.", "") != "int64":
            raise ValueError(f"sums must be int64 [5, n, n] = {(5,) + spec.shape}, not {sums.dtype} {tuple(sums.shape)}")
        self.sums, self.spec = sums, spec
        self._finished = None

    def __getitem__(self, name):
        return getattr(self, name)

    @property
    def on_device(self):
        return _is_tensor(self.sums)

    def _finish(self):
        """wspd, wspd_std, vr, vt from the sums: `*`, `/`, `-` and sqrt alone, one operation per step."""
        if self._finished is None:
            if self.on_device:
                import torch
                f64 = lambda a: a.to(torch.float64)
                # (filled on the device: a tensor made from a host scalar would wait for the stream)
                nan, zero = (torch.full((), v, dtype=torch.float64, device=self.sums.device) for v in (float("nan"), 0.0))
                n, ss, sq, sr, st = self.sums.unbind(0)
                nd = f64(n)
                wspd, vr, vt = (f64(ss) / nd) * Q24, (f64(sr) / nd) * Q24, (f64(st) / nd) * Q24
                s1, s2 = f64(ss) * Q24, f64(sq) * Q16
                var = (s2 - (s1 * s1) / nd) / (nd - 1.0)
                std = torch.where(n < 2, nan, torch.sqrt(torch.where(var < 0.0, zero, var)))
                self._finished = dict(wspd=wspd, wspd_std=std, vr=vr, vt=vt)
            else:
                self._finished = _finish_host(*self.sums)
        return self._finished

    count = property(lambda self: self.sums[0])
    wspd = property(lambda self: self._finish()["wspd"])
    wspd_std = property(lambda self: self._finish()["wspd_std"])
    vr = property(lambda self: self._finish()["vr"])
    vt = property(lambda self: self._finish()["vt"])

    def _same_lattice(self, other, what):
        if not isinstance(other, CentreScores):
            raise TypeError(f"{what} must be a CentreScores, not {type(other).__name__}")
        if other.spec != self.spec:
            raise ValueError(f"{what} lies on {other.spec}, not on {self.spec}: sums of different lattices cannot be merged")
        if other.on_device != self.on_device:
            raise ValueError(f"{what} holds {'device' if other.on_device else 'host'} sums, this one {'device' if self.on_device else 'host'} ones: "
                             "one container kind")

    def merge(self, other):
        """Add another result's `sums` (the same `spec`, the same container kind; else ValueError) into this one's, all five
        planes, and return self.  Exact: the form in which ranks or row tiles are combined."""
        self._same_lattice(other, "the other result")
        if self.on_device:
            self.sums += other.sums.to(self.sums.device)
        else:
            self.sums += other.sums
        self._finished = None
        return self

    __iadd__ = merge

    def host_sums(self):
        """`sums` as a numpy array.  For device sums this download of a few kilobytes is the one synchronisation of `best`."""
        return self.sums.cpu().numpy() if self.on_device else np.asarray(self.sums)

    def best(self, criterion="vt", min_coverage=0.9, rotation=None):
        """The `CentreFix` of the best eligible candidate.  A candidate is eligible iff it holds a pixel and its count is at
        least `min_coverage` times the largest count of the lattice: a candidate whose annulus leaves the scene (or the keep
        mask) is not compared with whole ones.  criterion: "vt" maximises rotation * vt, `rotation` +1 (counter-clockwise) or
        -1, None meaning the sign of the first guess's latitude: cyclonic; "wspd" maximises the annulus-mean speed; "calm"
        minimises it (for `annulus=(0, r_eye)`); "steady" minimises wspd_std.  A candidate whose score is NaN is not eligible;
        ties go to the smallest flat index i * n + j.  NaN with i = j = -1 where nothing is eligible.  Works on the host; for
        device sums the download of `sums` is its only synchronisation."""
        if criterion not in CRITERIA:
            raise ValueError(f"criterion must be one of {CRITERIA}, not {criterion!r}")
        min_coverage = float(min_coverage)
        if not 0.0 <= min_coverage <= 1.0:
            raise ValueError(f"min_coverage must lie in [0, 1], not {min_coverage}")
        if rotation is None:
            rotation = 1.0 if self.spec.lat_g >= 0.0 else -1.0
        elif rotation not in (1, -1):
            raise ValueError(f"rotation must be +1, -1 or None, not {rotation!r}")
        s = self.host_sums()
        f = _finish_host(*s)
        if criterion == "vt":
            score = float(rotation) * f["vt"]
            rank = score
        elif criterion == "wspd":
            score = f["wspd"]
            rank = score
        else:
            score = f["wspd"] if criterion == "calm" else f["wspd_std"]
            rank = -score
        n = s[0]
        eligible = (n > 0) & (n.astype(np.float64) >= min_coverage * float(n.max())) & ~np.isnan(score)
        if not eligible.any():
            nan = float("nan")
            return CentreFix(nan, nan, nan, nan, -1, -1, nan, False)
        flat = int(np.argmax(np.where(eligible, rank, -np.inf)))   # the first of equal values
        i, j = divmod(flat, self.spec.n)
        lon, lat = self.spec._lonlat()
        last = self.spec.n - 1
        return CentreFix(float(lon[i, j]), float(lat[i, j]), float(self.spec.x_km[j]), float(self.spec.y_km[i]), i, j, float(score[i, j]),
                         bool(i in (0, last) or j in (0, last)))


def _centre_path():
    v = os.environ.get("XSW_CENTRE_PATH")
    if v is not None and v != "direct":
        raise ValueError(f"XSW_CENTRE_PATH must be direct, or unset, not {v!r}")


def _wind_centre(src, kind, what, tie_points, first_guess, step_km, n, annulus, line, sample, keep, into, lut=None):
    # every host check
    keep = _keep(keep, src, what)
    if not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    L, S = (int(v) for v in src.shape)
    line, sample = _pixel_axis(line, L, tie_points.line, "line"), _pixel_axis(sample, S, tie_points.sample, "sample")
    spec = CentreSpec(first_guess, step_km, n, annulus)
    _centre_path()
    if into is not None:
        if not isinstance(into, CentreScores):
            raise TypeError(f"into must be a CentreScores, not {type(into).__name__}")
        if into.spec != spec:
            raise ValueError(f"into lies on {into.spec}, the call asks for {spec}")
        if into.on_device != _is_tensor(src):
            raise ValueError(f"into holds {'device' if into.on_device else 'host'} sums but {what} is a {'device' if _is_tensor(src) else 'host'} array: "
                             "one container kind per call")
    lf, lt = bracket(tie_points.line, line)
    sf, st = bracket(tie_points.sample, sample)
    cos_g, sin_g = spec.tables()

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
        out = CentreScores(sums, spec)
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
        args = (L, S, call.mem, kind, src, keep, len(tie_points.line), len(tie_points.sample), *tables, spec.lon_g, spec.lat_g, cos_g, sin_g,
                spec.step_km, spec.n, spec.r_in_km, spec.r_out_km, sums)
        if lut is None:
            call.launch("wind_centre_raw", *args)
        else:  # codes: the context must hold their LUT when the kernel reads `sol`
            from .windspeed import _engine
            is_array = lambda a: hasattr(a, "data_ptr") or isinstance(a, np.ndarray)

            def run(ctx, mem):
                with ctx.lock:
                    _engine.ensure_luts(ctx, lut, None)
                    ctx.wind_centre_raw(*[call.ptr(a) if is_array(a) else a for a in args])
            call.run(run, [a for a in args if is_array(a)])
        out._finished = None
    return out


def wind_centre_scores(wind, tie_points, *, first_guess, step_km, n, annulus, line=None, sample=None, keep=None, into=None):
    """`CentreScores` of a complex wind raster on the `n x n` lattice of candidates, `step_km` apart, around first_guess =
    (lon, lat), for the annulus = (r_in_km, r_out_km) around each candidate.

    wind: complex128 or complex64 `[L, S]`, antenna convention, numpy or a device tensor.  tie_points: the scene's `TiePoints`
    (required: every pixel is geolocated).  line / sample: the raster's coordinate vectors (default np.arange; a row tile passes
    its own lines); every coordinate lies inside the tie points' span.  The first guess (a best track, the scene's middle) may
    lie outside the raster.  A pixel counts for a candidate iff its distance from it on the chart lies in [r_in_km, r_out_km),
    neither part is NaN, its keep byte (bool / uint8 `[L, S]` in the raster's container kind) is non-zero, its heading is
    defined and its speed is below 256 m/s.

    into: a `CentreScores` of the same `CentreSpec` and container kind, which the call accumulates into (and returns): a scene
    in row tiles.  Any order gives the same bits.  Without it the sums start at zero.

    ValueError / TypeError for a wrong rank, dtype or container kind, a `keep` of another shape, `tie_points` that is not a
    `TiePoints`, coordinates outside the tie span, a first guess that is not two finite numbers or lies beyond 89 degrees of
    latitude, an `n` that is even or outside 1 .. 31, step_km <= 0 (for n > 1), an annulus that is not 0 <= r_in_km < r_out_km,
    an `into` of another spec, an XSW_CENTRE_PATH other than `direct` -- all before any device call."""
    src, name = _source(wind, "wind", ("complex128", "complex64"))
    return _wind_centre(src, _lib.CELLS_C128 if name == "complex128" else _lib.CELLS_C64, "wind", tie_points, first_guess, step_km, n, annulus, line,
                        sample, keep, into)


def codes_centre_scores(codes, lut_co, tie_points, *, first_guess, step_km, n, annulus, line=None, sample=None, keep=None, into=None):
    """`wind_centre_scores` from co-pol grid codes `[L, S]` (uint32 numpy, or an int32 / uint32 device tensor) of the LUT `lut_co`
    (`CopolCodes.centre_scores` calls this): 4 B per pixel are read and nothing is expanded; bit for bit `wind_centre_scores` of
    the complex128 expansion."""
    src, _ = _source(codes, "codes", ("uint32", "int32"))
    if not _is_tensor(src):
        src = src.view(np.uint32)
    return _wind_centre(src, _lib.CELLS_CODES, "codes", tie_points, first_guess, step_km, n, annulus, line, sample, keep, into, lut=lut_co)


def _find(scores, tie_points, first_guess, steps_km, n, criterion, min_coverage, rotation):
    """`find_centre` behind both sources: `scores(first_guess=, step_km=, n=)` is the scoring call."""
    if not isinstance(tie_points, TiePoints):
        raise TypeError("tie_points must be a TiePoints")
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}, not {criterion!r}")
    try:
        steps = [float(s) for s in steps_km]
    except TypeError:
        raise TypeError(f"steps_km must be a sequence of numbers, not {steps_km!r}") from None
    if not steps or not all(math.isfinite(s) and s > 0.0 for s in steps):
        raise ValueError(f"steps_km must hold one finite positive step or more, not {steps_km!r}")
    if first_guess is None:  # the middle of the tie points (their longitudes are continuous already)
        first_guess = (float(np.mean(tie_points.longitude)), float(np.mean(tie_points.latitude)))
    levels, fix = [], None
    for step in steps:
        level = scores(first_guess=first_guess, step_km=step, n=n).best(criterion, min_coverage, rotation)
        levels.append(level)
        if not level.found:
            break
        fix, first_guess = level, (level.lon, level.lat)
    fix = fix if fix is not None else levels[-1]
    return CentreFix(fix.lon, fix.lat, fix.x_km, fix.y_km, fix.i, fix.j, fix.score, fix.on_border, levels)


def find_centre(wind, tie_points, *, first_guess=None, steps_km=(8.0, 2.0, 0.5), n=9, annulus, criterion="vt", keep=None, line=None, sample=None,
                min_coverage=0.9, rotation=None):
    """The centre of the cyclone in a complex wind raster, coarse to fine: `wind_centre_scores(...).best(criterion, min_coverage,
    rotation)` on an `n x n` lattice for every step of `steps_km` in turn, each lattice laid around the best node of the one
    before, the first around `first_guess = (lon, lat)` (None: the mean longitude and latitude of the tie points).  Returns the
    last level's `CentreFix`, with the fixes of all levels in `.levels`; `x_km`, `y_km`, `i`, `j` are those of its own lattice.
    If a level has nothing eligible the search stops with the fix of the level before (with that level's own NaN fix if it was
    the first).  Arguments and refusals otherwise as `wind_centre_scores` and `CentreScores.best`."""
    return _find(lambda **k: wind_centre_scores(wind, tie_points, annulus=annulus, keep=keep, line=line, sample=sample, **k), tie_points, first_guess,
                 steps_km, n, criterion, min_coverage, rotation)


def codes_find_centre(codes, lut_co, tie_points, *, first_guess=None, steps_km=(8.0, 2.0, 0.5), n=9, annulus, criterion="vt", keep=None, line=None,
                      sample=None, min_coverage=0.9, rotation=None):
    """`find_centre` from co-pol grid codes (`CopolCodes.find_centre` calls this): nothing is expanded."""
    return _find(lambda **k: codes_centre_scores(codes, lut_co, tie_points, annulus=annulus, keep=keep, line=line, sample=sample, **k), tie_points,
                 first_guess, steps_km, n, criterion, min_coverage, rotation)
