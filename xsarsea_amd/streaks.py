"""From direction histograms to the inversion's a-priori wind: the link between `gradients` and `windspeed`.

    Gradients(sigma0).histogram -> streaks_direction -> Streaks.resolve(ancillary_wind) -> ancillary_from_streaks -> invert_from_model

`streaks_direction` is what the reference's notebook docs/examples/streaks.ipynb does by hand with the histograms: mean over
pol / downscale_factor / window_size, `circ_smooth`, peak bin, rotated by pi/2 (streaks lie across the gradient): one direction
modulo pi per window.  `Streaks.resolve` removes the 180 degree ambiguity with the model wind, and `ancillary_from_streaks` spreads
the resolved directions over the raster (bilinear between window centres) with the model's speed: the `ancillary_wind` of a co-pol
inversion.  The per-window reduction and the full-raster pass run in HIP kernels (csrc/xsw_streaks.hip, include/xsw.h:
xsw_streaks_*); brackets and nearest pixels are host arithmetic on the coordinate vectors.

Containers as in `gradients`: numpy in gives numpy out (through host buffers); a device tensor in gives device tensors out, computed
asynchronously on the caller's current stream.  Complex winds follow the antenna convention (real = sample axis, imag = line axis);
angles are radians from the sample axis towards the line axis.
"""
import numpy as np

from ._raster import _Call, _coord_values, _is_tensor, _Raster, _small, _unwrap
from .gradients import GradientsHistogram, nearest_indexer

__all__ = ["Streaks", "streaks_direction", "ancillary_from_streaks", "bracket"]


def bracket(centres, coords):
    """Bracket of every coordinate between neighbouring window centres (ascending): (first, t), the index of the bracket's first
    centre (int32) and the weight t of the next one (float64, one IEEE division; the first one weighs 1 - t).  Outside the first /
    last centre, and for a single centre, the edge centre weighs 1: t = 0."""
    c, x = np.asarray(centres, dtype=np.float64), np.asarray(coords, dtype=np.float64)
    if c.ndim != 1 or len(c) < 1:
        raise ValueError("window centres must be a non-empty vector")
    if len(c) > 1 and not (np.diff(c) > 0).all():
        raise ValueError("window centres must be strictly ascending")
    first = np.clip(np.searchsorted(c, x, side="right") - 1, 0, len(c) - 1)
    nxt = np.minimum(first + 1, len(c) - 1)
    inside = (x > c[0]) & (first < len(c) - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(inside, (x - c[first]) / np.where(inside, c[nxt] - c[first], 1.0), 0.0)
    return first.astype(np.int32), t


class Streaks:
    """Result of `streaks_direction`: angle (float64, modulo pi), weight (the histogram's value at the peak), used_ratio
    [line, sample], index (int32, the peak bin), line / sample (window centres) and angles (the direction of every bin:
    angle = angles[index]).  Attribute or item access."""

    def __init__(self, angle, weight, used_ratio, index, line, sample, angles=None):
        self.angle, self.weight, self.used_ratio, self.index, self.line, self.sample, self.angles = angle, weight, used_ratio, index, line, sample, angles

    def __getitem__(self, name):
        return getattr(self, name)

    def _unit(self, call):
        """exp(1j * angle) of every window: through the table of the bins' unit vectors where the peak bins are known."""
        if self.index is not None and self.angles is not None:
            table = np.exp(1j * np.asarray(self.angles, dtype=np.float64))
            if call.device:
                return _small(call, table, np.complex128)[call.prep(self.index, np.int32).long()]
            return table[np.asarray(self.index)]
        if call.device:
            a = call.prep(self.angle, np.float64)
            return call.torch.polar(call.torch.ones_like(a), a)
        return np.exp(1j * np.asarray(self.angle, dtype=np.float64))

    def resolve(self, ancillary_wind, line=None, sample=None, min_weight=None, min_used_ratio=None):
        """Unit vectors exp(1j * angle) [line, sample] (complex128) with the 180 degree ambiguity removed against the a-priori
        wind: negated where Re(d * conj(a)) < 0 (a zero dot product keeps d).  `ancillary_wind` is the full complex raster (with
        its `line` / `sample` coordinates, default np.arange), from which each window takes the pixel nearest its centre (ties
        to the larger coordinate), or an array of the windows' own shape.  NaN + NaN j where angle / weight is NaN, where `a` has
        a NaN part or is 0, and where weight < min_weight or used_ratio < min_used_ratio when these are given."""
        call = _Call(self.angle, self.weight, self.used_ratio, ancillary_wind)
        shape = tuple(self.weight.shape)
        anc = _unwrap(ancillary_wind)
        if tuple(anc.shape) != shape:
            r = _Raster(ancillary_wind, line, sample)
            rows, cols = nearest_indexer(r.line, _coord_values(self.line)), nearest_indexer(r.sample, _coord_values(self.sample))
            if call.device:
                full = call.prep(r.values, np.complex128) if not _is_tensor(r.values) else r.values
                anc = full[_small(call, rows, np.int64)][:, _small(call, cols, np.int64)]
            else:
                anc = np.asarray(r.values)[np.ix_(rows, cols)]
        d0, anc = call.prep(self._unit(call), np.complex128), call.prep(anc, np.complex128)
        weight, ratio = call.prep(self.weight, np.float64), call.prep(self.used_ratio, np.float64)
        out = call.empty(shape, np.complex128)
        nw = int(np.prod(shape))
        lo_w = np.nan if min_weight is None else float(min_weight)
        lo_r = np.nan if min_used_ratio is None else float(min_used_ratio)
        if nw:
            call.launch("streaks_resolve_raw", nw, call.mem, d0, weight, ratio, anc, lo_w, lo_r, out)
        return out


def streaks_direction(hist, smooth=True, orthogonal=True, angles=None, line=None, sample=None):
    """One streak direction per window from direction histograms (the notebook's steps, fused in one kernel).

    hist: a `gradients.GradientsHistogram` (from `Gradients` or `Gradients2D`), or a bare weight array [..., line, sample, angles]
    with the bin centres `angles=` (then used_ratio is NaN, and `line=` / `sample=` name the window centres, default np.arange).
    Per window: the NaN-skipping mean of the histograms over every leading axis, `circ_smooth` (with `smooth`), the first
    arg-max with NaN counted as 0; angle = angles[index] + pi/2 with `orthogonal` (streaks lie across the gradient), weight = the
    smoothed mean at the peak (NaN stays NaN), used_ratio = NaN-skipping mean over the same axes."""
    if isinstance(hist, GradientsHistogram):
        weight, ratio, angles, line, sample = hist.weight, hist.used_ratio, hist.angles, hist.line, hist.sample
    else:
        weight, ratio = _unwrap(hist), None
        if angles is None:
            raise ValueError("a bare weight array needs the bin centres: angles=")
    angles = np.asarray(angles, dtype=np.float64)
    if len(weight.shape) < 3 or weight.shape[-1] != len(angles):
        raise ValueError(f"weight must be [..., line, sample, angles] with {len(angles)} angles, not {tuple(weight.shape)}")
    nl, ns, n = (int(v) for v in weight.shape[-3:])
    call = _Call(weight)
    w = call.prep(weight, np.float64).reshape((-1, nl, ns, n))
    if ratio is None:
        ratio = call.torch.full(tuple(w.shape[:3]), float("nan"), dtype=call.torch.float64, device=call.dev) if call.device else \
            np.full(w.shape[:3], np.nan)
    r = call.prep(ratio, np.float64).reshape((-1, nl, ns))
    if r.shape[0] != w.shape[0]:
        raise ValueError("used_ratio must have weight's shape without the angles axis")
    table = angles + np.pi / 2 if orthogonal else angles
    index, wout, rout = call.empty((nl, ns), np.int32), call.empty((nl, ns), np.float64), call.empty((nl, ns), np.float64)
    if nl * ns:
        call.launch("streaks_peak_raw", w.shape[0], nl * ns, n, call.mem, smooth, w, r, index, wout, rout)
    angle = _small(call, table, np.float64)[index.long()] if call.device else table[index]
    line = np.arange(nl) if line is None else _coord_values(line)
    sample = np.arange(ns) if sample is None else _coord_values(sample)
    return Streaks(angle, wout, rout, index, line, sample, table)


def ancillary_from_streaks(streaks_or_dirs, ancillary_wind, line=None, sample=None, windows_line=None, windows_sample=None, **resolve_kwargs):
    """The a-priori raster for `invert_from_model` (complex128, `ancillary_wind`'s shape): the speed |ancillary_wind| of every
    pixel with the direction of the resolved streak field, bilinearly interpolated between window centres in the raster's
    `line` / `sample` coordinates (default np.arange; outside the first / last centre the edge centre is used).

    streaks_or_dirs: a `Streaks` (resolved here against `ancillary_wind`, `resolve_kwargs` = min_weight / min_used_ratio), or
    an already resolved complex [line, sample] field with its centres `windows_line=` / `windows_sample=`.  Per pixel
    v = sum of weight * direction over the four corners (NaN corners skipped); out = |a| * v / |v|; out = a where no corner is
    valid or they cancel (the model's direction survives where the streaks say nothing); NaN + NaN j where a has a NaN part."""
    r = _Raster(ancillary_wind, line, sample)
    if isinstance(streaks_or_dirs, Streaks):
        dirs = streaks_or_dirs.resolve(r.values, r.line, r.sample, **resolve_kwargs)
        at_line, at_sample = _coord_values(streaks_or_dirs.line), _coord_values(streaks_or_dirs.sample)
    else:
        if resolve_kwargs:
            raise TypeError(f"unexpected arguments for an already resolved field: {sorted(resolve_kwargs)}")
        if windows_line is None or windows_sample is None:
            raise ValueError("a resolved direction field needs its window centres: windows_line=, windows_sample=")
        dirs = _unwrap(streaks_or_dirs)
        at_line, at_sample = _coord_values(windows_line), _coord_values(windows_sample)
    if tuple(dirs.shape) != (len(at_line), len(at_sample)):
        raise ValueError(f"directions {tuple(dirs.shape)} do not match the window centres ({len(at_line)}, {len(at_sample)})")
    lf, lt = bracket(at_line, r.line)
    sf, st = bracket(at_sample, r.sample)
    call = _Call(r.values, dirs)
    anc, dirs = call.prep(r.values, np.complex128), call.prep(dirs, np.complex128)
    L, S = (int(v) for v in anc.shape)
    lf, lt, sf, st = _small(call, lf, np.int32), _small(call, lt, np.float64), _small(call, sf, np.int32), _small(call, st, np.float64)
    out = call.empty((L, S), np.complex128)
    if L * S:
        if not len(at_line) * len(at_sample):
            raise ValueError("no window")
        call.launch("streaks_ancillary_raw", L, S, call.mem, anc, len(at_line), len(at_sample), dirs, lf, lt, sf, st, out)
    return out
