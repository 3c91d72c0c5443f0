"""The hand-built histograms at which the GPU tests hold k_streaks_peak (csrc/xsw_streaks.hip) to the BIT, and the two designed
fields of the raster pass: tests/test_gpu_streaks_exact.py runs them on the device, tests/test_streaks_cpu.py runs every builder
so that the assertions below are exercised without one.  Each case carries the restatement's result (tests/streaks_ref.py),
computed once and read-only; a builder asserts, on the restatement alone, the property its case exists for.  Numpy only.

Why bits can be expected.  The kernel's header states its sums as float64 in a fixed order, free of contractions, and the
restatement adds in that order: the mean over the leading axes in axis order with one division, every smoothing pass from 0 over
all its taps in ascending order, the zero taps included.  No operation of the peak kernel is a library call.

What each family can catch (lane l of the window's wave owns the bins l, l + 64, ...; the arg-max is a scan of a lane's own bins
followed by a 64-lane butterfly on (value, index)):
  periodic   a histogram of period p | n has bit-identical smoothed values at a, a + p, ...: an exact tie of n / p bins.
             n = 360, p = 60, class 10: bins 10, 70, 130, 190, 250, 310 in lanes 10, 6, 2, 62, 58, 54.  The answer is 10, while
             lower lanes hold larger indices: a butterfly that preferred the lower lane, or that dropped `oi < bi`, answers 130
             (lane 2 is the lowest lane that holds a tied bin).  n = 128, p = 64: bins 5 and 69 in ONE lane: a scan with `>=`
             answers 69.  n = 512, p = 64: the eight strides of lane 63.  n = 130, p = 65: bins 64 and 129, lanes 0 and 1 in their
             second and third stride.  n = 72, p = 6: a twelve-way tie
  lanes      the unique maximum at bin 0, n - 1, 63, 64 and the last bin of the last full stride, for n_angles on both sides of
             every multiple of 64 the kernel can meet: a lane that scans one stride too few or too many, a butterfly that loses a
             lane.  With 8 bins the smoothed histogram is flat and rounding decides: the restatement's two largest values either
             differ in bits or are bit-equal, and both kinds decide the index exactly
  counts     1, 3, 4, 5 and 9 windows: a workgroup of four waves whose idle waves recompute the last window, exactly one full
             workgroup, one window past it; every window with a different peak
  values     negative means, an all-NaN bin among them (it wins as 0, weight NaN), signed zeros, +inf under the zero taps, NaN
             in 1, 2 and all of the configurations, NaN in used_ratio"""
import functools
from collections import namedtuple

import numpy as np

import gradients_ref as ref
import streaks_ref as sref

Case = namedtuple("Case", "name weight ratio n smooth want claim")   # weight [C, nl, ns, n], ratio [C, nl, ns]; want: sref.streaks_direction

PERIODIC = ((360, 60, 10), (128, 64, 5), (512, 64, 63), (130, 65, 64), (72, 6, 5))   # (n_angles, period, class of the peak)
LANE_ANGLES = (8, 12, 63, 64, 65, 127, 128, 129, 360, 511, 512)
WINDOW_COUNTS = ((1, 1), (1, 3), (2, 2), (5, 1), (3, 3))                               # nl x ns = 1, 3, 4, 5, 9
HEIGHTS = (5.0, 50.0, 500.0)


def _rng(name):
    return np.random.default_rng(list(name.encode()))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def filled(m):
    """What the arg-max compares: NaN counts as 0."""
    return np.where(np.isnan(m), 0.0, m)


def top_two(m):
    """The two largest compared values of every window, largest first."""
    f = np.sort(filled(m), axis=-1)
    return f[..., -1], f[..., -2]


def _case(name, weight, ratio, smooth, **claim):
    weight, ratio = np.ascontiguousarray(weight, dtype=np.float64), np.ascontiguousarray(ratio, dtype=np.float64)
    assert weight.ndim == 4 and ratio.shape == weight.shape[:3], name
    n = weight.shape[-1]
    with np.errstate(invalid="ignore"):   # 0 * inf under the zero taps
        want = sref.streaks_direction(weight, ratio, ref.angles_bins(n), smooth=smooth)
    for a in (weight, ratio, *want.values()):
        a.setflags(write=False)
    # the first maximum, restated once more without numpy's argmax
    f = filled(want["m"])
    first = np.array([[int(np.flatnonzero(row == row.max())[0]) for row in plane] for plane in f])
    np.testing.assert_array_equal(want["index"], first, err_msg=name)
    return Case(name, weight, ratio, n, smooth, want, claim)


def _ratio(rng, shape):
    return rng.uniform(0.1, 1.0, shape)


# ------------------------------------------------------------------------------------------------------------- periodic ties
def periodic_case(n, p, peak, smooth, C):
    """Two windows [C, 1, 2, n] of period p with the largest value in class `peak`: every configuration is periodic, so the mean
    and every smoothing pass do the same operations on the same values at a, a + p, a + 2p, ..."""
    name = f"periodic_n{n}_p{p}_{'smooth' if smooth else 'raw'}_C{C}"
    rng = _rng(name)
    assert n % p == 0 and 0 <= peak < p
    W = np.empty((C, 1, 2, n))
    for w in range(2):
        for c in range(C):
            pattern = rng.uniform(0.0, 0.5, p)
            pattern[peak] = 2.0 + 0.37 * c + 0.11 * w
            W[c, 0, w] = np.tile(pattern, n // p)
    case = _case(name, W, _ratio(rng, (C, 1, 2)), smooth, tied=tuple(range(peak, n, p)), period=p)
    tied = np.array(case.claim["tied"])
    for w in range(2):
        m = case.want["m"][0, w]
        assert len(set(bits(m[tied]).tolist())) == 1, name                # equal as bit patterns
        others = np.delete(m, tied)
        assert (others < m[peak]).all(), name                             # and the maximum, nothing else reaching it
        assert case.want["index"][0, w] == peak == tied.min(), name      # the smallest of them
    if n == 360:   # lower lanes hold larger indices: neither the lower lane nor the last stride may win
        assert any(b > peak and b % 64 < peak % 64 for b in tied), name
        assert min(tied, key=lambda b: b % 64) == 130
    if (n, p) == (128, 64):
        assert {int(b) % 64 for b in tied} == {peak}                      # one lane, two strides
    return case


# ------------------------------------------------------------------------------------------------------------ lane ownership
def lane_positions(n):
    pos = {0, n - 1}
    pos.update(b for b in (63, 64) if b < n)
    if n >= 64:
        pos.add(n // 64 * 64 - 1)   # the last bin of the last full stride
    return tuple(sorted(pos))


def lane_case(n, smooth):
    """One window per position of the unique maximum, [2, 1, positions, n].  With smoothing the peak must stay unique on the
    restatement (the height is raised until it does); with 8 bins it cannot (the passes average every bin), so that case holds
    windows of both decided kinds instead: top two values different in bits, and bit-equal."""
    name = f"lanes_n{n}_{'smooth' if smooth else 'raw'}"
    rng = _rng(name)
    pos = lane_positions(n)
    if n == 8 and smooth:
        W = rng.uniform(0.0, 1.0, (2, 1, 24, n))
        W[:, 0, 0] = np.array([1, 2, 3, 4, 5, 6, 7, 8.0]) / 16       # dyadic: every sum exact, all eight bins bit-equal
        W[:, 0, 1] = np.array([8, 1, 1, 1, 1, 1, 1, 1.0]) / 32
        case = _case(name, W, _ratio(rng, W.shape[:3]), smooth, positions=None)
        hi, lo = top_two(case.want["m"])
        equal = bits(hi) == bits(lo)
        assert equal.any() and (~equal).any(), name                    # both kinds occur
        assert sref.near_tie(case.want["m"]).all(), name               # (and every one of them was excused before)
        assert equal[0, 0] and case.want["index"][0, 0] == 0
        return case
    for height in HEIGHTS:
        W = rng.uniform(0.0, 1.0, (2, 1, len(pos), n))
        for k, b in enumerate(pos):
            W[:, 0, k, b] = height
        case = _case(name, W, _ratio(rng, W.shape[:3]), smooth, positions=pos, height=height)
        if not sref.near_tie(case.want["m"]).any():
            break
    else:
        raise AssertionError(f"{name}: no height keeps the peak unique")
    np.testing.assert_array_equal(case.want["index"][0], pos, err_msg=name)
    return case


# -------------------------------------------------------------------------------------------------------------- window counts
def count_case(nl, ns, smooth, n=72, C=2):
    name = f"counts_{nl}x{ns}_n{n}_{'smooth' if smooth else 'raw'}_C{C}"
    rng = _rng(name)
    W = rng.uniform(0.0, 1.0, (C, nl, ns, n))
    peaks = (7 + 53 * np.arange(nl * ns)) % n          # all different (53 is prime to 72 and to 512)
    assert len(set(peaks.tolist())) == nl * ns
    for w, b in enumerate(peaks):
        W[:, w // ns, w % ns, b] = 50.0
    case = _case(name, W, _ratio(rng, (C, nl, ns)), smooth, peaks=tuple(int(b) for b in peaks))
    np.testing.assert_array_equal(case.want["index"].ravel(), peaks, err_msg=name)
    assert not sref.near_tie(case.want["m"]).any(), name
    return case


# --------------------------------------------------------------------------------------------------------------------- values
TINY = 5e-324


def value_cases():
    out = []
    for smooth in (False, True):
        tag = "smooth" if smooth else "raw"
        # negative means only
        rng = _rng("negative" + tag)
        W = -rng.uniform(0.1, 1.0, (2, 1, 3, 72))
        c = _case(f"values_negative_{tag}", W, _ratio(rng, (2, 1, 3)), smooth)
        assert (c.want["m"] < 0).all() and (c.want["weight"] < 0).all() and not sref.near_tie(c.want["m"]).any()
        out.append(c)
        # negative means and one all-NaN bin: NaN counts as 0 and wins; the stored weight is the NaN itself
        W = -rng.uniform(0.1, 1.0, (2, 1, 3, 72))
        W[:, 0, :, 17] = np.nan
        W[:, 0, 2, 71] = np.nan                         # a second one in the last window: the reach wraps to bin 0
        c = _case(f"values_negative_nan_bin_{tag}", W, _ratio(rng, (2, 1, 3)), smooth)
        nan_bins = [np.flatnonzero(np.isnan(c.want["m"][0, w])) for w in range(3)]
        assert [int(b[0]) for b in nan_bins] == c.want["index"][0].tolist() and np.isnan(c.want["weight"]).all()
        assert c.want["index"][0].tolist() == ([2, 2, 0] if smooth else [17, 17, 17])   # the cumulative reach is 15 bins
        out.append(c)
        # +inf in one bin: 0 * inf under the zero taps is NaN, which counts as 0
        for C in (1, 2):
            W = rng.uniform(0.0, 1.0, (C, 1, 2, 72))
            W[0, 0, 0, 40] = np.inf
            W[C - 1, 0, 1, 3] = np.inf
            c = _case(f"values_inf_{tag}_C{C}", W, _ratio(rng, (C, 1, 2)), smooth)
            m = c.want["m"]
            if smooth:   # Bx keeps +inf at 39 .. 41; the zero taps of the later passes turn what they touch into NaN, while their
                # outer taps carry +inf on, beyond the NaN: bins 26 .. 54 are NaN, 25 and 55 +inf, and the peak is the first of these
                for w, b in ((0, 40), (1, 3)):
                    nan, inf = np.flatnonzero(np.isnan(m[0, w])), np.flatnonzero(np.isinf(m[0, w]))
                    assert sorted(nan.tolist()) == sorted((b + k) % 72 for k in range(-14, 15)), c.name
                    assert sorted(inf.tolist()) == sorted(((b - 15) % 72, (b + 15) % 72)) and c.want["index"][0, w] == inf.min(), c.name
                assert c.want["index"][0].tolist() == [25, 18] and np.isinf(c.want["weight"]).all()
            else:
                assert c.want["index"][0].tolist() == [40, 3] and np.isinf(c.want["weight"]).all()
            out.append(c)
        # a bin that is NaN in 1, 2 and all 3 configurations
        W = rng.uniform(0.0, 1.0, (3, 1, 2, 72))
        W[1, 0, :, 5] = np.nan
        W[0, 0, :, 20] = W[2, 0, :, 20] = np.nan
        W[:, 0, :, 40] = np.nan
        W[1, 0, 1, 5] = np.nan
        W[:, 0, 1, 20] = [np.nan, 30.0, np.nan]         # the single finite term of this bin is the window's peak
        c = _case(f"values_nan_counts_{tag}", W, _ratio(rng, (3, 1, 2)), smooth)
        m0 = sref.nanmean_leading(W, 3)
        assert m0[0, 0, 5] == (W[0, 0, 0, 5] + W[2, 0, 0, 5]) / 2 and m0[0, 0, 20] == W[1, 0, 0, 20] and np.isnan(m0[0, 0, 40])
        if not smooth:
            assert c.want["index"][0, 1] == 20 and c.want["weight"][0, 1] == 30.0
        out.append(c)
    # signed zeros among negatives, without smoothing (a pass starts from +0 and cannot give -0).  The mean starts from +0 too,
    # so a -0.0 given in every configuration is averaged to +0.0 (window 0: bin 3 is -0.0, bin 9 is +0.0, both compare equal,
    # the index is 3 and the stored weight is +0.0); a mean of -0.0 comes from a sum that rounds to it: (-5e-324 + 0 + 0) / 3
    # (window 1: the index is 3 and the stored weight keeps its sign bit)
    rng = _rng("zeros")
    W = -rng.uniform(0.1, 1.0, (3, 1, 2, 72))
    W[:, 0, 0, 3], W[:, 0, 0, 9] = -0.0, 0.0
    W[:, 0, 1, 3], W[:, 0, 1, 9] = [-TINY, 0.0, 0.0], 0.0
    c = _case("values_signed_zeros_raw", W, _ratio(rng, (3, 1, 2)), False)
    assert c.want["index"][0].tolist() == [3, 3] and (c.want["weight"] == 0).all()
    assert np.signbit(c.want["weight"][0]).tolist() == [False, True]
    assert not np.signbit(c.want["m"][0, :, 9]).any()
    out.append(c)
    # used_ratio with NaN in some and in all configurations
    W = rng.uniform(0.0, 1.0, (3, 1, 4, 72))
    R = rng.uniform(0.1, 1.0, (3, 1, 4))
    R[1, 0, 0] = np.nan
    R[0, 0, 1] = R[2, 0, 1] = np.nan
    R[:, 0, 2] = np.nan
    c = _case("values_ratio_nan", W, R, True)
    u = c.want["used_ratio"][0]
    assert u[0] == (R[0, 0, 0] + R[2, 0, 0]) / 2 and u[1] == R[1, 0, 1] and np.isnan(u[2])
    assert u[3] == (R[0, 0, 3] + R[1, 0, 3] + R[2, 0, 3]) / 3
    out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------ all cases
@functools.lru_cache(maxsize=None)
def periodic_cases():
    return tuple(periodic_case(n, p, peak, smooth, C) for n, p, peak in PERIODIC for smooth in (True, False) for C in (1, 3))


@functools.lru_cache(maxsize=None)
def lane_cases():
    return tuple(lane_case(n, smooth) for n in LANE_ANGLES for smooth in (True, False))


@functools.lru_cache(maxsize=None)
def count_cases():
    """The largest input of the module is the last: 512 bins, 9 windows, C = 3."""
    return tuple(count_case(nl, ns, smooth) for nl, ns in WINDOW_COUNTS for smooth in (True, False)) + \
        tuple(count_case(3, 3, smooth, n=512, C=3) for smooth in (True, False))


BUILDERS = {"periodic": periodic_cases, "lanes": lane_cases, "counts": count_cases, "values": functools.lru_cache(maxsize=None)(lambda: tuple(value_cases()))}


@functools.lru_cache(maxsize=None)
def cases():
    out = {c.name: c for build in BUILDERS.values() for c in build()}
    assert len(out) == sum(len(build()) for build in BUILDERS.values())
    return out


def names():
    """Case names without building anything but the names' own inputs (for pytest's collection)."""
    return sorted(cases())


# ------------------------------------------------------------------------------------------------------ the raster pass's fields
Field = namedtuple("Field", "name dirs windows_line windows_sample anc line sample claim")
FIELD_SHAPE = (203, 301)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def small_components_field():
    """Resolved directions within 1e-8 rad of the axes: one component of v is about 1e-8 of the other, with every combination
    of signs.  The directions keep one axis and one sign over large patches of windows (as a resolved field does: opposite
    neighbours would cancel), the small angle changes sign and size from window to window."""
    rng = _rng("small components")
    L, S = FIELD_SHAPE
    wl, ws = np.arange(8) * 29.0 + 3, np.arange(11) * 31.0 - 7     # the last centres inside the raster on lines, outside on samples
    base = np.zeros((8, 11))
    base[:4, 6:], base[4:, :6], base[4:, 6:] = np.pi / 2, np.pi, -np.pi / 2
    eps = rng.uniform(0.05, 1.0, base.shape) * 1e-8 * rng.choice([-1.0, 1.0], base.shape)
    dirs = np.exp(1j * (base + eps))
    dirs[2, 3] = dirs[6, 8] = complex(np.nan, np.nan)
    anc = rng.normal(0, 6, FIELD_SHAPE) + 1j * rng.normal(0, 6, FIELD_SHAPE)
    anc[rng.random(FIELD_SHAPE) < 0.01] = complex(np.nan, np.nan)
    anc[rng.random(FIELD_SHAPE) < 0.01] = 0
    line, sample = np.arange(float(L)), np.arange(float(S))
    want = sref.ancillary(dirs, wl, ws, anc, line, sample)
    ex = sref.ancillary_exact(dirs, wl, ws, anc, line, sample)
    blend = ex["blend"]
    mag = np.hypot(anc.real, anc.imag)
    small = blend & (np.minimum(np.abs(want.real), np.abs(want.imag)) < 1e-6 * mag)
    assert blend.sum() > 0.9 * blend.size and small.sum() * 4 > blend.sum(), (int(small.sum()), int(blend.sum()))
    signs = {(bool(a), bool(b)) for a, b in zip(np.signbit(want.real[small]), np.signbit(want.imag[small]))}
    assert len(signs) == 4                                           # signs mixed
    _frozen(dirs, wl, ws, anc, line, sample)
    return Field("small_components", dirs, wl, ws, anc, line, sample, dict(small=int(small.sum()), blend=int(blend.sum())))


AXES = (complex(1.0, 0.0), complex(-1.0, -0.0), complex(0.0, 1.0), complex(-0.0, -1.0))   # 1, -1 as k_streaks_resolve's negation stores it, 1j, -1j


@functools.lru_cache(maxsize=None)
def closed_form_field():
    """Every window is 1, -1, 1j or -1j, in patches of 2 x 2 and larger; a lies on an axis with |a| = 7 * 2**k; the centres are 32
    apart, so every blend weight is a multiple of 1 / 32 and every product and sum of the blend is exact.  `claim`: the mask of
    the pixels whose four corners are bit-equal, and the output expected there: |a| times the corners' axis, the other part +0.0."""
    rng = _rng("closed form")
    L, S = FIELD_SHAPE
    wl, ws = np.arange(7) * 32.0, np.arange(10) * 32.0              # the last centres at 192 and 288: clamped pixels past them
    patch = rng.integers(0, 4, (4, 5))
    patch[0, :4] = [0, 1, 2, 3]                                       # each of the four at least once
    which = np.repeat(np.repeat(patch, 2, axis=0), 2, axis=1)[:7, :10]
    dirs = np.array(AXES)[which]
    assert np.signbit(dirs[which == 1].imag).all() and np.signbit(dirs[which == 3].real).all()
    k = rng.integers(-20, 21, FIELD_SHAPE)
    mag = 7.0 * np.exp2(k)
    axis = rng.integers(0, 4, FIELD_SHAPE)
    anc = np.empty(FIELD_SHAPE, dtype=np.complex128)   # filled part by part to keep the signs of zero
    anc.real = np.where(axis == 0, mag, np.where(axis == 1, -mag, np.where(axis == 3, -0.0, 0.0)))
    anc.imag = np.where(axis == 2, mag, np.where(axis == 3, -mag, np.where(axis == 1, -0.0, 0.0)))
    line, sample = np.arange(float(L)), np.arange(float(S))
    i0, i1, _ = sref.bracket(wl, line)
    j0, j1, _ = sref.bracket(ws, sample)
    corners = [which[np.ix_(i, j)] for i in (i0, i1) for j in (j0, j1)]
    equal = (corners[0] == corners[1]) & (corners[0] == corners[2]) & (corners[0] == corners[3])
    assert equal.sum() > 0.3 * equal.size and (~equal).sum() > 0.3 * equal.size
    d = dirs[np.ix_(i0, j0)]
    expected = np.zeros(FIELD_SHAPE, dtype=np.complex128)
    expected.real = np.where(d.real != 0, mag * d.real, 0.0)          # exact: +-1 times 7 * 2**k
    expected.imag = np.where(d.imag != 0, mag * d.imag, 0.0)
    assert not np.signbit(expected.real[d.real == 0]).any() and not np.signbit(expected.imag[d.imag == 0]).any()
    _frozen(dirs, wl, ws, anc, line, sample, equal, expected)
    return Field("closed_form", dirs, wl, ws, anc, line, sample, dict(equal=equal, expected=expected))


FIELDS = {"small_components": small_components_field, "closed_form": closed_form_field}
