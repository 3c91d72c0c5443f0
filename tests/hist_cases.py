"""The windows at which the GPU tests hold k_grad_hist / k_grad_hist_masked (csrc/xsw_gradients.hip: hist_window) to the BIT:
tests/test_gpu_hist_exact.py runs them, tests/test_hist_cases_cpu.py keeps them what they claim to be and holds every expected
value to the restatement (tests/gradients_ref.py::gradient_histogram, numpy's own median and np.add.at).  Numpy only.

Why bits can be expected.  A kept pixel adds v = a / (a + m) * c to its bin (a = |g2|, m = the median of the kept a).  With c = 0
it adds +0.0, yet it is kept and enters the median.  For g2 = a + 0j, hypot(a, 0) is a and atan2(0, a) is 0.  A window in which
one pixel, the PROBE, has c != 0 therefore holds fl(fl(a_p / fl(a_p + m)) * c_p) in one bin and +0.0 in all others, whatever the
summation order; used_ratio is fl(kept / (wl * ws)).  `closed_form` states this (for any window with at most one lit pixel per bin).

Group A, the median (`multisets()`, placed by `group_a()`, packed into launches by `pack`).  A multiset is the kept |G2| of one window; its probes are members of it:
lo * 2**k for some k (lo = the lower middle value) and one fixed value, lit one at a time in side-by-side copies of the box.  The
CPU test asserts that replacing m by any of the eight values nearest in rank, or by either middle value, changes at least one probe
weight.  Families:
  diverge  ~1400 values; the two middle values first differ in bit t (t = the top and the bottom bit of each of the six digits of
           the radix select: 62 and 53, 52 and 42, 41 and 31, 30 and 20, 19 and 9, 8 and 0; bit 63 is the sign), garbage in the
           low 9 bits, the others 3 .. 2**22 ulps beyond the pair; and the odd twin of each, one value above the middle removed
  dup      all equal (odd, even); the ranks inside a run of 2, 3 and ~n/2 equal values; lo the last of one run and hi the first
           of the next; a two-valued set split in half and one off half
  count    1, 2, 3, 4, 511, 512, 513, 1023, 1024, 1025, 2047, 2049 distinct random values, in a window of exactly that many
           pixels and in a 45 x 47 window (2115 pixels, no multiple of 512) with holes
  range    every binade; the smallest denormal as a member and as the median; denormal lo and hi; the largest finite double as both
           middle values (m = inf); +inf in the upper half; +inf as the median
Holes of a window (pixels that are not kept) are NaN, 0.0 and -0.0 on the unmasked route, and finite positive values with keep = 0
on the masked one; c is 0.5 there, so a hole that was kept would show.

Group B, the bin sweeps (HIST_CHUNK = 72 bins per sweep): `one_per_bin`, `several_windows`, `pythagorean_window`, `random_box`.
Group C, window geometry: `geometry_raster`, `geometry_centres`, `geometry_expected`, with `rolling_box` the (wl, ws) form of gradients_ref.rolling_window."""
import functools
from collections import namedtuple

import numpy as np

N_ANGLES = 72                       # Group A: one sweep, so that a failure there is the median's
SWEEP_ANGLES = (2, 71, 72, 73, 143, 144, 145, 360)
KS = (-30, -1, 0, 1, 30)
FIXED = 1.5
C_PROBES = (0.75, 0.625, 0.875, 0.5625, 0.6875, 0.8125, 0.9375, 0.53125)   # dyadic
C_HOLE = 0.5
MAXF = np.finfo(np.float64).max
TINY = 5e-324
DIGIT_BOUNDS = (53, 42, 31, 20, 9)  # pass p covers bits below DIGIT_BOUNDS[p - 1] down to DIGIT_BOUNDS[p]
DIVERGE_BITS = (62, 53, 52, 42, 41, 31, 30, 20, 19, 9, 8, 0)
COUNTS = (1, 2, 3, 4, 511, 512, 513, 1023, 1024, 1025, 2047, 2049)
W_MAIN, W_BIG = (37, 41), (45, 47)

Multiset = namedtuple("Multiset", "name family values probes claim")   # probes: indices into values
Launch = namedtuple("Launch", "name g2 c keep window rows cols n_angles weight ratio labels")


def angles_bins(n_angles):
    b = np.linspace(-np.pi / 2, np.pi / 2, n_angles + 1)
    return (b[1:] + b[:-1]) / 2


def f64(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def one(b):
    return float(f64([b])[0])


def divergence_pass(lo, hi):
    """(pass of the radix select in which the prefixes of lo and hi part, highest differing bit); (None, None) when equal."""
    x = bit1(lo) ^ bit1(hi)
    if not x:
        return None, None
    t = x.bit_length() - 1
    return sum(t < b for b in DIGIT_BOUNDS), t


def middle(values):
    """(n, lo, hi, m) of the kept values: the order statistics (n-1)//2 and n//2 and numpy's median of them."""
    s = np.sort(np.asarray(values, dtype=np.float64))
    n = len(s)
    lo, hi = s[(n - 1) // 2], s[n // 2]
    with np.errstate(over="ignore"):
        m = lo if n & 1 else (lo + hi) / 2.0
    return n, float(lo), float(hi), float(m)


def probe_weight(a, m, c):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float64(a) / (np.float64(a) + np.float64(m)) * np.float64(c)
    return 0.0 if np.isnan(v) else float(v)


def closed_form(g2, c, bins, keep=None):
    """(weights, used_ratio) of one box in which no two lit pixels (c != 0, kept) share a bin: no sum is ever rounded."""
    g2, c = np.asarray(g2, dtype=np.complex128).ravel(), np.asarray(c, dtype=np.float64).ravel()
    with np.errstate(invalid="ignore"):
        a = np.hypot(g2.real, g2.imag)
        kept = ~np.isnan(a) & (a > 0)
    if keep is not None:
        kept &= np.asarray(keep).ravel() != 0
    w = np.zeros(len(bins))
    n = int(kept.sum())
    if n:
        m = middle(a[kept])[3]
        start, step = bins[0], bins[1] - bins[0]
        for p in np.flatnonzero(kept & (c != 0)):
            k = int(np.round((np.arctan2(g2.imag[p], g2.real[p]) - start) / step))
            k = 0 if k == len(bins) else k
            assert w[k] == 0.0, "two lit pixels in one bin"
            w[k] = probe_weight(a[p], m, c[p])
    return w, n / g2.size


# ------------------------------------------------------------------------------------------------------------ multisets
def _rng(name):
    return np.random.default_rng(list(name.encode()))


def bit1(x):
    """The bit pattern of one double, as a Python int."""
    return int(bits([x])[0])


def near(rng, b0, sign, count):
    """count distinct values 3 .. 2**22 ulps beyond the bit pattern b0 (sign -1: below), log-uniform in the distance."""
    d, seen = [], set()
    while len(d) < count:
        for x in np.exp2(rng.uniform(np.log2(3), 22, count)).astype(np.int64):
            if int(x) not in seen and len(d) < count:
                seen.add(int(x))
                d.append(int(x))
    return f64(np.array([int(b0) + sign * x for x in d], dtype=np.uint64))


def spread(rng, b_from, b_to, count):
    """count distinct random bit patterns in [b_from, b_to)."""
    out = set()
    while len(out) < count:
        out.update(int(x) for x in rng.integers(int(b_from), int(b_to), count - len(out), dtype=np.uint64))
    return f64(np.array(sorted(out), dtype=np.uint64))


def split_probes(lo, hi, ks=KS, fixed=FIXED, more=()):
    """The probe values other than lo itself, as (below lo, above hi)."""
    p = [lo * 2.0 ** k for k in ks if k] + ([fixed] if fixed is not None else []) + list(more)
    assert all((v < lo or v > hi) and v > 0 for v in p), (lo, hi, p)
    return [v for v in p if v < lo], [v for v in p if v > hi]


def assemble(name, family, below, mid, above, probes, **claim):
    """The multiset below + mid + above (the caller balances the sides), shuffled; probes: values, each a member."""
    vals = np.array(list(below) + list(mid) + list(above), dtype=np.float64)
    assert below == [] or max(below) <= min(mid)
    assert above == [] or min(above) >= max(mid)
    _rng(name).shuffle(vals)
    b = bits(vals)
    idx = []
    for p in probes:
        hit = np.flatnonzero(b == bit1(p))
        assert len(hit), (name, p)
        idx.append(int(hit[0]))
    assert len(set(idx)) == len(idx), name
    vals.setflags(write=False)
    return Multiset(name, family, vals, tuple(idx), claim)


def _around(name, family, lo, hi, n, drop_above=0, ks=KS, fixed=FIXED, **claim):
    """n values (n - drop_above in the end) whose middle pair is (lo, hi): the probes, then values `near` the pair on either side."""
    rng = _rng(name.replace("_odd", ""))   # the odd twin draws the same values
    pb, pa = split_probes(lo, hi, ks, fixed)
    side = (n - 2) // 2
    below = pb + list(near(rng, bit1(lo), -1, side - len(pb)))
    above = pa + list(near(rng, bit1(hi), +1, side - len(pa)))[drop_above:]
    return assemble(name, family, below, [lo, hi], above, [lo] + pb + pa, n=n - drop_above, **claim)


def diverge_pair(t):
    """Two bit patterns whose highest differing bit is t, garbage below it (the low 9 bits non-zero in both)."""
    g1, g2 = 0x3FD5A3C9E17B2D6B, 0x0012F6E4B8D3A5C7
    if t == 62:   # the exponents part, and 2 * lo must stay above hi (lo * 2**k is a member for k = 1)
        return 0x3FFFA3C9E17B2D6B, 0x4000F6E4B8D3A5C7
    if t == 53:
        return 0x3FDFA3C9E17B2D6B, 0x3FE0F6E4B8D3A5C7
    low = (1 << t) - 1
    high = g1 & ~((1 << (t + 1)) - 1)
    lo, hi = high | (g1 & low), high | (1 << t) | (g2 & low)
    if t < 9:   # keep garbage in the bits of the last digit that lie above t
        lo, hi = lo | (0x1AA & ~((1 << (t + 1)) - 1) & 0x1FF), hi | (0x1AA & ~((1 << (t + 1)) - 1) & 0x1FF)
    return lo, hi


def _diverge():
    out = []
    for t in DIVERGE_BITS:
        lo, hi = (one(b) for b in diverge_pair(t))
        p = sum(t < b for b in DIGIT_BOUNDS)
        fixed = 100.0 if lo <= FIXED <= hi else FIXED
        out.append(_around(f"diverge_bit{t}", "diverge", lo, hi, 1400, fixed=fixed, bit=t, **{"pass": p}))
        out.append(_around(f"diverge_bit{t}_odd", "diverge", lo, hi, 1400, drop_above=1, fixed=fixed, bit=None, **{"pass": None}))
    return out


def _dups():
    v, w = one(0x3FD5A3C9E17B2D6B), one(0x3FD5A3C9E17B2F11)
    out = [assemble("dup_all_equal_odd", "dup", [], [v] * 1399, [], [v], n=1399, run=(1399, 699)),
           assemble("dup_all_equal_even", "dup", [], [v] * 1400, [], [v], n=1400, run=(1400, 699)),
           assemble("dup_two_valued_half", "dup", [], [v] * 700 + [w] * 700, [], [v, w], n=1400, run=(700, 699)),
           assemble("dup_two_valued_off_half", "dup", [], [v] * 701 + [w] * 699, [], [v, w], n=1400, run=(701, 699))]
    for name, mid, n in (("dup_run2", [v, v], 1400), ("dup_run3", [v, v, v], 1401), ("dup_run_half", [v] * 700, 1400),
                         ("dup_run_to_run", [v, v, v, w, w, w], 1400)):
        rng = _rng(name)
        lo, hi = mid[(len(mid) - 1) // 2], mid[len(mid) // 2]
        pb, pa = split_probes(lo, hi)
        side = (n - len(mid)) // 2
        below = pb + list(near(rng, bit1(mid[0]), -1, side - len(pb)))
        above = pa + list(near(rng, bit1(mid[-1]), +1, side - len(pa)))
        run = sum(x == lo for x in mid)
        out.append(assemble(name, "dup", below, mid, above, [lo] + pb + pa + ([hi] if hi != lo else []), n=n,
                            run=(run, (n - 1) // 2 - side)))
    return out


def _counts():
    out = []
    for n in COUNTS:
        name = f"count_{n}"
        rng = _rng(name)
        if n <= 4:
            vals = list(spread(rng, bit1(2.0 ** -40), bit1(2.0 ** 40), n))
            out.append(assemble(name, "count", [], vals, [], vals, n=n))
            continue
        lo, hi = one(0x4008C5A3C9E17B2D), one(0x400B36E4B8D3A5C7)   # 3.09.. and 3.40..
        mid = [lo, hi] if n % 2 == 0 else [lo]
        pb, pa = split_probes(lo, mid[-1])
        side = (n - len(mid)) // 2
        below = pb + list(spread(rng, bit1(lo * 2.0 ** -40), bit1(lo), side - len(pb)))
        above = pa + list(spread(rng, bit1(mid[-1]) + 1, bit1(hi * 2.0 ** 40), side - len(pa)))
        out.append(assemble(name, "count", below, mid, above, [lo] + pb + pa, n=n))
    return out


def _ranges():
    out = []
    # every binade, 2**-1022 .. 2**1023, each with its own mantissa garbage
    rng = _rng("range_binades")
    man = rng.integers(1, 1 << 52, 2046, dtype=np.uint64)
    man[1022], man[1023] = 0xFA3C9E17B2D6B, 0x0F6E4B8D3A5C7   # the middle pair: 2 * lo (a member) stays above hi
    v = f64((np.arange(1, 2047, dtype=np.uint64) << np.uint64(52)) | man)   # v[i] is in binade i - 1022
    lo, hi = float(v[1022]), float(v[1023])
    pb, pa = split_probes(lo, hi, fixed=2.0 ** -7 * 1.5)
    below, above = pb + list(v[:1022]), pa + list(v[1024:])
    below += list(near(rng, bit1(lo), -1, max(len(above) - len(below), 0)))
    above += list(near(rng, bit1(hi), +1, max(len(below) - len(above), 0)))
    out.append(assemble("range_binades", "range", below, [lo, hi], above, [lo] + pb + pa, n=2 + 2 * len(below), **{"pass": 0}))
    # the smallest denormal as a member
    lo, hi = one(0x3FD5A3C9E17B2D6B), one(0x3FD5A3C9E17B2F11)
    rng = _rng("range_tiny_member")
    pb, pa = split_probes(lo, hi, more=(TINY,))
    below = pb + list(near(rng, bit1(lo), -1, 699 - len(pb)))
    above = pa + list(near(rng, bit1(hi), +1, 699 - len(pa)))
    out.append(assemble("range_tiny_member", "range", below, [lo, hi], above, [lo] + pb + pa, n=1400))
    # the smallest denormal as the median: the last of a run of it at the bottom
    pa = [TINY * 2.0 ** k for k in (1, 2, 10, 30)] + [FIXED]
    above = pa + list(spread(_rng("range_tiny_median"), 4, bit1(1.0), 695 - len(pa)))
    out.append(assemble("range_tiny_median", "range", [], [TINY] * 696, above, [TINY] + pa, n=1391, run=(696, 695)))
    # denormal lo and hi
    lo, hi = one(0x000000000ABCD123), one(0x000000000ABCD925)
    rng = _rng("range_denormal_pair")
    pb, pa = split_probes(lo, hi, ks=(-20, -1, 0, 1, 30))
    below = pb + list(near(rng, bit1(lo), -1, 699 - len(pb)))
    above = pa + list(near(rng, bit1(hi), +1, 699 - len(pa)))
    out.append(assemble("range_denormal_pair", "range", below, [lo, hi], above, [lo] + pb + pa, n=1400, **{"pass": 4}))
    # the largest finite double as both middle values: lo + hi overflows, m = inf
    rng = _rng("range_max_pair")
    pb = [MAXF * 2.0 ** k for k in (-30, -10, -2, -1)] + [FIXED]
    below = pb + list(near(rng, bit1(MAXF), -1, 699 - len(pb)))
    above = [MAXF] * 350 + [np.inf] * 349
    out.append(assemble("range_max_pair", "range", below, [MAXF, MAXF], above, [MAXF] + pb + [np.inf], n=1400, median=np.inf))
    # +inf among the upper half
    lo, hi = one(0x3FD5A3C9E17B2D6B), one(0x3FD5A3C9E17B2F11)
    rng = _rng("range_inf_above")
    pb, pa = split_probes(lo, hi, more=(np.inf,))
    below = pb + list(near(rng, bit1(lo), -1, 699 - len(pb)))
    above = pa + list(near(rng, bit1(hi), +1, 600 - len(pa))) + [np.inf] * 99
    out.append(assemble("range_inf_above", "range", below, [lo, hi], above, [lo] + pb + pa, n=1400))
    # +inf as the median: odd count, the middle value the first of a run of +inf
    rng = _rng("range_inf_median")
    pb = [FIXED, 2.0 ** -30, 0.37, 1e300, MAXF]
    below = pb + list(spread(rng, bit1(2.0 ** -40), bit1(2.0 ** 40), 699 - len(pb)))
    out.append(assemble("range_inf_median", "range", below, [np.inf], [np.inf] * 699, pb + [np.inf], n=1399, median=np.inf,
                        run=(700, 0)))
    return out


@functools.lru_cache(maxsize=None)
def multisets():
    out = _diverge() + _dups() + _counts() + _ranges()
    assert len({m.name for m in out}) == len(out)
    return tuple(out)


def multiset(name):
    return next(m for m in multisets() if m.name == name)


@functools.lru_cache(maxsize=None)
def group_a():
    """((multiset, window), ...): each multiset in a window with holes; the counts also in a window of exactly n pixels."""
    out = []
    for m in multisets():
        n = len(m.values)
        if m.family == "count":
            out.append((m, (1, n)))
        out.append((m, W_MAIN if n <= 1420 else W_BIG))
    return tuple(out)


DEVICE_ROUTE = ("diverge_bit0", "dup_run_to_run", "count_513", "range_denormal_pair")   # one per family, on device tensors


# ------------------------------------------------------------------------------------------------------------ placement
HOLES = (complex(np.nan, np.nan), 0j, complex(-0.0, 0.0), complex(np.nan, 0.0), complex(0.0, -0.0))


def box_of(m, window):
    """(|g2| box [wl, ws] (holes NaN), hole mask, flat pixel of each value): the values in row-major order between the holes."""
    wl, ws = window
    n, P = len(m.values), wl * ws
    assert n <= P
    rng = _rng(m.name + f"{wl}x{ws}")
    hole = np.zeros(P, bool)
    hole[rng.choice(P, P - n, replace=False)] = True
    a = np.full(P, np.nan)
    pix = np.flatnonzero(~hole)
    a[pix] = m.values
    return a.reshape(wl, ws), hole.reshape(wl, ws), pix


def pack(placements, variant, n_angles=N_ANGLES):
    """The launches of `placements` ((multiset, window) pairs), one per window shape: every multiset's box once per probe,
    side by side, copy k with c lit at probe k only.  variant: "plain" (holes NaN / 0.0 / -0.0, no keep), "ones" (the same
    with a keep of all ones) or "masked" (holes finite and positive, keep 0 on them).  Expected bits included."""
    assert variant in ("plain", "ones", "masked")
    bins = angles_bins(n_angles)
    k0 = int(np.round((0.0 - bins[0]) / (bins[1] - bins[0])))   # the bin of angle 0, by the expression of both sides
    by_window = {}
    for m, window in placements:
        by_window.setdefault(window, []).append(m)
    out = []
    for (wl, ws), ms in by_window.items():
        cols_n = sum(len(m.probes) for m in ms)
        g2 = np.empty((wl, ws * cols_n), dtype=np.complex128)
        c = np.zeros((wl, ws * cols_n))
        keep = np.ones((wl, ws * cols_n), np.uint8)
        weight, ratio, labels = np.zeros((1, cols_n, n_angles)), np.zeros((1, cols_n)), []
        j = 0
        for m in ms:
            a, hole, pix = box_of(m, (wl, ws))
            n, lo, hi, med = middle(m.values)
            box = a.astype(np.complex128)       # a + 0j
            hp = np.flatnonzero(hole.ravel())
            if variant == "masked":             # what would move the median and the bins if it were kept
                junk = np.where(np.arange(len(hp)) % 2 == 0, lo if np.isfinite(lo) else 1.0, 3.0 * FIXED)
                box.ravel()[hp] = junk + 0j
            else:
                box.ravel()[hp] = [HOLES[i % len(HOLES)] for i in range(len(hp))]
            for k, p in enumerate(m.probes):
                sl = slice(j * ws, (j + 1) * ws)
                g2[:, sl] = box
                cc = np.where(hole, C_HOLE, 0.0)
                cc.ravel()[pix[p]] = C_PROBES[k % len(C_PROBES)]
                c[:, sl] = cc
                if variant == "masked":
                    keep[:, sl] = ~hole
                weight[0, j, k0] = probe_weight(m.values[p], med, C_PROBES[k % len(C_PROBES)])
                ratio[0, j] = n / (wl * ws)
                labels.append(f"{m.name} {wl}x{ws} probe {k}")
                j += 1
        out.append(Launch(f"{variant} {wl}x{ws}", g2, c, None if variant == "plain" else keep, (wl, ws), [wl // 2],
                          [i * ws + ws // 2 for i in range(cols_n)], n_angles, weight, ratio, labels))
    return out


def boxes_of(launch):
    """(label, g2 box, c box, keep box or None, expected weights, expected ratio) of every window of a side-by-side launch."""
    wl, ws = launch.window
    for j, label in enumerate(launch.labels):
        sl = slice(j * ws, (j + 1) * ws)
        yield (label, launch.g2[:, sl], launch.c[:, sl], None if launch.keep is None else launch.keep[:, sl], launch.weight[0, j],
               launch.ratio[0, j])


# --------------------------------------------------------------------------------------------------------------- Group B
W_SWEEP = (5, 73)   # 365 pixels: room for one kept pixel per bin up to 360 bins


def one_per_bin(n_angles, seed=0):
    """(g2, c) of one W_SWEEP box: one kept pixel per bin at the bin's centre angle, |g2| and c (dyadic) differing from bin to
    bin, at shuffled positions; the other pixels NaN.  Every bin's weight is one product: a misplaced bin is an error of
    order one."""
    rng = np.random.default_rng(1000 * seed + n_angles)
    bins = angles_bins(n_angles)
    P = W_SWEEP[0] * W_SWEEP[1]
    g2 = np.full(P, complex(np.nan, np.nan))
    c = np.full(P, C_HOLE)
    pix = rng.permutation(P)[:n_angles]
    a = 0.5 + rng.permutation(n_angles) / n_angles * 3.0           # distinct magnitudes in [0.5, 3.5)
    g2[pix] = a * np.exp(1j * bins)
    c[pix] = (1 + (np.arange(n_angles) * 37) % 255) / 256.0        # k / 256, never 0
    return g2.reshape(W_SWEEP), c.reshape(W_SWEEP)


def several_windows(n_angles):
    """(g2, c, rows, cols): 2 x 3 W_SWEEP windows with different contents in one raster, the window (1, 1) empty (all NaN);
    the others hold one pixel per bin of a different seed, with every third (fourth, ...) pixel removed."""
    wl, ws = W_SWEEP
    g2 = np.full((2 * wl, 3 * ws), complex(np.nan, np.nan))
    c = np.full((2 * wl, 3 * ws), C_HOLE)
    for i in range(2):
        for j in range(3):
            if (i, j) == (1, 1):
                continue
            b2, bc = one_per_bin(n_angles, seed=1 + 3 * i + j)
            drop = np.flatnonzero(~np.isnan(b2.real).ravel())[::3 + 3 * i + j]
            b2.ravel()[drop] = complex(np.nan, np.nan)
            g2[i * wl:(i + 1) * wl, j * ws:(j + 1) * ws], c[i * wl:(i + 1) * wl, j * ws:(j + 1) * ws] = b2, bc
    return g2, c, [wl // 2, wl + wl // 2], [ws // 2, ws + ws // 2, 2 * ws + ws // 2]


PYTHAGOREAN = ((3, 4), (5, 12), (8, 15), (7, 24), (20, 21), (9, 40), (28, 45), (11, 60), (33, 56), (16, 63))
PYTH_SCALE = 2.0 ** -6
PYTH_ANGLES = (145, 360)


def pythagorean_probes():
    """The 40 probes (x + iy) * PYTH_SCALE: both orders of each pair and both signs of the imaginary part (the real part
    positive, as a principal root's), with their exact moduli."""
    z, r = [], []
    for x, y in PYTHAGOREAN:
        h = float(round((x * x + y * y) ** 0.5))
        assert h * h == x * x + y * y
        for re, im in ((x, y), (y, x), (x, -y), (y, -x)):
            z.append(complex(re, im) * PYTH_SCALE)
            r.append(h * PYTH_SCALE)
    return np.array(z), np.array(r)


@functools.lru_cache(maxsize=None)
def pythagorean_window():
    """(g2, c) of ONE W_MAIN window: the multiset of diverge_bit31 (its middle pair parts in the bottom bit of the third digit)
    with the 40 Pythagorean probes among its members, all lit at once; everything else real with c = 0."""
    z, r = pythagorean_probes()
    lo, hi = (one(b) for b in diverge_pair(31))
    rng = _rng("pythagorean")
    below, above = [v for v in r if v < lo], [v for v in r if v > hi]
    assert len(below) + len(above) == len(r)
    side = 699
    below = below + list(near(rng, bit1(lo), -1, side - len(below)))
    above = above + list(near(rng, bit1(hi), +1, side - len(above)))
    m = assemble("pythagorean", "diverge", below, [lo, hi], above, [lo, hi], n=1400, bit=31, **{"pass": 2})
    a, hole, pix = box_of(m, W_MAIN)
    g2 = a.astype(np.complex128)
    hp = np.flatnonzero(hole.ravel())
    g2.ravel()[hp] = [HOLES[i % len(HOLES)] for i in range(len(hp))]
    c = np.where(hole, C_HOLE, 0.0)
    vb = bits(m.values)
    used = set()
    for k, (zk, rk) in enumerate(zip(z, r)):
        i = next(int(i) for i in np.flatnonzero(vb == bit1(rk)) if int(i) not in used)
        used.add(i)
        g2.ravel()[pix[i]] = zk
        c.ravel()[pix[i]] = C_PROBES[k % len(C_PROBES)]
    g2.setflags(write=False)
    c.setflags(write=False)
    return g2, c


def random_box(seed=6):
    """A 37 x 53 box of principal roots with NaN, a zero and an angle of +pi/2, as tests/test_gpu_gradients.py draws it."""
    rng = np.random.default_rng(seed)
    g2 = np.sqrt(rng.normal(size=(37, 53)) + 1j * rng.normal(size=(37, 53)))
    g2[3, :7] = np.nan
    g2[5, 5] = 0
    g2[6, 6] = np.sqrt(-3 + 0j)
    return g2, rng.uniform(0, 1, g2.shape)


# --------------------------------------------------------------------------------------------------------------- Group C
GEOMETRY_RASTERS = ((7, 11), (40, 50))
GEOMETRY_WINDOWS = ((1, 1), (1, 7), (6, 1), (4, 9), (9, 4), (33, 20), (64, 64))


def rolling_box(a, i, j, wl, ws):
    """gradients_ref.rolling_window for a wl x ws window: rows i - wl//2 .. i - wl//2 + wl - 1, NaN outside the raster."""
    out = np.full((wl, ws), np.nan, dtype=a.dtype) if np.iscomplexobj(a) else np.full((wl, ws), np.nan)
    r0, c0 = i - wl // 2, j - ws // 2
    ra, rb, ca, cb = max(r0, 0), min(r0 + wl, a.shape[0]), max(c0, 0), min(c0 + ws, a.shape[1])
    if rb > ra and cb > ca:
        out[ra - r0:rb - r0, ca - c0:cb - c0] = a[ra:rb, ca:cb]
    return out


def geometry_centres(n, w):
    """Window centres along an axis of n pixels for a window of w: entirely outside on both sides, hanging over each end, on
    the first and the last pixel, inside."""
    return sorted({-w, -(w - w // 2), -1, 0, 1, n // 2, n - 2, n - 1, n + w // 2 - 1, n + w // 2, n + w})


def geometry_raster(shape, lit, kind):
    """(g2, c) of a raster.  kind "probe": g2 real and positive (distinct values over twelve binades, a few NaN and zeros),
    c one-hot at pixel `lit`: a window holds one lit probe or none, so its bits are expected whatever it clips.
    kind "random": complex principal roots and a random c, for the comparison at tolerance."""
    L, S = shape
    rng = np.random.default_rng(L * 1000 + S + (17 if kind == "random" else 0))
    if kind == "random":
        g2 = np.sqrt(rng.normal(size=shape) + 1j * rng.normal(size=shape))
        c = rng.uniform(0, 1, shape)
    else:
        g2 = (np.exp2(rng.uniform(-6, 6, shape)) + 0j)
        c = np.zeros(shape)
        c[lit] = C_PROBES[0]
    holes = rng.random(shape) < 0.08
    if lit is not None:
        holes[lit] = False
    g2[holes] = np.where(rng.random(int(holes.sum())) < 0.5, complex(np.nan, np.nan), 0j)
    return g2, c


def geometry_lit(shape):
    L, S = shape
    return ((0, 0), (L - 1, S - 1), (L // 2, S // 2), (0, S - 1))


def geometry_expected(g2, c, window, rows, cols, n_angles=N_ANGLES):
    """closed_form of every window of a launch: (weights [rows, cols, n_angles], ratios)."""
    bins = angles_bins(n_angles)
    w, r = np.zeros((len(rows), len(cols), n_angles)), np.zeros((len(rows), len(cols)))
    for a, i in enumerate(rows):
        for b, j in enumerate(cols):
            w[a, b], r[a, b] = closed_form(rolling_box(g2, i, j, *window), rolling_box(c, i, j, *window), bins)
    return w, r
