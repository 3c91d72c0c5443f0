"""The exact reference for sigma0 -> dB on a float32 raster (xsw_device.hpp: to_db(float)), and the adjudicator that holds a
device value to it.  TEST INFRASTRUCTURE ONLY; standard library and numpy.

    E(x) = fl32(10f * RN32(log10(y))),   y = fl32(x + 1e-15f)

RN32 is round-to-nearest-even to float32 of the EXACT logarithm (`decimal` at PREC digits: a widened float32 is a finite decimal,
and Decimal.log10 is correctly rounded to the context's precision).  y == 0 gives -inf, y < 0 or NaN gives NaN, +inf gives +inf.

The kernel rounds twice (a float64 logarithm good to ~1e-15, then float32), so it may legitimately return 10f * l for the OTHER
float32 neighbour l of the exact logarithm -- but only where the logarithm lies within ALLOW * |L| of the boundary between the
two neighbours.  `judge` gives that verdict for one argument, `adjudicate` for a list.

A float64 log10 that is right to DECIDE relative settles every argument whose logarithm lies further than DECIDE * |L| from both
rounding boundaries around it (`decided`): that is the filter of the full sweep (tests/test_gpu_db_f32.py, on the device through
torch) and of the CPU test (tests/test_db_f32_cpu.py, numpy); what it does not settle is judged exactly."""
import decimal
import functools
from collections import namedtuple

import numpy as np

EPS32 = np.float32(1e-15)
TEN32 = np.float32(10.0)
PREC = 70        # digits of the exact logarithm (|L| <= 45: 68 digits behind the point)
DECIDE = 1e-13   # the filter: a float64 log10 right to this settles an argument further than this from a boundary
ALLOW = 2e-15    # a double rounding is legitimate within this of the boundary (the header's "~1e-15", doubled)
HOST_MAX = 1 << 16  # a piece of the sweep that sends more arguments than this to the host has a broken filter

_LOG = decimal.Context(prec=PREC)
_WIDE = decimal.Context(prec=400)  # sums and halves of widened float32 values: exact
_INF32 = np.float32(np.inf)


def as_f32(patterns):
    return np.asarray(patterns, dtype=np.uint32).view(np.float32)


def as_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def y_of(x):
    """fl32(x + 1e-15f).  (Never a denormal: below 2**-74 the sum is 1e-15f itself, above it is a multiple of 2**-73.)"""
    with np.errstate(all="ignore"):
        return np.asarray(x, dtype=np.float32) + EPS32


def decided(L, c, up, dn, xp=np):
    """The filter, on numpy arrays or torch tensors (xp = numpy or torch).  L: a float64 log10; c: L rounded to float32; up, dn:
    c's float32 neighbours; the three widened to float64 (the midpoints are then exact).  True where RN32 of any value within
    DECIDE * |L| of L is c -- and for L == 0 (y == 1: exact) and the specials (-inf, +inf, NaN), which have no neighbours."""
    d = xp.minimum(xp.abs(L - (c + up) * 0.5), xp.abs(L - (c + dn) * 0.5))
    return (d > DECIDE * xp.abs(L)) | (L == 0) | ~xp.isfinite(L)


def predict_np(x, log10=None):
    """(prediction, decided) of a float32 array in numpy: 10f * fl32(log10(float64(y))) and the filter."""
    y = y_of(x)
    with np.errstate(all="ignore"):
        L = (log10 or np.log10)(y.astype(np.float64))
        c = L.astype(np.float32)
        up, dn = np.nextafter(c, _INF32), np.nextafter(c, -_INF32)
        ok = decided(L, c.astype(np.float64), up.astype(np.float64), dn.astype(np.float64))
        return TEN32 * c, ok


Exact = namedtuple("Exact", "L lo hi rn other dist")  # dist: |L - boundary| / |L| (inf where L is a float32)


@functools.lru_cache(maxsize=1 << 16)
def exact_log10(y):
    """The exact logarithm of a positive finite float and its float32 frame: neighbours lo <= L <= hi, RN32(L), the other
    neighbour, and the relative distance of L from the boundary between the two."""
    L = _LOG.log10(decimal.Decimal(float(y)))
    c = np.float32(float(L))  # within one ulp of L on either side
    dc = decimal.Decimal(float(c))
    if dc == L:
        return Exact(L, c, c, c, c, np.inf)
    lo, hi = (c, np.nextafter(c, _INF32)) if dc < L else (np.nextafter(c, -_INF32), c)
    mid = _WIDE.divide(_WIDE.add(decimal.Decimal(float(lo)), decimal.Decimal(float(hi))), decimal.Decimal(2))
    if L == mid:
        rn = lo if int(as_bits(lo)) & 1 == 0 else hi
    else:
        rn = lo if L < mid else hi
    other = hi if rn is lo else lo
    return Exact(L, lo, hi, rn, other, float(abs(L - mid) / abs(L)))


def expected(pattern):
    """E(x) of one float32 bit pattern, as float32."""
    y = y_of(as_f32(pattern))
    if np.isnan(y) or y < 0:
        return np.float32(np.nan)
    if y == 0:
        return np.float32(-np.inf)
    if np.isinf(y):
        return _INF32
    return TEN32 * exact_log10(float(y)).rn


def _same(a, b):
    return (a == b) or (np.isnan(a) and np.isnan(b))


Verdict = namedtuple("Verdict", "kind dist message")  # kind: "equal", "double" (a legitimate double rounding) or "wrong"


def judge(pattern, got):
    """The verdict on the device value `got` (float32) of one argument."""
    pattern, got = int(pattern), np.float32(got)
    want = expected(pattern)
    y = y_of(as_f32(pattern))
    e = exact_log10(float(y)) if np.isfinite(y) and y > 0 else None
    dist = None if e is None else e.dist
    if _same(got, want):
        return Verdict("equal", dist, "")
    if e is not None:
        if e.other is not e.rn and got == TEN32 * e.other and dist <= ALLOW:
            return Verdict("double", dist, "")
    where = "" if dist is None else f", log10 lies {dist / 1e-15:.3g} x 1e-15 |L| from the rounding boundary"
    return Verdict("wrong", dist, f"x = 0x{pattern:08X} ({as_f32(pattern)!r}): got {got!r} (0x{int(as_bits(got)):08X}), "
                                  f"expected {want!r} (0x{int(as_bits(want)):08X}){where}")


# doubles: [(pattern, dist in units of 1e-15 |L|)]; wrong: [message]; closest: (dist in those units, pattern) of the judged argument
# nearest its rounding boundary, or None
Report = namedtuple("Report", "judged doubles wrong closest")


def adjudicate(patterns, got):
    doubles, wrong, closest = [], [], None
    for p, g in zip(np.asarray(patterns, dtype=np.uint32).tolist(), np.asarray(got, dtype=np.float32)):
        v = judge(p, g)
        if v.dist is not None and (closest is None or v.dist / 1e-15 < closest[0]):
            closest = (v.dist / 1e-15, p)
        if v.kind == "double":
            doubles.append((p, v.dist / 1e-15))
        elif v.kind == "wrong":
            wrong.append(v.message)
    return Report(len(patterns), doubles, wrong, closest)


def summary(what, rep):
    worst = max((d for _, d in rep.doubles), default=0.0)
    near = "" if rep.closest is None else f"; nearest a boundary 0x{rep.closest[1]:08X} at {rep.closest[0]:.3g} x 1e-15 |L|"
    return (f"{what}: {rep.judged} arguments judged exactly, {len(rep.doubles)} legitimate double roundings "
            f"[{', '.join(f'0x{p:08X}' for p, _ in rep.doubles)}], largest distance {worst:.3g} x 1e-15 |L|, {len(rep.wrong)} wrong{near}")


def check(x, got, what=""):
    """The whole method on the host: settle by the numpy filter, judge the rest exactly.  Returns the Report; the caller asserts."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    got = np.ascontiguousarray(got, dtype=np.float32).ravel()
    pred, ok = predict_np(x)
    settled = ok & ((got == pred) | (np.isnan(got) & np.isnan(pred)))
    idx = np.flatnonzero(~settled)
    assert idx.size <= HOST_MAX, f"{what}: {idx.size} arguments not settled by the filter"
    return adjudicate(as_bits(x)[idx], got[idx])


# ------------------------------------------------------------------------------------------------ arguments
SPECIAL_PATTERNS = (
    0x00000000,  # +0
    0x80000000,  # -0
    0xA6901D7D,  # -1e-15f: y == 0
    0xA6901D7C,  # one ulp nearer zero: the smallest positive y, 2**-73
    0xA6901D7E,  # one ulp further: y == -2**-73
    0x00000001,  # the smallest denormal
    0x00800000,  # FLT_MIN
    0x7F7FFFFF,  # FLT_MAX
    0x7F800000,  # +inf
    0x7FC00000,  # NaN
    0xBF800000,  # -1
    0x3F800000,  # 1.0f
)


@functools.lru_cache(maxsize=None)
def near_boundary(first_pattern):
    """The arguments x of the binade that starts at bit pattern `first_pattern` which the numpy filter does not settle."""
    x = as_f32(np.arange(first_pattern, first_pattern + (1 << 23), dtype=np.uint32))
    _, ok = predict_np(x)
    out = as_bits(x)[~ok]
    out.setflags(write=False)
    return out


BINADE_2M7, BINADE_HALF, BINADE_ONE = 0x3C000000, 0x3F000000, 0x3F800000  # [2**-7, 2**-6), [0.5, 1), [1, 2)


@functools.lru_cache(maxsize=None)
def hard_arguments():
    """float32 values: the specials, every binade edge +- 1 ulp from 2**-74 to 2**127, and the near-boundary arguments of three
    binades.  Read-only."""
    edges = np.array([((e + 127) << 23) + d for e in range(-74, 128) for d in (-1, 0, 1)], dtype=np.uint32)
    bits = np.concatenate([np.array(SPECIAL_PATTERNS, dtype=np.uint32), edges] + [near_boundary(b) for b in (BINADE_2M7, BINADE_HALF, BINADE_ONE)])
    out = bits.view(np.float32)
    out.setflags(write=False)
    return out
