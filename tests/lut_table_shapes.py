"""The co-pol tables at which the tests hold a LUT install's device-built tables to their restatement (tests/lut_tables_ref.py):
tests/test_gpu_lut_tables.py installs each and reads every table back; tests/test_lut_tables_cpu.py holds each entry to the edge it
is here for, computed from the geometry, and the content to the classes listed below.

shape = (n_inc, n_w, n_phi), the smallest that reaches the edge:

  one_block     (3, 9, 5)        everything inside one block, cell, tile and wave; phi_pad 8 > n_phi; two blocks and one row; one band
  default_phi   (2, 33, 181)     the default direction axis (phi_pad 184): last block 5 directions wide, last sub-block 1; nbc 12 ->
                                 blk_g 5, nine block rows: two bands, the second of four block rows (at 37 speed rows it would be
                                 a whole five); two cell rows; level 7 != level 6; three lane trips of k_pad_co
  wide_phi      (2, 70, 300)     n_phi > 256: second trip of k_tail_min's loops; no pad column; transpose tiles ragged both ways
  band_per_row  (1, 6, 1030)     nbc 65 > 64 -> blk_g 1, one band per block row; a single slice
  many_rows     (70, 500, 6)     35 000 rows > 32 768: k_pad_co's grid stride; two workgroups of k_mono_rows / k_inv_rows, ragged
  no_inverse    (2048, 2, 512)   inv_n * 2 = 2^32 bytes: inv_rows / inv_grid absent, everything else present

Content (seeded; `table(key)` builds it, the same on every call).  Each slice is of one KIND:
  "sat"    rises, then falls (a saturating GMF).  The descent starts at row `mono` in ONE direction (never direction 0), later
           in about a third of the others, never in the rest: mono_rows is set by that one direction and differs between slices.
  "mono"   non-decreasing throughout (mono == n_w, tail_min all +inf).
  "mono1"  a "sat" slice whose one early direction already falls at row 1.
  "flat"   one constant: a slice of no width.
Every kind but "flat" has equal neighbours along the speed axis, values of both signs, and every third direction holds multiples of
1/64 (float32 holds them exactly) beside directions of arbitrary doubles.  In the first "sat" slice of a table with room for it
(`plants`), one entry is set to a threshold t_b exactly, and one to the smaller of the fused and the unfused t_b at a bin where the
two differ (found by search)."""
import functools
from collections import namedtuple

import numpy as np

import lut_tables_ref as ref

SHAPES = {
    "one_block": (3, 9, 5),
    "default_phi": (2, 33, 181),
    "wide_phi": (2, 70, 300),
    "band_per_row": (1, 6, 1030),
    "many_rows": (70, 500, 6),
    "no_inverse": (2048, 2, 512),
}
# the order of the GPU test's installs on one context: a smaller table after a larger one and back
INSTALL_ORDER = ("default_phi", "one_block", "many_rows", "band_per_row", "no_inverse", "wide_phi", "one_block")

KINDS = {
    "one_block": ("sat", "mono1", "mono"),
    "default_phi": ("sat", "sat"),
    "wide_phi": ("sat", "mono"),
    "band_per_row": ("sat",),
    "many_rows": ("sat", "sat", "mono", "mono1", "flat", "sat", "sat"),  # cycled
    "no_inverse": ("sat", "mono", "flat"),                               # cycled
}

Plant = namedtuple("Plant", "slice row phi bin")  # dense[slice, row, phi] was set by bin `bin` of that slice's threshold grid


def kind(key, i):
    return KINDS[key][i % len(KINDS[key])]


def descent_row(n_w, i):
    """`mono` of "sat" slice i: two thirds up the axis, shifted by the slice so that neighbours differ."""
    return max(1, (2 * n_w) // 3 - i % 3)


def descent_phi(n_phi, i):
    p = (7 * i + 3) % n_phi
    return p if p else 1


def unfused(b, width, t0):
    return b * width + t0


def _slice(rng, what, i, n_w, n_phi):
    if what == "flat":
        return np.full((n_w, n_phi), -7.25 + 0.5 * (i % 5))
    scale = 40.0 / max(n_w, 2)
    step = rng.uniform(0.1, 1.0, (n_w, n_phi)) * scale
    step[rng.random((n_w, n_phi)) < 0.1] = 0.0  # equal neighbours
    first = np.full(n_phi, n_w)  # first row lower than its predecessor, per direction
    if what != "mono":
        m, p1 = (1 if what == "mono1" else descent_row(n_w, i)), descent_phi(n_phi, i)
        later = rng.random(n_phi) < 0.35
        later[0] = True  # direction 0 descends, but not first
        first[later] = np.minimum(m + 1 + rng.integers(0, 4, n_phi), n_w)[later]
        first[p1] = m
    falls = np.arange(n_w)[:, None] >= first[None, :]
    step[falls] = -rng.uniform(0.1, 1.0, (n_w, n_phi))[falls] * scale
    v0 = -8.0 + 3.0 * np.cos(np.radians(2.0 * np.arange(n_phi))) + rng.uniform(-0.5, 0.5, n_phi)
    exact = np.arange(n_phi) % 3 == 0
    q = np.sign(step) * np.ceil(np.abs(step) * 64.0) / 64.0
    step[:, exact] = q[:, exact]
    v0[exact] = np.round(v0[exact] * 64.0) / 64.0
    step[0] = v0
    out = np.cumsum(step, axis=0)  # sequential sums: value + 0.0 is the value
    # the slice's minimum sits in a direction of arbitrary doubles: a threshold grid between two multiples of 1/64 would have a
    # width of few bits, b * width would be exact and the fused threshold never differ from the unfused one
    c = 2 if (what != "mono" and p1 == 1) else 1
    out[0, c] = out.min() - 0.123456789
    return out


def _plant(dense, i, want_differ, taken):
    """Sets one interior entry of the monotone rows of slice i to min(fused, unfused) t_b, strictly between its neighbours along
    the speed axis, at a bin where the two agree (want_differ False) or differ; None when the slice has no room."""
    sl = dense[i]
    mono = int(ref.mono_rows(dense[i:i + 1])[0])
    grid = ref.inv_grid(dense[i:i + 1], [mono])[0]
    if grid[1] == 0.0:
        return None
    t0, width, inv_width = grid
    for p in range(1, sl.shape[1]):
        if p % 3 == 0 or p in taken:
            continue
        for r in range(1, mono - 1):
            lo, hi = sl[r - 1, p], sl[r + 1, p]
            b0, b1 = int((lo - t0) * inv_width) + 2, min(int((hi - t0) * inv_width) - 1, ref.INV_BINS - 1)
            for b in range(max(b0, 1), b1 + 1):
                tf, tu = ref.fma_exact(float(b), width, t0), unfused(b, width, t0)
                if (tf != tu) != want_differ or not (lo < min(tf, tu) and max(tf, tu) < hi):
                    continue
                old = sl[r, p]
                sl[r, p] = min(tf, tu)
                if int(ref.mono_rows(dense[i:i + 1])[0]) == mono and np.array_equal(ref.inv_grid(dense[i:i + 1], [mono])[0], grid):
                    return Plant(i, r, p, b)
                sl[r, p] = old
    return None


@functools.lru_cache(maxsize=None)
def _build(key):
    n_inc, n_w, n_phi = SHAPES[key]
    rng = np.random.default_rng(list(key.encode()))
    dense = np.empty((n_inc, n_w, n_phi))
    for i in range(n_inc):
        dense[i] = _slice(rng, kind(key, i), i, n_w, n_phi)
    plants = {}
    i0 = next(i for i in range(n_inc) if kind(key, i) == "sat")
    if ref.geometry(n_inc, n_w, n_phi).inv_ok:
        exact = _plant(dense, i0, False, ())
        if exact:
            plants["exact"] = exact
            differ = _plant(dense, i0, True, (exact.phi,))
            if differ:
                plants["unfused"] = differ
    dense.setflags(write=False)
    return dense, plants


def table(key):
    """The dense dB table of SHAPES[key], read-only."""
    return _build(key)[0]


def plants(key):
    """{"exact": Plant, "unfused": Plant} of the table (empty where the monotone part has no interior row, or no inverse)."""
    return dict(_build(key)[1])


def axes(key):
    """Uniform axes for an install: the table is searchable as far as its values allow."""
    n_inc, n_w, n_phi = SHAPES[key]
    return np.linspace(17.0, 50.0, n_inc) if n_inc > 1 else np.array([30.0]), np.linspace(0.5, 50.0, n_w), np.linspace(0.0, 180.0, n_phi)
