"""tests/hist_cases.py kept what it claims to be, without a GPU: every multiset's kept count, ranks, run lengths and the pass of the
radix select in which its two middle values part; the probes' power to tell the median from its neighbours in rank; and every
expected value of the GPU test (tests/test_gpu_hist_exact.py) held bit for bit to the restatement's gradient_histogram (numpy's
median, np.add.at), so that the closed form is never the ground truth by itself."""
import warnings

import numpy as np
import pytest

import gradients_ref as ref
import hist_cases as hc
from util import bits_equal

NAN = complex(np.nan, np.nan)


def nan_where_masked(g2, keep):
    out = np.array(g2, dtype=np.complex128)
    if keep is not None:
        out[np.asarray(keep) == 0] = NAN
    return out


def test_bins_are_the_restatements():
    for n in hc.SWEEP_ANGLES + hc.PYTH_ANGLES + (90,):
        assert bits_equal(hc.angles_bins(n), ref.angles_bins(n))


def test_the_families_are_all_there():
    fam = {}
    for m in hc.multisets():
        fam.setdefault(m.family, []).append(m.name)
    assert len(fam["diverge"]) == 24 and len(fam["dup"]) == 8 and len(fam["count"]) == 12 and len(fam["range"]) == 7
    assert [len(hc.multiset(f"count_{n}").values) for n in hc.COUNTS] == list(hc.COUNTS)
    assert {hc.multiset(n).family for n in hc.DEVICE_ROUTE} == set(fam)
    # six or more probes wherever the multiset has six distinct values to offer
    for m in hc.multisets():
        assert len(m.probes) >= min(6, len(np.unique(m.values))), m.name
        n, lo, hi, med = hc.middle(m.values)
        if m.family != "dup" and n > 4 and np.isfinite(lo):
            assert {lo * 2.0 ** k for k in (0, 1)} <= set(m.values[list(m.probes)]), m.name
    # windows: with holes (kept != read, the pixel count no multiple of the 512 threads), and of exactly n pixels for the counts
    for m, (wl, ws) in hc.group_a():
        assert wl * ws >= len(m.values) and ((wl * ws) % 512 != 0 or wl == 1)
    assert sum(1 for m, w in hc.group_a() if w[0] == 1 and w[1] == len(m.values)) == 12
    assert all(any(w != (1, len(m.values)) for mm, w in hc.group_a() if mm is m) for m in hc.multisets())


@pytest.mark.parametrize("m", hc.multisets(), ids=lambda m: m.name)
def test_claims(m):
    s = np.sort(m.values)
    n, lo, hi, med = hc.middle(m.values)
    assert n == m.claim["n"] == len(s)
    assert lo == s[(n - 1) // 2] and hi == s[n // 2]
    with np.errstate(over="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the sum of the largest finite double with itself
        assert bits_equal(np.float64(med), np.float64(np.median(m.values)))
    assert (m.values > 0).all() and not np.isnan(m.values).any()
    p, t = hc.divergence_pass(lo, hi)
    if "pass" in m.claim:
        assert p == m.claim["pass"]
    if "bit" in m.claim:
        assert t == m.claim["bit"]
    if "median" in m.claim:
        assert med == m.claim["median"]
    if "run" in m.claim:
        length, offset = m.claim["run"]
        first = int(np.searchsorted(s, lo, side="left"))
        assert int((s == lo).sum()) == length and (n - 1) // 2 - first == offset
    if m.family == "diverge":
        # garbage in the last digit of both middle values; the others 3 .. 2**22 ulps beyond the pair, apart from the probes;
        # the even case and its odd twin differ by one value above the middle
        assert hc.bit1(lo) & 0x1FF and hc.bit1(hi) & 0x1FF
        hi_even = hi if n % 2 == 0 else float(s[n // 2 + 1])
        b = hc.bits(s).astype(np.int64)
        d = np.where(s < lo, hc.bit1(lo) - b, b - hc.bit1(hi_even))
        close = (d >= 3) & (d <= 1 << 22)
        assert close.sum() >= n - 2 - 6 and (d[~close] > 1 << 22)[(s[~close] != lo) & (s[~close] != hi_even)].all()
        # every digit below the parting one still has neighbours to count: within 2**9 and beyond 2**20 ulps on either side
        for side in (s < lo, s > hi_even):
            assert (d[side] < 1 << 9).sum() >= 50 and (d[side & close] > 1 << 20).sum() >= 20
        if n % 2:
            twin = np.sort(hc.multiset(m.name[:-4]).values)
            assert len(twin) == n + 1 and lo == twin[n // 2] and set(s) < set(twin) and (np.setdiff1d(twin, s) > lo).all()
            assert p is None
    if m.name == "dup_two_valued_half":
        assert len(np.unique(s)) == 2 and lo != hi and (s == lo).sum() == (s == hi).sum() and med not in (lo, hi)
    if m.name == "dup_two_valued_off_half":
        assert len(np.unique(s)) == 2 and lo == hi == s[0] and (s == lo).sum() == n // 2 + 1
    if m.name == "dup_run_to_run":
        assert lo < hi and (s == lo).sum() == 3 and (s == hi).sum() == 3 and s[(n - 1) // 2 - 2] == lo and s[n // 2 + 2] == hi
    if m.name in ("dup_run2", "dup_run3", "dup_run_half"):
        assert lo == hi and 0 <= m.claim["run"][1] and n // 2 - int(np.searchsorted(s, lo)) < m.claim["run"][0]
    if m.family == "count":
        assert len(np.unique(hc.bits(s))) == n
    if m.name == "range_binades":
        assert set(np.frexp(s)[1] - 1) >= set(range(-1022, 1024))
    if m.name == "range_tiny_member":
        assert s[0] == hc.TINY and lo > 0.1
    if m.name == "range_tiny_median":
        assert lo == med == hc.TINY
    if m.name == "range_denormal_pair":
        assert 0 < lo < hi < np.finfo(np.float64).tiny
    if m.name == "range_max_pair":
        assert lo == hi == hc.MAXF and med == np.inf and np.isinf(s).any()
    if m.name == "range_inf_above":
        assert np.isinf(s[-99:]).all() and np.isfinite(med)
    if m.name == "range_inf_median":
        assert np.isinf(lo) and np.isfinite(s[(n - 1) // 2 - 1])


@pytest.mark.parametrize("m", hc.multisets(), ids=lambda m: m.name)
def test_probes_tell_the_median_from_its_neighbours(m):
    """Replace m by any of the eight values nearest in rank, or by either middle value: at least one probe weight changes."""
    s = np.sort(m.values)
    n, lo, hi, med = hc.middle(m.values)
    r0, r1 = (n - 1) // 2, n // 2
    near = [s[i] for i in list(range(max(r0 - 4, 0), r0)) + list(range(r1 + 1, min(r1 + 5, n)))] + [lo, hi]
    others = {float(x) for x in near if hc.bit1(x) != hc.bit1(med)}
    want = [hc.probe_weight(m.values[p], med, hc.C_PROBES[k % len(hc.C_PROBES)]) for k, p in enumerate(m.probes)]
    for x in sorted(others):
        got = [hc.probe_weight(m.values[p], x, hc.C_PROBES[k % len(hc.C_PROBES)]) for k, p in enumerate(m.probes)]
        assert not bits_equal(np.array(got), np.array(want)), f"{m.name}: a median of {x!r} in place of {med!r} would pass"
    if m.name not in ("dup_all_equal_odd", "dup_all_equal_even", "dup_run_half", "count_1"):   # these have no other value that near
        assert others, m.name


@pytest.mark.parametrize("variant", ["plain", "ones", "masked"])
def test_group_a_closed_form_is_the_restatement(variant):
    bins = ref.angles_bins(hc.N_ANGLES)
    n_win = 0
    for launch in hc.pack(hc.group_a(), variant):
        assert (launch.keep is None) == (variant == "plain")
        for label, g2, c, keep, w, r in hc.boxes_of(launch):
            hr, ur, _amb = ref.gradient_histogram(nan_where_masked(g2, keep), c, bins)
            assert bits_equal(w, hr) and r == ur, label
            cw, cr = hc.closed_form(g2, c, bins, keep)
            assert bits_equal(cw, w) and cr == r, label
            assert ((c != 0) & (c != hc.C_HOLE)).sum() == 1 and (g2.imag[~np.isnan(g2.imag)] == 0).all(), label
            if variant == "masked" and g2.size > len(launch.labels) and not keep.all():
                holes = g2.real[keep == 0]                                         # keep = 0 on finite g2, not NaN
                assert np.isfinite(holes).all() and (holes > 0).all() and not np.isnan(g2.real).any(), label
                unmasked = ref.gradient_histogram(g2, c, bins)[0]
                assert not bits_equal(unmasked, hr), label                         # and they would show if they were kept
            n_win += 1
    assert n_win == sum(len(m.probes) for m, _ in hc.group_a())


def test_group_a_launches_hold_every_hole_kind():
    launch = hc.pack(hc.group_a(), "plain")[0]
    g2 = launch.g2
    assert np.isnan(g2.real).any() and (np.isnan(g2.real) & ~np.isnan(g2.imag)).any()
    zero = (g2.real == 0) & (g2.imag == 0)
    assert (zero & np.signbit(g2.real)).any() and (zero & ~np.signbit(g2.real)).any()
    assert (g2.imag[~np.isnan(g2.real) & ~zero] == 0).all() and not np.signbit(g2.imag[~np.isnan(g2.real) & ~zero]).any()


# --------------------------------------------------------------------------------------------------------------- Group B
@pytest.mark.parametrize("n_angles", hc.SWEEP_ANGLES)
def test_one_per_bin(n_angles):
    bins = ref.angles_bins(n_angles)
    g2, c = hc.one_per_bin(n_angles)
    h, u, amb = ref.gradient_histogram(g2, c, bins)
    assert amb == 0.0 and (h > 0).all() and u == n_angles / g2.size
    k = np.round((np.angle(g2[~np.isnan(g2.real)]) - bins[0]) / (bins[1] - bins[0])).astype(int)
    assert sorted(k) == list(range(n_angles))
    assert len(np.unique(h)) == n_angles   # a bin that took another's value would show


@pytest.mark.parametrize("n_angles", hc.PYTH_ANGLES)
def test_several_windows(n_angles):
    bins = ref.angles_bins(n_angles)
    g2, c, rows, cols = hc.several_windows(n_angles)
    assert len(rows) == 2 and len(cols) == 3
    seen = []
    for i in rows:
        for j in cols:
            box = hc.rolling_box(g2, i, j, *hc.W_SWEEP)
            assert not np.isnan(box.real).all() or (i, j) == (rows[1], cols[1])
            h, u, amb = ref.gradient_histogram(box, hc.rolling_box(c, i, j, *hc.W_SWEEP), bins)
            assert amb == 0.0
            seen.append(h)
    assert (seen[4] == 0).all()
    for a in range(6):
        for b in range(a):
            assert (seen[a] != seen[b]).sum() > n_angles // 2 or 4 in (a, b)
    # the windows tile the raster: none reads another's pixels
    assert g2.shape == (2 * hc.W_SWEEP[0], 3 * hc.W_SWEEP[1])


def test_pythagorean_window():
    z, r = hc.pythagorean_probes()
    assert len(z) == 40 and (z.real > 0).all() and (z.imag < 0).sum() == 20
    assert bits_equal(np.hypot(z.real, z.imag), r) and bits_equal(np.abs(z), r)
    g2, c = hc.pythagorean_window()
    assert g2.shape == hc.W_MAIN
    lit = (c != 0) & (c != hc.C_HOLE)
    assert lit.sum() == 40 and (g2.imag[~lit & ~np.isnan(g2.imag)] == 0).all()
    edge = np.angle(z)
    u72 = (edge - hc.angles_bins(72)[0]) / (np.pi / 72)
    assert len(np.unique(np.round(u72))) == 32 and (np.abs(u72 - (np.floor(u72) + 0.5)) * np.pi / 72 > 1e-3).all()
    kept = np.abs(g2)[~np.isnan(np.abs(g2)) & (np.abs(g2) > 0)]
    n, lo, hi, med = hc.middle(kept)
    assert n == 1400 and hc.divergence_pass(lo, hi) == (2, 31)
    for n_angles in hc.PYTH_ANGLES:
        bins = ref.angles_bins(n_angles)
        step = bins[1] - bins[0]
        u = (edge - bins[0]) / step
        assert len(np.unique(np.round(u))) == 40                      # no two probes share a bin
        assert (np.abs(u - (np.floor(u) + 0.5)) * step > 1e-4).all()   # none within 1e-4 rad of an edge (atan2 errs by 1e-15)
        h, ur, _amb = ref.gradient_histogram(g2, c, bins)
        w, cr = hc.closed_form(g2, c, bins)
        assert bits_equal(w, h) and cr == ur and (w != 0).sum() == 40
        sweeps = np.bincount(np.flatnonzero(w) // 72)                # HIST_CHUNK = 72 bins per sweep
        if n_angles == 145:
            assert list(sweeps) == [20, 20]                           # half of the occupied bins lie in the second sweep
        else:
            assert len(sweeps) == 5 and (sweeps >= 4).all()           # and all five sweeps of 360 bins are occupied


def test_random_box_is_the_existing_one():
    g2, c = hc.random_box()
    assert g2.shape == (37, 53) and np.isnan(g2[3, 0]) and g2[5, 5] == 0 and np.angle(g2[6, 6]) == np.pi / 2
    for n in (90, 145):
        h, u, amb = ref.gradient_histogram(g2, c, ref.angles_bins(n))
        assert h.sum() > 0 and 0 < u < 1


# --------------------------------------------------------------------------------------------------------------- Group C
def test_rolling_box_is_rolling_window():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(7, 11)) + 1j * rng.normal(size=(7, 11))
    for w in (1, 4, 9, 64):
        for i in (-w, -1, 0, 3, 6, 7 + w):
            for j in (-w, 0, 5, 10, 11 + w):
                assert bits_equal(hc.rolling_box(a, i, j, w, w), ref.rolling_window(a, i, j, w))
                assert bits_equal(hc.rolling_box(a.real, i, j, w, w), ref.rolling_window(a.real, i, j, w))
    box = hc.rolling_box(a, 0, 10, 4, 9)   # rows -2 .. 1, columns 6 .. 14
    assert np.isnan(box[:2].real).all() and bits_equal(box[2:, :5], a[:2, 6:]) and np.isnan(box[:, 5:].real).all()


@pytest.mark.parametrize("shape", hc.GEOMETRY_RASTERS)
def test_geometry_cases(shape):
    """Every window shape meets: windows entirely outside on every side, hanging over each edge and corner, centred on the
    first and the last pixel, larger than the raster; the probe rasters' closed form is the restatement bit for bit; the random
    rasters have no ambiguous pixel."""
    L, S = shape
    bins = ref.angles_bins(hc.N_ANGLES)
    larger = set()
    for wl, ws in hc.GEOMETRY_WINDOWS:
        rows, cols = hc.geometry_centres(L, wl), hc.geometry_centres(S, ws)
        r0, c0 = np.array(rows) - wl // 2, np.array(cols) - ws // 2
        for lo, w, n in ((r0, wl, L), (c0, ws, S)):
            assert (lo + w <= 0).any() and (lo >= n).any()                       # entirely outside, both sides
            assert (lo + w == 0).any() and (lo == n).any()                       # by exactly one pixel
            assert 0 in lo + w // 2 and n - 1 in lo + w // 2                     # centred on the first and the last pixel
            if w > 1:
                assert ((lo < 0) & (lo + w > 0)).any() and ((lo < n) & (lo + w > n)).any()   # hanging over each edge
        larger.add((wl > L, ws > S))
        g2, c = hc.geometry_raster(shape, None, "random")
        assert np.isnan(g2.real).any() and (g2 == 0).any() and (g2.imag[~np.isnan(g2.imag)] != 0).any()
        for i in rows:
            for j in cols:
                assert ref.gradient_histogram(hc.rolling_box(g2, i, j, wl, ws), hc.rolling_box(c, i, j, wl, ws), bins)[2] == 0.0
        for lit in hc.geometry_lit(shape):
            g2, c = hc.geometry_raster(shape, lit, "probe")
            assert (c != 0).sum() == 1 and (g2.imag[~np.isnan(g2.imag)] == 0).all()
            w, r = hc.geometry_expected(g2, c, (wl, ws), rows, cols)
            n_lit = 0
            for a, i in enumerate(rows):
                for b, j in enumerate(cols):
                    h, u, _ = ref.gradient_histogram(hc.rolling_box(g2, i, j, wl, ws), hc.rolling_box(c, i, j, wl, ws), bins)
                    assert bits_equal(w[a, b], h) and r[a, b] == (0.0 if np.isnan(u) else u), (wl, ws, i, j)
                    n_lit += bool(h.any())
            assert 0 < n_lit < len(rows) * len(cols)
            assert (r == 0).any() and (((r > 0) & (r < 1)).any() or wl * ws == 1)
    assert {(True, True), (False, False)} <= larger and (shape != (7, 11) or (True, False) in larger)
