"""CPU: the restatement of xsarsea_amd.streaks (tests/streaks_ref.py) and the module's host geometry, pinned on hand-built cases."""
import numpy as np
import pytest

import gradients_ref as ref
import streak_cases as sc
import streaks_ref as sref
from util import bits_equal
from xsarsea_amd import _lib, gradients, streaks

BINS = ref.angles_bins(72)
STEP = BINS[1] - BINS[0]
NAN = complex(np.nan, np.nan)


def one_window(hist):
    """[C, 1, 1, n] weights and [C, 1, 1] used ratios from C histograms of one window."""
    h = np.atleast_2d(np.asarray(hist, dtype=np.float64))
    return h[:, None, None, :], np.ones((h.shape[0], 1, 1))


def delta(k, n=72, v=1.0):
    h = np.zeros(n)
    h[k] = v
    return h


@pytest.mark.parametrize("k", [0, 71, 35])
def test_peak_at_the_first_and_last_bin_wraps(k):
    w, r = one_window(delta(k))
    s = sref.streaks_direction(w, r, BINS)
    assert s["index"][0, 0] == k
    m = s["m"][0, 0]
    np.testing.assert_array_equal(m, np.roll(sref.circ_smooth(delta(35)), k - 35))  # the smoothing is exactly circular
    assert m[(k - 3) % 72] == m[(k + 3) % 72] > 0 and s["weight"][0, 0] == m[k]
    assert m.sum() == pytest.approx(1.0, rel=1e-15)


def test_circ_smooth_restatements_agree():
    h = np.random.default_rng(1).uniform(0, 1, (5, 72))
    np.testing.assert_array_equal(sref.circ_smooth(h), gradients.circ_smooth(h))  # the package's tap order, bit for bit
    np.testing.assert_allclose(sref.circ_smooth(h), ref.circ_smooth(h), rtol=1e-14)
    h8 = np.random.default_rng(2).uniform(0, 1, 8)  # shorter than the widest kernel: the taps wrap more than once
    np.testing.assert_array_equal(sref.circ_smooth(h8), gradients.circ_smooth(h8))


def test_tie_takes_the_first_index():
    h = delta(10) + delta(50)  # the two smoothed bumps are translates of each other: equal maxima
    w, r = one_window(h)
    s = sref.streaks_direction(w, r, BINS)
    assert s["m"][0, 0, 10] == s["m"][0, 0, 50] and s["index"][0, 0] == 10
    assert sref.near_tie(s["m"])[0, 0]
    s = sref.streaks_direction(w, r, BINS, smooth=False)
    assert s["index"][0, 0] == 10 and s["weight"][0, 0] == 1.0


def test_all_nan_and_all_zero_windows():
    for h in (np.full(72, np.nan), np.zeros(72)):
        w, r = one_window(h)
        s = sref.streaks_direction(w, r * np.nan if np.isnan(h[0]) else r, BINS)
        assert s["index"][0, 0] == 0 and s["angle"][0, 0] == BINS[0] + np.pi / 2
        assert np.isnan(s["weight"][0, 0]) == bool(np.isnan(h[0]))
        assert not sref.near_tie(s["m"])[0, 0]  # nothing to exclude: both evaluations give bin 0
    assert np.isnan(sref.streaks_direction(*one_window(np.full(72, np.nan)), BINS)["weight"][0, 0])
    assert np.isnan(sref.nanmean_leading(np.full((3, 1, 1), np.nan), 2)[0, 0])


def test_nan_in_one_configuration_is_skipped_by_the_mean():
    a, b = delta(20, v=2.0), np.full(72, np.nan)
    c = delta(20, v=4.0)
    w, _ = one_window([a, b, c])
    m = sref.nanmean_leading(w, 3)[0, 0]
    assert m[20] == 3.0 and m[0] == 0.0  # (2 + 4) / 2: the NaN histogram does not count
    w[1, 0, 0, 5] = 7.0  # one finite bin in the NaN configuration: that bin averages three terms
    assert sref.nanmean_leading(w, 3)[0, 0, 5] == 7.0 / 3
    r = np.array([0.5, np.nan, 1.0])[:, None, None]
    assert sref.streaks_direction(w, r, BINS)["used_ratio"][0, 0] == 0.75
    lead = np.arange(24.0).reshape(2, 3, 4, 1, 1)  # leading axes are flattened in order
    assert sref.nanmean_leading(lead, 2)[0, 0] == np.arange(24.0).sum() / 24


def test_orthogonal_on_and_off():
    w, r = one_window(delta(30))
    on, off = sref.streaks_direction(w, r, BINS), sref.streaks_direction(w, r, BINS, orthogonal=False)
    assert off["angle"][0, 0] == BINS[30] and on["angle"][0, 0] == BINS[30] + np.pi / 2  # one float64 addition
    assert on["index"][0, 0] == off["index"][0, 0] == 30


def test_resolve_sign_flip_exactly_at_a_zero_dot_product():
    angle = np.array([[0.0, 0.0, 0.0, np.pi / 2, -np.pi / 2, 0.3, 0.3, np.nan, 0.3]])
    a = np.array([[5j, -5j, -1 + 5j, 2j, 2j, 0, 1 + 1j, 1 + 1j, complex(np.nan, 1)]])
    weight = np.ones(angle.shape)
    d = sref.resolve(angle, weight, weight, a)
    assert d[0, 0] == 1 and d[0, 1] == 1  # exp(0j) . (0, +-5) == 0: kept
    assert d[0, 2] == -1  # a negative dot product flips
    assert d[0, 3] == np.exp(0.5j * np.pi) and d[0, 4] == -np.exp(-0.5j * np.pi)  # +-pi/2 against +2j
    assert np.isnan(d[0, 5]) and d[0, 6] == np.exp(0.3j) and np.isnan(d[0, 7]) and np.isnan(d[0, 8])
    weight[0, 6] = np.nan
    assert np.isnan(sref.resolve(angle, weight, np.ones(angle.shape), a)[0, 6])
    weight[0, 6] = 0.2
    ratio = np.full(angle.shape, 0.4)
    assert np.isnan(sref.resolve(angle, weight, ratio, a, min_weight=0.25)[0, 6])
    assert sref.resolve(angle, weight, ratio, a, min_weight=0.2, min_used_ratio=0.4)[0, 6] == np.exp(0.3j)  # equality passes
    assert np.isnan(sref.resolve(angle, weight, ratio, a, min_used_ratio=0.5)[0, 6])


def test_bracket_clamps_outside_the_centres_and_matches_the_package():
    c = np.array([10.0, 20.0, 50.0])
    x = np.array([-5.0, 10.0, 12.5, 20.0, 35.0, 50.0, 80.0])
    i0, i1, t = sref.bracket(c, x)
    np.testing.assert_array_equal(i0, [0, 0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(i1, [0, 0, 1, 2, 2, 2, 2])
    np.testing.assert_array_equal(t, [0, 0, 0.25, 0, 0.5, 0, 0])
    first, tt = streaks.bracket(c, x)
    assert first.dtype == np.int32 and tt.dtype == np.float64
    # the package names the bracket by its first centre; the second is the next one, or the same past the last
    np.testing.assert_array_equal(tt, t)
    same = (t == 0) & (i0 == i1)
    np.testing.assert_array_equal(first[~same], i0[~same])
    np.testing.assert_array_equal(np.minimum(first + 1, len(c) - 1)[~same], i1[~same])
    rng = np.random.default_rng(3)
    c = np.cumsum(rng.uniform(0.5, 30, 17))  # irregular centres, float coordinates
    x = np.sort(rng.uniform(c[0] - 20, c[-1] + 20, 400))
    i0, i1, t = sref.bracket(c, x)
    first, tt = streaks.bracket(c, x)
    np.testing.assert_array_equal(tt, t)
    np.testing.assert_array_equal(c[first] * (1 - tt) + c[np.minimum(first + 1, 16)] * tt, c[i0] * (1 - t) + c[i1] * t)
    with pytest.raises(ValueError):
        streaks.bracket([3.0, 2.0], x)


def test_single_row_of_windows_is_constant_along_lines():
    dirs = np.exp(1j * np.array([[0.2, 1.2, 2.0]]))
    anc = np.full((5, 7), 3 + 4j)
    out = sref.ancillary(dirs, [2.0], [1.0, 3.0, 5.0], anc, np.arange(5.0), np.arange(7.0))
    np.testing.assert_array_equal(out, np.broadcast_to(out[0], out.shape))
    np.testing.assert_allclose(np.abs(out), 5.0, rtol=1e-15)
    np.testing.assert_allclose(out[0, [0, 1, 3, 5, 6]], 5 * dirs[0, [0, 0, 1, 2, 2]], rtol=1e-15)  # clamped at both ends
    v = 0.5 * dirs[0, 0] + 0.5 * dirs[0, 1]
    np.testing.assert_allclose(out[0, 2], 5 * v / abs(v), rtol=1e-15)
    first, t = streaks.bracket([2.0], np.arange(5.0))
    assert not first.any() and not t.any()


def test_nan_corners_are_skipped_and_the_model_survives_where_nothing_is_valid():
    dirs = np.array([[1, NAN, NAN], [1j, NAN, NAN]])
    anc = np.full((3, 5), -2 + 0j)
    anc[2, 4] = complex(1, np.nan)
    anc[0, 1] = 0
    out = sref.ancillary(dirs, [0.0, 2.0], [0.0, 2.0, 4.0], anc, np.arange(3.0), np.arange(5.0))
    assert out[0, 0] == 2 and out[2, 0] == 2j  # at a centre: that centre's direction, the model's speed
    np.testing.assert_allclose(out[1, 1], 2 * (1 + 1j) / np.sqrt(2), rtol=1e-15)  # the NaN corners' weight is simply dropped
    assert out[0, 1] == 0  # |a| = 0
    np.testing.assert_array_equal(out[:2, 3:], anc[:2, 3:])  # no valid corner: a itself, bit for bit
    assert out[0, 2] == -2 and out[1, 2] == -2  # the only valid corners weigh 0 there: v == 0
    assert np.isnan(out[2, 4].real) and np.isnan(out[2, 4].imag)
    cancel = sref.ancillary(np.array([[1, -1]], dtype=complex), [0.0], [0.0, 2.0], np.full((1, 3), 3j), [0.0], np.arange(3.0))
    assert cancel[0, 1] == 3j and cancel[0, 0] == 3 and cancel[0, 2] == -3  # opposite corners cancel in the middle: a


def test_at_windows_takes_the_nearest_pixel_ties_to_the_larger_coordinate():
    anc = np.arange(12).reshape(3, 4) * (1 + 1j)
    line, sample = np.array([0.0, 10.0, 20.0]), np.array([0.0, 10.0, 20.0, 30.0])
    got = sref.at_windows(anc, line, sample, [5.0, 14.0], [-3.0, 25.0, 100.0])
    np.testing.assert_array_equal(got, anc[np.ix_([1, 1], [0, 3, 3])])
    np.testing.assert_array_equal(gradients.nearest_indexer(line, [5.0, 14.0]), [1, 1])


def test_streak_scene_quadrants_are_recovered():
    thetas = [0.4, -0.9, 1.2, -0.2]
    s0 = ref.streak_scene((320, 320), thetas, np.random.default_rng(5), wavelength=16.0)
    line = sample = np.arange(320) * 10.0
    at = {"line": np.array([800.0, 2400.0]), "sample": np.array([800.0, 2400.0])}
    W, R, _, _ = ref.histogram(s0, line, sample, windows_sizes=(1600,), windows_at=at)
    s = sref.streaks_direction(W, R, BINS)
    assert s["angle"].shape == (2, 2)
    for k, th in enumerate(thetas):
        d = (s["angle"][divmod(k, 2)] - (th + np.pi / 2) + np.pi / 2) % np.pi - np.pi / 2
        assert abs(d) <= STEP + 1e-12, (k, s["angle"][divmod(k, 2)], th)
    # resolved against a wind blowing along +sample, spread over the raster: speed kept, direction within a bin of the streaks
    a_win = np.full((2, 2), 7 + 0j)
    dirs = sref.resolve(s["angle"], s["weight"], s["used_ratio"], a_win)
    assert (dirs.real >= 0).all()
    out = sref.ancillary(dirs, at["line"], at["sample"], np.full((32, 32), 7 + 0j), line[::10], sample[::10])
    np.testing.assert_allclose(np.abs(out), 7.0, rtol=1e-14)
    np.testing.assert_array_equal(out[:9, :9], np.broadcast_to(7 * dirs[0, 0], (9, 9)))


@pytest.mark.parametrize("family", sorted(sc.BUILDERS))
def test_streak_case_builders_hold_what_they_claim(family):
    """Every builder of tests/streak_cases.py runs here, with the assertions it makes on the restatement."""
    built = sc.BUILDERS[family]()
    assert len(built) == {"periodic": 20, "lanes": 22, "counts": 12, "values": 12}[family]
    assert len({c.name for c in built}) == len(built) and set(sc.names()) >= {c.name for c in built}
    for c in built:
        assert not c.weight.flags.writeable and not c.want["index"].flags.writeable and c.want["index"].dtype == np.int32
        assert c.weight.shape[-1] == c.n and 8 <= c.n <= 512
    if family == "periodic":
        assert {(c.n, c.claim["period"]) for c in built} == {(n, p) for n, p, _ in sc.PERIODIC}
        assert {len(c.claim["tied"]) for c in built} == {6, 2, 8, 12}
    if family == "lanes":
        assert {c.n for c in built} == set(sc.LANE_ANGLES)
        assert sc.lane_positions(512) == (0, 63, 64, 511) and sc.lane_positions(360) == (0, 63, 64, 319, 359)
        assert sc.lane_positions(65) == (0, 63, 64) and sc.lane_positions(63) == (0, 62) and sc.lane_positions(129) == (0, 63, 64, 127, 128)
    if family == "counts":
        assert sorted({c.weight.shape[1] * c.weight.shape[2] for c in built}) == [1, 3, 4, 5, 9]
        assert max(c.weight.size for c in sc.cases().values()) == built[-1].weight.size == 3 * 9 * 512


def smooth_in_python(h):
    """circ_smooth of one histogram, element by element in Python floats: the same taps in the same order."""
    x = [float(v) for v in h]
    n = len(x)
    for reach in (1, 2, 4, 8):
        taps = [0.0] * (2 * reach + 1)
        taps[0], taps[reach], taps[-1] = 0.25, 0.5, 0.25
        out = []
        for i in range(n):
            s = 0.0
            for j, b in enumerate(taps):
                s = s + b * x[(i + j - reach) % n]
            out.append(s)
        x = out
    return np.array(x)


def test_circ_smooth_agrees_with_a_loop_in_python_floats_on_the_periodic_cases():
    for c in sc.periodic_cases():
        m0 = sref.nanmean_leading(c.weight, 3)
        for w in range(m0.shape[1]):
            if c.smooth:
                assert bits_equal(smooth_in_python(m0[0, w]), c.want["m"][0, w]), c.name
            else:
                assert bits_equal(m0[0, w], c.want["m"][0, w]), c.name
    h8 = sc.cases()["lanes_n8_smooth"]   # the taps wrap more than once
    assert bits_equal(smooth_in_python(sref.nanmean_leading(h8.weight, 3)[0, 5]), h8.want["m"][0, 5])


@pytest.mark.parametrize("name", sorted(sc.FIELDS))
def test_raster_fields_and_the_longdouble_finish(name):
    """The two designed fields of the raster pass hold what they claim, and numpy's own finish of the restatement stays within
    K = 2h + 2 = 4 ulp of the longdouble finish per component (h = 1: glibc's hypot is within 1 ulp)."""
    f = sc.FIELDS[name]()
    want = sref.ancillary(f.dirs, f.windows_line, f.windows_sample, f.anc, f.line, f.sample)
    ex = sref.ancillary_exact(f.dirs, f.windows_line, f.windows_sample, f.anc, f.line, f.sample)
    assert (ex["nan"] ^ ex["fallback"] ^ ex["blend"]).all()
    np.testing.assert_array_equal(np.isnan(want.real), ex["nan"])
    assert bits_equal(want[ex["fallback"]], f.anc[ex["fallback"]])
    if name == "closed_form":   # |a| times the corners' axis, the other part +0.0, to the bit
        eq = f.claim["equal"]
        assert not (eq & ~ex["blend"]).any()
        assert bits_equal(want[eq], f.claim["expected"][eq])
        assert set(np.abs(f.claim["expected"][eq]) / 7) <= {2.0 ** k for k in range(-20, 21)}
    if sref.LONGDOUBLE_EPS >= 2.0 ** -60:
        pytest.skip("np.longdouble is no wider than float64 here: nothing to compare the ulps against")
    worst, worst_tiny, n_tiny, n = sref.ancillary_ulps(want, ex)
    print(f"{name}: numpy finish worst {worst:.3g} ulp over {n} components, {n_tiny} below the smallest normal")
    assert worst <= 4 and n_tiny == 0 and worst_tiny == 0


def test_public_call_raises_without_gpu():
    if _lib.device_count_safe() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.XswError):
        streaks.streaks_direction(np.zeros((2, 2, 72)), angles=BINS)
    with pytest.raises(_lib.XswError):
        streaks.ancillary_from_streaks(np.ones((2, 2), complex), np.ones((8, 8), complex), windows_line=[1, 5], windows_sample=[1, 5])
