"""xsarsea_amd.gradients without a GPU: the semantics its kernels reproduce, pinned by hand-computed cases on the CPU
restatement (tests/gradients_ref.py), the host geometry of the product against the restatement, and argument validation."""
import numpy as np
import pytest

import gradients_ref as ref
from xsarsea_amd import _lib, gradients

BINS = ref.angles_bins(72)


# ---- rule 1: R2
def test_coarsen_mean_skips_nan():
    a = np.array([[1.0, np.nan, 7.0, 8.0], [3.0, 5.0, 9.0, 10.0], [np.nan, np.nan, 1.0, 1.0], [np.nan, np.nan, 1.0, 1.0]])
    out = ref.coarsen_mean(a)
    assert out[0, 0] == 3.0  # (1 + 3 + 5) / 3: the NaN is skipped, not propagated
    assert out[0, 1] == 8.5
    assert np.isnan(out[1, 0])  # all-NaN block
    assert out[1, 1] == 1.0
    assert ref.coarsen_mean(np.ones((5, 7))).shape == (2, 3)  # boundary="trim"


def test_r2_symm_border_and_unit_normalisation():
    x = np.tile(np.arange(6.0), (6, 1))  # constant along line: B2 acts as [1, 2, 1] / 4 along sample
    out = ref.conv_symm(x, ref.B2)
    assert out[0, 0] == 0.25  # symm: d c b a | a b c d -> (0 + 2*0 + 1) / 4
    assert out[0, 5] == 4.75  # (4 + 2*5 + 5) / 4
    np.testing.assert_array_equal(ref.R2(np.full((9, 11), 2.5)), np.full((4, 5), 2.5))


def test_r2_nan_taps_propagate():
    x = np.ones((16, 16))
    x[8, 8] = np.nan
    out = ref.R2(x)
    # the 5x5 taps spread the NaN over fine rows/cols 6..10; a coarse block is NaN only when all four are (coarse 3..4: fine
    # 10 is NaN, 11 is not, so block 5 skips it); the 3x3 taps spread that over coarse 2..5
    expect = np.zeros((8, 8), bool)
    expect[2:6, 2:6] = True
    np.testing.assert_array_equal(np.isnan(out), expect)


# ---- rule 2: local_gradients
def test_scharr_reflect101_differs_from_symm():
    a = np.tile(np.array([0.0, 1.0, 4.0, 9.0, 16.0]), (5, 1))
    dx, dy = ref.scharr(a)
    assert np.all(dx[:, 0] == 0.0)  # reflect-101: d c b | a b c d -> a[-1] = a[1]; symm would give 16 * (1 - 0)
    assert np.all(dx[:, 1] == 16.0 * (4.0 - 0.0))
    assert np.all(dy == 0.0)
    b = a.copy()
    b[2, 2] = np.nan
    dx, dy = ref.scharr(b)
    assert np.isnan(dx[1:4, 1:4]).all() and np.isnan(dx).sum() == 9  # every tap multiplies, the zero tap included


def test_local_gradients_angle_and_quality():
    y, x = np.mgrid[0:64, 0:64].astype(float)
    th = 0.3
    ampl = 1 + 0.2 * np.sin((x * np.cos(th) + y * np.sin(th)) * 2 * np.pi / 9)
    g2, g3, c = ref.local_gradients(ampl)
    assert g2.shape == (32, 32) and g3.shape == (32, 32)
    inner = np.angle(g2[8:-8, 8:-8])
    assert abs(np.median(inner) - th) < 0.02
    assert (c >= 0).all() and (c <= 1).all()


# ---- rule 3: geometry
def test_rolling_window_even_offset():
    a = np.arange(100.0).reshape(10, 10)
    w4 = ref.rolling_window(a, 5, 5, 4)
    assert w4[0, 0] == a[3, 3] and w4[3, 3] == a[6, 6]  # rows i - w//2 .. i - w//2 + w - 1
    w5 = ref.rolling_window(a, 5, 5, 5)
    assert w5[0, 0] == a[3, 3] and w5[4, 4] == a[7, 7]
    edge = ref.rolling_window(a, 0, 9, 4)
    assert np.isnan(edge[:2]).all() and np.isnan(edge[:, 3]).all() and edge[2, 0] == a[0, 7]


def test_nearest_ties_go_to_the_larger_coordinate():
    index = np.array([0.0, 2.0, 4.0, 6.0])
    target = np.array([1.0, 3.0, 5.0, -1.0, 7.0, 4.0, 2.9, 100.0])
    expect = [1, 2, 3, 0, 3, 2, 1, 3]
    np.testing.assert_array_equal(ref.nearest(index, target), expect)
    np.testing.assert_array_equal(gradients.nearest_indexer(index, target), expect)


def test_geometry_helpers_match_the_restatement():
    rng = np.random.default_rng(3)
    line = np.arange(1203) * 10.0 + 5
    sample = np.arange(1597) * 10.0 + 5
    for f in (1, 2, 3):
        lf = gradients.coarsen_coords(line, f) if f > 1 else line
        sf = gradients.coarsen_coords(sample, f) if f > 1 else sample
        np.testing.assert_array_equal(lf, ref.coarsen_coords(line, f))
        lg_l, lg_s = ref.coarsen_coords(ref.coarsen_coords(lf, 2), 2), ref.coarsen_coords(ref.coarsen_coords(sf, 2), 2)
        for ws in (1600, 3200, 1000):
            assert gradients.window_pixels(ws, lg_l, lg_s) == ref.window_pixels(ws, lg_l, lg_s)
        for _ in range(3):
            t = np.sort(rng.uniform(line[0] - 50, line[-1] + 50, 40))
            t[:5] = lg_l[3:8] + np.diff(lg_l)[0] / 2  # exact ties
            np.testing.assert_array_equal(gradients.nearest_indexer(lg_l, t), ref.nearest(lg_l, t))
    np.testing.assert_array_equal(gradients.angles_bins(72), BINS)


def test_windows_at_from_window_step():
    s0 = np.ones((1203, 1597), np.float32)
    line, sample = np.arange(1203) * 10.0, np.arange(1597) * 10.0
    g = gradients.Gradients2D(s0, window_size=1600, line=line, sample=sample)
    np.testing.assert_array_equal(g.windows_at["line"], line[::160])
    np.testing.assert_array_equal(g.windows_at["sample"], sample[::160])
    g = gradients.Gradients2D(s0, window_size=1600, window_step=0.5, line=line, sample=sample)
    np.testing.assert_array_equal(g.windows_at["sample"], sample[::80])
    assert g.n_angles == 72
    # Gradients: the first (pol, factor, size) fixes the centres of all the others
    G = gradients.Gradients(np.stack([s0, s0]), windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=1, line=line,
                            sample=sample)
    assert len(G.gradients_list) == 8
    for g in G.gradients_list:
        np.testing.assert_array_equal(g.windows_at["line"], line[::160])


def test_window_step_and_windows_at_are_exclusive():
    with pytest.raises(ValueError, match="mutually exclusive"):
        gradients.Gradients2D(np.ones((64, 64)), window_step=1, windows_at={"line": [0], "sample": [0]})


def test_coordinates_come_from_the_container():
    import xr_standin
    line, sample = np.arange(40) * 10.0 + 3, np.arange(48) * 10.0 + 1
    da = xr_standin.DataArray(np.ones((2, 40, 48)), dims=("pol", "line", "sample"),
                              coords={"pol": np.array(["VV", "VH"]), "line": line, "sample": sample})
    G = gradients.Gradients(da, windows_sizes=[160])
    assert list(G.pol) == ["VV", "VH"]
    np.testing.assert_array_equal(G.gradients_list[0].windows_at["line"], line[::16])
    with pytest.raises(ValueError):
        gradients.Gradients2D(np.ones((4, 4, 4)))


# ---- rule 4: gradient_histogram
def test_even_count_median():
    g2 = np.array([[1.0, 2.0], [3.0, 10.0]], complex)
    h, u, _ = ref.gradient_histogram(g2, np.ones((2, 2)), BINS)
    k = int(np.round((0.0 - BINS[0]) / (BINS[1] - BINS[0])))
    assert k == 36
    m = 2.5  # (2 + 3) / 2
    assert h[k] == pytest.approx(1 / (1 + m) + 2 / (2 + m) + 3 / (3 + m) + 10 / (10 + m), rel=1e-15)
    assert h.sum() == h[k] and u == 1.0


def test_round_half_even_at_the_lower_edge():
    # angle(-1j) = -pi/2 puts (angle - start) / step at exactly -0.5: numpy's round gives -0 (bin 0); C's round would give -1,
    # i.e. the last bin through numpy's negative index
    assert (np.angle(-1j) - BINS[0]) / (BINS[1] - BINS[0]) == -0.5
    g2 = np.array([[-1j, 1.0 + 0j]])
    h, u, amb = ref.gradient_histogram(g2, np.ones((1, 2)), BINS)
    assert h[0] == pytest.approx(1 / 2) and h[71] == 0.0
    assert amb > 0  # it sits on a bin edge


def test_bin_72_folds_onto_bin_0():
    # G2 = sqrt(negative real + 0j) = +1j: angle +pi/2 rounds to bin 72, where the reference's np.add.at raises IndexError
    g2 = np.sqrt(np.array([[-4.0 + 0j, -1.0 + 0j]]))
    assert np.angle(g2[0, 0]) == np.pi / 2
    with pytest.raises(IndexError):
        ref.gradient_histogram(g2, np.ones((1, 2)), BINS, fold=False)
    h, u, _ = ref.gradient_histogram(g2, np.ones((1, 2)), BINS)
    assert h[0] == pytest.approx(2 / (2 + 1.5) + 1 / (1 + 1.5)) and u == 1.0


def test_kept_pixels_and_used_ratio():
    g2 = np.array([[np.nan, 0.0, 1.0, 1j]])
    h, u, _ = ref.gradient_histogram(g2, np.array([[1.0, 1.0, 0.5, 0.0]]), BINS)
    assert u == 0.5  # NaN and |g2| == 0 are not kept
    assert h.sum() == pytest.approx(0.5 * 0.5)


# ---- rule 5: resampling
def test_area_mean_trims_and_propagates_nan():
    a = np.arange(35.0).reshape(5, 7)
    a[0, 0] = np.nan
    out = ref.area(a.astype(np.float32), 2)
    assert out.dtype == np.float32 and out.shape == (2, 3)
    assert np.isnan(out[0, 0]) and out[1, 2] == np.float32((18 + 19 + 25 + 26) / 4)
    np.testing.assert_array_equal(gradients.coarsen_coords(np.arange(7.0), 2), [0.5, 2.5, 4.5])


# ---- rule 6: circ_smooth
def test_circ_smooth_is_circular():
    h = np.zeros((3, 72))
    h[0, 0] = 1.0
    h[1, 71] = 1.0
    h[2] = np.random.default_rng(0).random(72)
    s = gradients.circ_smooth(h)
    np.testing.assert_allclose(s, ref.circ_smooth(h), rtol=1e-13, atol=1e-16)
    np.testing.assert_allclose(s[0], np.roll(s[1], 1), rtol=1e-13, atol=1e-16)  # no edge: a shift commutes with it
    assert s.sum() == pytest.approx(h.sum())


def test_streaks_recovered_by_the_restatement():
    rng = np.random.default_rng(5)
    thetas = [0.4, -0.9, 1.2, -0.2]
    s0 = ref.streak_scene((320, 320), thetas, rng, wavelength=16.0)
    line = sample = np.arange(320) * 10.0
    W, R, A, at = ref.histogram(s0, line, sample, windows_sizes=(1600,), window_step=1,
                                windows_at={"line": [800.0, 2400.0], "sample": [800.0, 2400.0]})
    step = BINS[1] - BINS[0]
    for k, th in enumerate(thetas):
        i, j = divmod(k, 2)
        peak = BINS[np.argmax(ref.circ_smooth(W[0, 0, i, j]))]
        d = (peak - th + np.pi / 2) % np.pi - np.pi / 2
        assert abs(d) <= step + 1e-12, (k, peak, th)


def test_histogram_raises_without_gpu():
    if _lib.device_count_safe() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.XswError):
        gradients.Gradients(np.ones((64, 64)), windows_sizes=[16]).histogram
