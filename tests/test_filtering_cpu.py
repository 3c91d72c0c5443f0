"""CPU: the restatement tests/filtering_ref.py against scipy itself, the host-side pieces of
xsarsea_amd.gradients.filtering_parameters, and the conditions that keep the GPU comparison honest, asserted on the restatement
alone for every scene tests/test_gpu_filtering.py uses and every case of tests/filter_cases.py (the seam shapes and in-ramp inputs
of tests/test_gpu_filter_seams.py), with four wrong halos that the comparison there has to be able to see."""
import numpy as np
import pytest
from scipy import ndimage, signal

import filter_cases as fc
import filtering_ref as fr
from xsarsea_amd import gradients
from xsarsea_amd.gradients import FilteringParameters, Mean, filtering_parameters, smoothing  # noqa: F401  (the feature's names)


@pytest.mark.parametrize("shapes", [((7, 9), (15, 19)), ((50, 79), (100, 159)), ((51, 80), (103, 160)), ((8, 8), (16, 17)),
                                    ((1, 3), (2, 7)), ((1, 1), (3, 2)), ((2, 2), (4, 5))])
def test_zoom_linear_is_scipy_zoom(shapes):
    n_in, n_out = shapes
    a = np.random.default_rng(1).normal(size=n_in)
    if a.size > 20:
        a[n_in[0] // 2, n_in[1] // 2] = np.nan
        a[-2, -1] = np.nan  # reached by the mirrored zero-weight tap of the last output row
    z = ndimage.zoom(a, (n_out[0] / n_in[0], n_out[1] / n_in[1]), order=1)
    mine = fr.zoom_linear(a, n_out)
    assert z.shape == tuple(n_out) == mine.shape
    np.testing.assert_array_equal(np.isnan(mine), np.isnan(z))
    m = ~np.isnan(z)
    assert (np.abs(mine[m] - z[m]) <= 1e-15 * np.abs(z[m])).all()


def test_zoom_zero_weight_taps_multiply():
    """One NaN in a 7 x 9 input zoomed to 15 x 19 gives 25 NaN outputs: the exact-integer coordinates, whose second tap has
    weight 0, are among them.  The second tap of the last output is the mirrored element n - 2."""
    a = np.ones((7, 9))
    a[3, 4] = np.nan
    for z in (ndimage.zoom(a, (15 / 7, 19 / 9), order=1), fr.zoom_linear(a, (15, 19))):
        assert np.isnan(z).sum() == 25
        assert np.isnan(z[7, 9])  # coordinate (3.0, 4.0): the NaN is the first tap; (3.0, .) rows also reach row 4 with weight 0
    b = np.ones((7, 9))
    b[5, 3] = np.nan
    for z in (ndimage.zoom(b, (15 / 7, 19 / 9), order=1), fr.zoom_linear(b, (15, 19))):
        assert np.isnan(z[14]).any()  # the last row reads row 6 (weight 1) and the mirrored row 5 (weight 0)


def test_zoom_last_coordinate_is_exact():
    """o * ((n_in - 1) / (n_out - 1)) at the last output is exactly n_in - 1 for every axis length up to 20000 and both
    parities of the half-resolution axis: the 'outside the array' branch (cval 0) never runs there."""
    n_in = np.arange(1, 20001, dtype=np.float64)
    for n_out in (2 * n_in, 2 * n_in + 1):
        assert ((n_out - 1) * ((n_in - 1) / (n_out - 1)) == n_in - 1).all()


def test_zoom_linear_on_a_crop_at_global_coordinates():
    a = np.random.default_rng(2).normal(size=(60, 70))
    full = fr.zoom_linear(a, (121, 140))
    rows, cols = np.arange(40, 81), np.arange(100, 140)
    crop = fr.zoom_linear(a[15:45, 45:], (121, 140), rows, cols, origin=(15, 45), in_shape=a.shape)
    np.testing.assert_array_equal(crop, full[40:81, 100:140])


def test_kernels_are_dyadic_and_sum_to_one():
    assert fr.B42.shape == (9, 9) and (fr.B42 != 0).sum() == 25
    np.testing.assert_array_equal(fr.B42[::2, ::2], fr.B4)  # B4 dilated by 2
    for k in (fr.B4, fr.B42):
        np.testing.assert_array_equal(k * 256, np.round(k * 256))
        assert k.sum() == 1.0
    # the divisions of Mean and smoothing are by exactly 1.0
    ones = np.ones((11, 13))
    for k in (fr.B2, fr.B4):
        assert (signal.convolve2d(ones, k, mode="same", boundary="symm") == 1.0).all()


def test_b42_nan_footprint_is_9x9():
    x = np.ones((31, 33))
    x[15, 16] = np.nan
    second = signal.convolve2d(x, fr.B42, mode="same", boundary="symm")
    assert np.isnan(second).sum() == 81 and np.isnan(second[11:20, 12:21]).all()
    assert np.isnan(fr.Mean(x)).sum() == 13 * 13  # B4 widens the NaN to 5 x 5 first
    y = np.ones((31, 33))
    y[15, 16] = np.inf
    assert np.isnan(signal.convolve2d(y, fr.B42, mode="same", boundary="symm")).sum() == 81 - 25  # 0 * inf on the zero taps


def test_result_container_and_coords():
    line, sample = np.arange(203) * 10.0 + 5, np.arange(317) * 10.0 + 5
    np.testing.assert_array_equal(gradients.coarsen_coords(line, 2), fr.coarsen_coords(line, 2))
    f = [np.full((101, 158), v) for v in (0.1, 0.2, 0.3, 0.4, 0.5)]
    r = FilteringParameters(*f, gradients.coarsen_coords(line, 2), gradients.coarsen_coords(sample, 2))
    f1, f2, f3, f4, F = r
    assert f1 is f[0] and F is f[4] and r.F is f[4] and len(r) == 5
    assert r.line.shape == (101,) and r.line[0] == 10.0 and r.sample.shape == (158,) and r.sample[-1] == np.mean(sample[314:316])
    for name in ("filtering_parameters", "Mean", "smoothing"):
        assert name in gradients.__all__


def test_smallest_raster_scipy_accepts():
    """A 4-pixel axis gives an r2 axis of 2 and a one-element quarter-resolution axis, which scipy's convolve2d and zoom accept
    (the zoom is then constant along that axis).  Below 4 the quarter-resolution raster is empty and the reference's zoom factor
    r2.shape / resampl.shape divides by zero; the port raises ValueError there, before any device call."""
    rng = np.random.default_rng(3)
    for shape in ((4, 4), (4, 9), (5, 7), (7, 4)):
        out = fr.filtering_parameters(0.1 + rng.uniform(0, 0.01, shape))
        assert out[4].shape == (shape[0] // 2, shape[1] // 2) and np.isfinite(out[4]).all()
    for shape in ((3, 8), (8, 3), (2, 2)):
        with pytest.raises(ZeroDivisionError):
            fr.filtering_parameters(np.full(shape, 0.1))
        with pytest.raises(ValueError, match="4 x 4"):
            filtering_parameters(np.full(shape, 0.1))


@pytest.mark.parametrize("spec", fr.GPU_SCENES + [fr.FULL_TILE], ids=lambda s: f"{s[0][0]}x{s[0][1]}-{np.dtype(s[1]).name}-g{s[3]}")
def test_scene_conditions(spec):
    """Ill-conditioned pixels (d <= 1e-9 J1) <= 0.1 % of the finite ones; at least 5 % of the finite pixels of every f_i inside
    its ramp; at least 80 % of the outputs finite."""
    shape, dtype, seed, gamma = spec
    out = fr.filtering_parameters(fr.full_tile() if spec == fr.FULL_TILE else fr.rain_scene(shape, dtype, seed, gamma))
    ill, min_ramp, finite, ramps = fr.conditions(*out)
    print(f"{spec}: ill-conditioned {ill:.2e}, d < 0: {int((out[5] < 0).sum())}, ramps {[round(float(r), 3) for r in ramps]}, "
          f"finite {finite:.3f}")
    assert ill <= 1e-3
    assert min_ramp >= 0.05
    assert finite >= 0.8


# ------------------------------------------------------------------------------------- the seam cases of tests/filter_cases.py
def test_filter_cases_conditions():
    """Builds every case of tests/filter_cases.py: each asserts on the restatement the property it is there for (designed inputs
    inside the ramps on >= 99 % of the pixels and no ill-conditioned pixel, >= 16 seam pixels inside every ramp of a chain scene,
    every valid-count of the 2 x 2 mean, NaN where the NaN variants want it and at least half of every field finite)."""
    fc.check_all()
    seam = fc.seam_mask((70, 40))
    assert seam[31].all() and seam[32].all() and seam[:, 5].all() and seam[:, 34].all() and seam[64].all() and seam[69].all()
    assert not seam[6:31, 6:31].any() and not seam[33:63, 6:31].any() and not seam[33, 33] and seam.sum() == 70 * 40 - (25 + 30) * (25 + 1)


def mean_by_tiles(x):
    """Wrong halo (a): every 32 x 32 tile reflects at its own edge."""
    out = np.empty_like(x)
    for y in range(0, x.shape[0], fc.TILE):
        for xx in range(0, x.shape[1], fc.TILE):
            out[y:y + fc.TILE, xx:xx + fc.TILE] = fr.Mean(x[y:y + fc.TILE, xx:xx + fc.TILE])
    return out


def mean_shifted_column(x):
    """Wrong halo (b): the output column 31 mod 32 comes from the input rolled by one column."""
    out = fr.Mean(x)
    out[:, fc.TILE - 1::fc.TILE] = fr.Mean(np.roll(x, 1, axis=1))[:, fc.TILE - 1::fc.TILE]
    return out


def mean_reflect_101(x):
    """Wrong halo (c): both convolutions with the reflect-101 border (numpy's "reflect") instead of "symm"."""
    a = signal.convolve2d(np.pad(x, 2, mode="reflect"), fr.B4, mode="valid")
    return signal.convolve2d(np.pad(a, 4, mode="reflect"), fr.B42, mode="valid")


def zoom_wrong_factor(q4, out_shape):
    """Wrong zoom (d): the output o reads the coordinate o * n_in / n_out instead of o * (n_in - 1) / (n_out - 1)."""
    taps = []
    for n_in, n_out in zip(q4.shape, out_shape):
        cc = np.arange(n_out) * (n_in / n_out)
        i0 = np.floor(cc).astype(np.int64)
        taps.append((np.minimum(i0, n_in - 1), np.minimum(i0 + 1, n_in - 1), cc - i0))
    (y0, y1, ty), (x0, x1, tx) = taps
    ty = ty[:, None]
    return (q4[np.ix_(y0, x0)] * (1 - ty) + q4[np.ix_(y1, x0)] * ty) * (1 - tx) + (q4[np.ix_(y0, x1)] * (1 - ty) + q4[np.ix_(y1, x1)] * ty) * tx


WRONG = {"tiles": mean_by_tiles, "column": mean_shifted_column, "reflect101": mean_reflect_101, "zoom": zoom_wrong_factor}


def test_wrong_halo_variants_are_wrong_only_where_they_should_be():
    """The variants themselves: equal to Mean away from the seam they break, the right zoom at the first output."""
    x = fc.mean_input((63, 65))
    right = fr.Mean(x)
    np.testing.assert_allclose(mean_by_tiles(x)[6:26, 6:26], right[6:26, 6:26], rtol=1e-13)
    assert not np.isclose(mean_by_tiles(x)[28:36], right[28:36], rtol=1e-6).all()
    np.testing.assert_array_equal(mean_shifted_column(x)[:, :31], right[:, :31])
    np.testing.assert_allclose(mean_reflect_101(x)[6:-6, 6:-6], right[6:-6, 6:-6], rtol=1e-13)
    assert np.abs(mean_reflect_101(x)[0] / right[0] - 1).max() > 1e-6
    q4 = fc.designed((63, 65), "B", 1)["q4"]
    assert zoom_wrong_factor(q4, (63, 65))[0, 0] == q4[0, 0]
    np.testing.assert_allclose(mean_reflect_101(np.ones((2, 9))), 1.0, rtol=1e-15)  # an axis shorter than the reach still pads


def applicable(grid, variant):
    """(a) needs an interior seam, (b) a column 31; (c) and (d) only the raster's edge."""
    return {"tiles": max(grid) > fc.TILE, "column": grid[1] >= fc.TILE}.get(variant, True)


@pytest.mark.parametrize("grid,variant", [(g, v) for g in fc.RAW_GRIDS if max(g) > 6 for v in sorted(WRONG) if applicable(g, v)],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_the_comparison_can_fail(grid, variant):
    """A wrong halo in Mean (set A, f1) or a wrong zoom factor (set B, f2) moves the restatement's own filter by more than
    1e3 ATOL = 1e-6 on at least one seam pixel strictly inside the ramp: the comparison of tests/test_gpu_filter_seams.py at
    ATOL = 1e-9 would fail on a kernel with that fault."""
    for phase in fc.PHASES:
        which, k = ("B", 1) if variant == "zoom" else ("A", 0)
        t = fc.designed(grid, which, phase)
        right = fc.designed_want(grid, which, phase)[k]
        if variant == "zoom":
            wrong = fc.combine_with(t, Z=zoom_wrong_factor(t["q4"], grid))[k]
        else:
            wrong = fc.combine_with(t, mean=WRONG[variant])[k]
        hit = fc.seam_mask(grid) & fc.inside(right) & (np.abs(wrong - right) > 1e-6)
        print(f"{grid} {variant} phase {phase:+d}: {int(hit.sum())} seam pixels moved, by up to {np.abs(wrong - right)[fc.inside(right)].max():.3g}")
        assert hit.any()
