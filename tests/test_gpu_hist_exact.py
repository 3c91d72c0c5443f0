"""k_grad_hist / k_grad_hist_masked on the MI355X at the windows of tests/hist_cases.py (rule 4).

Group A, the radix-select median: every window holds one lit probe, so its weights and used_ratio are expected to the BIT (the
closed form of hist_cases.py, which tests/test_hist_cases_cpu.py holds to the restatement's gradient_histogram).  Group B, the
sweeps of 72 bins: one kept pixel per bin at 2 .. 360 bins, several windows in one launch, 40 exact probes beyond bin 72, one
random box.  Group C, window geometry: rectangular windows over, on and off every edge of two rasters.
Comparisons that are not of bits use the figures of tests/test_gpu_gradients.py: 1e-9 relative with 1e-15 * sum absolute where the
restatement has no ambiguous pixel, L1 <= 2 * ambiguous + 1e-12 * sum otherwise.  Each prints the largest relative difference
it saw."""
import numpy as np
import pytest

import gradients_ref as ref
import hist_cases as hc
from test_gpu_gradients import assert_close
from util import bits_equal
from xsarsea_amd import gradients
from xsarsea_amd._raster import _Call

pytestmark = pytest.mark.gpu


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(launch, device=False):
    g2, c, keep = (cuda(x) for x in (launch.g2, launch.c, launch.keep)) if device else (launch.g2, launch.c, launch.keep)
    w, r = gradients._hist(g2, c, launch.window, launch.rows, launch.cols, launch.n_angles, normalise=False, keep=keep)
    assert hasattr(w, "is_cuda") == device
    return host(w), host(r)


def differing(launch, w, r):
    """Labels of the windows of a launch whose weights or used_ratio are not the expected bits."""
    assert w.shape == launch.weight.shape and r.shape == launch.ratio.shape
    return [f"{launch.name}: {label}" for j, label in enumerate(launch.labels)
            if not (bits_equal(w[0, j], launch.weight[0, j]) and bits_equal(r[0, j], launch.ratio[0, j]))]


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    m = b != 0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


# --------------------------------------------------------------------------------------------------------------- Group A
@pytest.mark.parametrize("variant", ["plain", "ones", "masked"])
def test_median_bits(variant):
    """Every multiset, every probe: the unmasked kernel on NaN / 0.0 / -0.0 holes, the masked kernel with a keep of all ones on
    the same rasters, and the masked kernel with the holes written as keep = 0 on finite g2."""
    bad, n = [], 0
    for launch in hc.pack(hc.group_a(), variant):
        w, r = run(launch)
        bad += differing(launch, w, r)
        n += len(launch.labels)
    print(f"group A {variant}: {n} windows compared bit for bit, {len(bad)} differ")
    assert not bad, bad[:20]


@pytest.mark.parametrize("variant", ["plain", "masked"])
def test_median_bits_on_device_tensors(variant):
    """One multiset per family through torch CUDA input: the expected bits, and so the numpy route's."""
    placements = [(m, w) for m, w in hc.group_a() if m.name in hc.DEVICE_ROUTE and w[0] > 1]
    assert len(placements) == len(hc.DEVICE_ROUTE)
    bad, n = [], 0
    for launch in hc.pack(placements, variant):
        w, r = run(launch, device=True)
        wn, rn = run(launch)
        assert bits_equal(w, wn) and bits_equal(r, rn), launch.name
        bad += differing(launch, w, r)
        n += len(launch.labels)
    print(f"group A {variant}, device tensors: {n} windows compared bit for bit, {len(bad)} differ")
    assert not bad, bad[:20]


# --------------------------------------------------------------------------------------------------------------- Group B
def close_to_restatement(got, want, label):
    """The existing rule for a window without an ambiguous pixel, per bin."""
    print(f"{label}: largest relative difference {max_rel(got, want):.3g}")
    assert_close(got, want, 1e-9, 1e-15 * want.sum())


@pytest.mark.parametrize("n_angles", hc.SWEEP_ANGLES)
def test_one_pixel_per_bin(n_angles):
    bins = ref.angles_bins(n_angles)
    g2, c = hc.one_per_bin(n_angles)
    want, ratio, amb = ref.gradient_histogram(g2, c, bins)
    assert amb == 0.0
    wl, ws = hc.W_SWEEP
    w, r = gradients._hist(g2, c, hc.W_SWEEP, [wl // 2], [ws // 2], n_angles, bins, normalise=False)
    assert w.shape == (1, 1, n_angles) and r[0, 0] == ratio
    close_to_restatement(w[0, 0], want, f"group B one pixel per bin, {n_angles} bins")
    wk, rk = gradients._hist(g2, c, hc.W_SWEEP, [wl // 2], [ws // 2], n_angles, bins, normalise=False, keep=np.ones(g2.shape, np.uint8))
    assert bits_equal(wk, w) and bits_equal(rk, r)
    if n_angles in (145, 360):
        h, u = gradients.gradient_histogram(g2, c, bins)
        assert bits_equal(h, w[0, 0]) and u == ratio
        wn, rn = gradients._hist(g2, c, hc.W_SWEEP, [wl // 2], [ws // 2], n_angles, bins, normalise=True)
        assert bits_equal(wn, w / float(wl * ws)) and bits_equal(rn, r)   # one IEEE division of the same sums
        close_to_restatement(wn[0, 0], want / (wl * ws), f"group B one pixel per bin, {n_angles} bins, normalised")
        hd, ud = gradients.gradient_histogram(cuda(g2), cuda(c), bins)
        assert bits_equal(host(hd), h) and float(ud) == ratio


@pytest.mark.parametrize("n_angles", hc.PYTH_ANGLES)
def test_several_windows_in_one_launch(n_angles):
    """2 x 3 windows of different contents, one empty: every element against the restatement; then the device route into an output
    that the test filled with a sentinel, with guard elements behind it: every element written, none beyond."""
    import torch
    bins = ref.angles_bins(n_angles)
    g2, c, rows, cols = hc.several_windows(n_angles)
    wl, ws = hc.W_SWEEP
    w, r = gradients._hist(g2, c, hc.W_SWEEP, rows, cols, n_angles, bins, normalise=False)
    assert w.shape == (2, 3, n_angles)
    worst = 0.0
    for a, i in enumerate(rows):
        for b, j in enumerate(cols):
            want, ratio, amb = ref.gradient_histogram(hc.rolling_box(g2, i, j, wl, ws), hc.rolling_box(c, i, j, wl, ws), bins)
            assert amb == 0.0 and r[a, b] == ratio
            assert_close(w[a, b], want, 1e-9, 1e-15 * want.sum())
            worst = max(worst, max_rel(w[a, b], want))
    assert bits_equal(w[1, 1], np.zeros(n_angles)) and r[1, 1] == 0.0
    print(f"group B several windows, {n_angles} bins: 6 windows, largest relative difference {worst:.3g}")
    sentinel, guard = -12345.678, 4 * n_angles
    tg, tc = cuda(g2), cuda(c)
    call = _Call(tg, tc)
    wd = torch.full((6 * n_angles + guard,), sentinel, dtype=torch.float64, device="cuda")
    rd = torch.full((6 + guard,), sentinel, dtype=torch.float64, device="cuda")
    call.launch("grad_hist_raw", g2.shape[0], g2.shape[1], call.mem, call.prep(tg, np.complex128), call.prep(tc, np.float64), wl, ws, 2,
                call.prep(np.asarray(rows, np.int32), np.int32), 3, call.prep(np.asarray(cols, np.int32), np.int32), n_angles,
                bins[0], bins[1] - bins[0], False, wd, rd)
    wd, rd = host(wd), host(rd)
    assert (wd[6 * n_angles:] == sentinel).all() and (rd[6:] == sentinel).all()
    assert bits_equal(wd[:6 * n_angles].reshape(2, 3, n_angles), w) and bits_equal(rd[:6].reshape(2, 3), r)


@pytest.mark.parametrize("n_angles", hc.PYTH_ANGLES)
def test_exact_probes_beyond_bin_72(n_angles):
    """40 Pythagorean probes (their moduli exact) lit at once in one window of 1400 kept pixels, each alone in its bin: the
    bits of the closed form in every sweep."""
    bins = ref.angles_bins(n_angles)
    g2, c = hc.pythagorean_window()
    want, ratio = hc.closed_form(g2, c, bins)
    wl, ws = hc.W_MAIN
    for keep in (None, np.ones(g2.shape, np.uint8)):
        w, r = gradients._hist(g2, c, hc.W_MAIN, [wl // 2], [ws // 2], n_angles, bins, normalise=False, keep=keep)
        diff = np.flatnonzero(w[0, 0].view(np.uint64) != want.view(np.uint64))
        print(f"group B exact probes, {n_angles} bins, {'unmasked' if keep is None else 'masked'}: 1 window, 40 occupied bins, "
              f"{len(diff)} bins differ, largest relative difference {max_rel(w[0, 0], want):.3g}")
        assert r[0, 0] == ratio
        assert len(diff) == 0, [(int(k), float(w[0, 0, k]), float(want[k])) for k in diff[:8]]


@pytest.mark.parametrize("n_angles", [90, 145])
def test_random_box(n_angles):
    bins = ref.angles_bins(n_angles)
    g2, c = hc.random_box()
    h, u = gradients.gradient_histogram(g2, c, bins)
    hr, ur, amb = ref.gradient_histogram(g2, c, bins)
    print(f"group B random box, {n_angles} bins: L1 difference {np.abs(h - hr).sum():.3g}, ambiguous weight {amb:.3g}, "
          f"largest relative difference {max_rel(h, hr):.3g}")
    assert u == ur
    assert np.abs(h - hr).sum() <= 2 * amb + 1e-12 * hr.sum()


# --------------------------------------------------------------------------------------------------------------- Group C
@pytest.mark.parametrize("shape", hc.GEOMETRY_RASTERS)
def test_window_geometry_bits(shape):
    """g2 real and positive, c lit at ONE raster pixel: whatever a window clips, it holds that probe or nothing, so its weights
    (through the median of exactly the pixels it covers) and its used_ratio are expected to the bit.  Both kernels."""
    L, S = shape
    n, bad = 0, []
    for wl, ws in hc.GEOMETRY_WINDOWS:
        rows, cols = hc.geometry_centres(L, wl), hc.geometry_centres(S, ws)
        for lit in hc.geometry_lit(shape):
            g2, c = hc.geometry_raster(shape, lit, "probe")
            want, ratio = hc.geometry_expected(g2, c, (wl, ws), rows, cols)
            w, r = gradients._hist(g2, c, (wl, ws), rows, cols, hc.N_ANGLES, normalise=False)
            wk, rk = gradients._hist(g2, c, (wl, ws), rows, cols, hc.N_ANGLES, normalise=False, keep=np.ones(shape, np.uint8))
            assert bits_equal(wk, w) and bits_equal(rk, r)
            for a, i in enumerate(rows):
                for b, j in enumerate(cols):
                    n += 1
                    if not (bits_equal(w[a, b], want[a, b]) and r[a, b] == ratio[a, b]):
                        bad.append(((wl, ws), lit, i, j))
    print(f"group C {L} x {S}, lit probes: {n} windows compared bit for bit, {len(bad)} differ")
    assert not bad, bad[:20]


@pytest.mark.parametrize("shape", hc.GEOMETRY_RASTERS)
def test_window_geometry_random(shape):
    """Random principal roots and a random c: used_ratio exact, weights per bin by the existing rule (no window has an ambiguous
    pixel: the CPU test holds that)."""
    L, S = shape
    bins = ref.angles_bins(hc.N_ANGLES)
    g2, c = hc.geometry_raster(shape, None, "random")
    n, worst = 0, 0.0
    for wl, ws in hc.GEOMETRY_WINDOWS:
        rows, cols = hc.geometry_centres(L, wl), hc.geometry_centres(S, ws)
        w, r = gradients._hist(g2, c, (wl, ws), rows, cols, hc.N_ANGLES, normalise=False)
        for a, i in enumerate(rows):
            for b, j in enumerate(cols):
                want, ratio, amb = ref.gradient_histogram(hc.rolling_box(g2, i, j, wl, ws), hc.rolling_box(c, i, j, wl, ws), bins)
                assert amb == 0.0 and r[a, b] == ratio, ((wl, ws), i, j)
                assert_close(w[a, b], want, 1e-9, 1e-15 * want.sum())
                worst = max(worst, max_rel(w[a, b], want))
                n += 1
    print(f"group C {L} x {S}, random: {n} windows, largest relative difference {worst:.3g}")
