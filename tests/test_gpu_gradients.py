"""xsarsea_amd.gradients on the MI355X against the CPU restatement (tests/gradients_ref.py): R2, local_gradients and the
resampling per pixel, Gradients(...).histogram per window, determinism, streak recovery, device tensors on a user stream,
(pol, line, sample) input and one full-size 20000 x 20000 raster."""
import numpy as np
import pytest

import gradients_ref as ref
from xsarsea_amd import gradients

pytestmark = pytest.mark.gpu
BINS = ref.angles_bins(72)


def scene(shape, dtype, seed, land=True):
    """Speckled sigma0 with some structure and NaN land patches (a rectangle at an edge, a disc inside)."""
    rng = np.random.default_rng(seed)
    L, S = shape
    y, x = np.mgrid[0:L, 0:S].astype(np.float64)
    s0 = 0.05 * (1.2 + np.sin(x / 23.0 + 0.4 * np.cos(y / 41.0)) * np.cos(y / 17.0)) * rng.gamma(20, 1 / 20, shape)
    if land:
        s0[: L // 5, S - S // 6:] = np.nan
        s0[(y - 0.6 * L) ** 2 + (x - 0.3 * S) ** 2 < (0.08 * min(L, S)) ** 2] = np.nan
        s0[L // 2, S // 3] = np.nan
    return s0.astype(dtype)


def assert_close(a, b, rtol, atol=0.0):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    err = np.abs(a[m] - b[m])
    tol = rtol * np.abs(b[m]) + (atol[m] if np.ndim(atol) else atol)
    assert (err <= tol).all(), f"max excess {np.max(err - tol):.3g}, max err {err.max():.3g}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(203, 317), (64, 65)])
def test_r2_and_ampl(dtype, shape):
    s0 = scene(shape, dtype, 1)
    r = ref.R2(s0)
    assert_close(gradients.R2(s0), r, 1e-12)
    assert_close(gradients._r2(s0, True), np.sqrt(r), 1e-12)


def assert_local_close(G2, G3, C, g2, g3, c):
    """(G2, G3, c) of the device against the restatement's.  R2(grad**2) sums signed values: the scale of an error is the magnitude
    of what was summed, G3; G2 is its square root, whose error grows where |R2(grad**2)| << G3, so G2 is compared through its
    square and, where c is not tiny, its angle."""
    scale = 1e-12 * np.nan_to_num(g3)
    assert_close((G2 ** 2).real, (g2 ** 2).real, 1e-12, scale)
    assert_close((G2 ** 2).imag, (g2 ** 2).imag, 1e-12, scale)
    np.testing.assert_array_equal(np.isnan(G2.real), np.isnan(g2.real))
    m = c > 1e-6
    if m.any():
        d = np.angle(G2[m]) - np.angle(g2[m])
        assert np.abs((d + np.pi / 2) % np.pi - np.pi / 2).max() < 1e-9  # modulo pi: +-pi/2 is one direction
    assert_close(G3, g3, 1e-12)
    assert_close(C, c, 1e-12, 1e-12)


@pytest.mark.parametrize("shape", [(203, 317), (66, 31)])
def test_local_gradients(shape):
    ampl = np.sqrt(ref.R2(scene((2 * shape[0] + 1, 2 * shape[1]), np.float64, 2)))
    g2, g3, c = ref.local_gradients(ampl)
    lg = gradients.local_gradients(ampl)
    assert (c > 1e-6).any()
    assert_local_close(lg.G2, lg.G3, lg.c, g2, g3, c)
    np.testing.assert_array_equal(lg.line, ref.coarsen_coords(np.arange(ampl.shape[0]), 2))


# fine shapes whose coarse grids lie on the seams of the 16 x 16 tiles of k_grad_r2 / k_grad_local or are thinner than a tile's
# halo: coarse 1 x 1, 1 x 350 and 350 x 1 (thin strips across 22 tiles), 15 (16k - 1: the reflected halo source is the tile's
# last real row), 17 and 33 (16k + 1: the last tile holds one row and the halo cells past it are clamped), 16 x 1 and 2 x 33
THIN_SHAPES = [(2, 2), (2, 3), (3, 2), (3, 3), (2, 700), (700, 3), (30, 31), (34, 35), (66, 67), (33, 2), (4, 66)]
THIN_CASES = [(s, False) for s in THIN_SHAPES] + [((34, 35), True), ((66, 67), True)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,nan_edges", THIN_CASES, ids=lambda v: "nan_edges" if v is True else "" if v is False else f"{v[0]}x{v[1]}")
def test_tile_kernels_on_seams_and_thin_rasters(shape, nan_edges, dtype):
    """R2, sqrt(R2), local_gradients and the two raw entry points that root sigma0 on load (xsw_grad_r2_sqrt,
    xsw_grad_local_sqrt) against the restatement at this file's tolerances (1e-12; G2 through its square and its angle), on
    rasters of one tile or less, of one coarse row or column across many tiles, and with a coarse axis of 16k - 1 and 16k + 1.
    nan_edges: NaN at the four corners and once on each edge, so that the reflected halos carry NaN; the NaN positions must be
    the restatement's.  No +-inf: the restatement convolves grad**2 as complex numbers and the kernel as two real planes, which
    differ on inf * 0, and an infinite sigma0 is no input this module defines."""
    from xsarsea_amd._raster import _Call
    L, S = shape
    s0 = scene(shape, dtype, 14 + L + S, land=False)
    if nan_edges:
        for y, x in ((0, 0), (0, S - 1), (L - 1, 0), (L - 1, S - 1), (0, S // 2), (L - 1, S // 3), (L // 2, 0), (L // 3, S - 1)):
            s0[y, x] = np.nan
    assert np.isnan(s0).sum() == (8 if nan_edges else 0) and not np.isinf(s0).any()
    r = ref.R2(s0)
    assert r.shape == (L // 2, S // 2) and np.isfinite(r).any()
    assert_close(gradients.R2(s0), r, 1e-12)
    assert_close(gradients._r2(s0, True), np.sqrt(r), 1e-12)
    root = np.sqrt(s0)                                                    # in the input's dtype, widened afterwards
    assert root.dtype == dtype
    ampl = root.astype(np.float64)
    g2, g3, c = ref.local_gradients(ampl)
    lg = gradients.local_gradients(ampl)
    assert_local_close(lg.G2, lg.G3, lg.c, g2, g3, c)
    call = _Call(s0)
    x = call.prep(s0)
    r2_sq, G3, C = (call.empty(r.shape, np.float64) for _ in range(3))
    G2 = call.empty(r.shape, np.complex128)
    call.launch("grad_r2_sqrt_raw", L, S, call.xsw_dtype(x), call.mem, x, r2_sq)
    call.launch("grad_local_sqrt_raw", L, S, call.xsw_dtype(x), call.mem, x, G2, G3, C)
    assert_close(r2_sq, ref.R2(ampl), 1e-12)
    assert_local_close(G2, G3, C, g2, g3, c)
    if nan_edges:
        assert np.isnan(r).any() and np.isnan(g3).any() and np.isfinite(g3).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("factor", [2, 3])
def test_area(dtype, factor):
    s0 = scene((203, 317), dtype, 3)
    out = gradients._area(s0, factor)
    assert out.dtype == dtype
    np.testing.assert_array_equal(out, ref.area(s0, factor))  # same float64 order, same rounding


def compare_histograms(h, W, R, A, label):
    """Per window: weights to 1e-9 relative where no pixel is ambiguous; else equal totals and an L1 difference of at most twice
    the ambiguous weight.  used_ratio exact."""
    np.testing.assert_array_equal(np.asarray(h.used_ratio), R)
    w = np.asarray(h.weight)
    assert w.shape == W.shape
    n_amb = 0
    for idx in np.ndindex(*W.shape[:-1]):
        a, b = w[idx], W[idx]
        if A[idx] == 0:
            assert_close(a, b, 1e-9, 1e-15 * b.sum())
        else:
            n_amb += 1
            assert a.sum() == pytest.approx(b.sum(), rel=1e-9, abs=1e-300)
            assert np.abs(a - b).sum() <= 2 * A[idx] * (1 + 1e-9) + 1e-12 * b.sum()
    print(f"{label}: {int(np.prod(W.shape[:-1]))} windows, {n_amb} with an ambiguous pixel")
    return n_amb


LINE = np.arange(1203) * 10.0 + 5
SAMPLE = np.arange(1597) * 10.0 + 5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("step", [1, 0.5])
def test_histogram_matches_the_restatement(dtype, step):
    s0 = scene((1203, 1597), dtype, 4)
    h = gradients.Gradients(s0, windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=step, line=LINE,
                            sample=SAMPLE).histogram
    W, R, A, at = ref.histogram(s0, LINE, SAMPLE, windows_sizes=(1600, 3200), downscales_factors=(1, 2), window_step=step)
    assert h.dims == ("downscale_factor", "window_size", "line", "sample", "angles") and h.pol is None
    np.testing.assert_array_equal(h.line, at["line"])
    np.testing.assert_array_equal(h.sample, at["sample"])
    np.testing.assert_array_equal(h.angles, BINS)
    assert list(h.window_size) == [1600, 3200] and list(h.downscale_factor) == [1, 2]
    assert (R > 0).any() and (R < 1).any() and (R == 0).any()  # full, partial (land, edges) and empty windows all occur
    compare_histograms(h, W, R, A, f"{np.dtype(dtype).name} step {step}")


def test_histogram_user_windows_at():
    s0 = scene((1203, 1597), np.float32, 5)
    at = {"line": np.array([-300.0, 37.5, 4005.0, 6000.0, 12025.0, 20000.0]), "sample": np.array([0.0, 805.0, 7990.0, 15975.0])}
    g = gradients.Gradients2D(s0, window_size=1600, windows_at=at, line=LINE, sample=SAMPLE)
    h = g.histogram
    W, R, A, _ = ref.histogram(s0, LINE, SAMPLE, windows_sizes=(1600,), windows_at=at)
    np.testing.assert_array_equal(h.line, at["line"])
    assert h.dims == ("line", "sample", "angles")

    class H:
        weight, used_ratio = np.asarray(h.weight)[None, None], np.asarray(h.used_ratio)[None, None]
    compare_histograms(H, W, R, A, "windows_at")


def test_gradient_histogram_one_box():
    rng = np.random.default_rng(6)
    g2 = np.sqrt(rng.normal(size=(37, 53)) + 1j * rng.normal(size=(37, 53)))  # a principal root, as G2 is
    g2[3, :7] = np.nan
    g2[5, 5] = 0
    g2[6, 6] = np.sqrt(-3 + 0j)  # angle +pi/2: bin 72, folded onto bin 0
    c = rng.uniform(0, 1, g2.shape)
    h, u = gradients.gradient_histogram(g2, c, BINS)
    hr, ur, amb = ref.gradient_histogram(g2, c, BINS)
    assert u == ur
    assert np.abs(h - hr).sum() <= 2 * amb + 1e-12 * hr.sum()


def test_deterministic():
    import torch
    t = torch.from_numpy(scene((1203, 1597), np.float32, 7)).cuda()
    kw = dict(windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=0.5, line=LINE, sample=SAMPLE)
    a = gradients.Gradients(t, **kw).histogram
    b = gradients.Gradients(t, **kw).histogram
    assert torch.equal(a.weight, b.weight) and torch.equal(a.used_ratio, b.used_ratio)
    assert a.weight.is_cuda and a.weight.dtype == torch.float64


def test_streak_recovery():
    """Stripes at known angles in the four quadrants of one scene: the peak of circ_smooth lands within one bin of each."""
    import torch
    thetas = [0.35, -1.0, 1.3, -0.15]
    s0 = ref.streak_scene((1280, 1280), thetas, np.random.default_rng(8), wavelength=16.0, speckle=0.1)
    line = sample = np.arange(1280) * 10.0
    at = {"line": np.array([3200.0, 9600.0]), "sample": np.array([3200.0, 9600.0])}
    g = gradients.Gradients2D(torch.from_numpy(s0).cuda(), window_size=4800, windows_at=at, line=line, sample=sample)
    smooth = gradients.circ_smooth(g.histogram.weight).cpu().numpy()
    step = BINS[1] - BINS[0]
    for k, th in enumerate(thetas):
        i, j = divmod(k, 2)
        peak = BINS[np.argmax(smooth[i, j])]
        d = (peak - th + np.pi / 2) % np.pi - np.pi / 2
        assert abs(d) <= step + 1e-12, (k, peak, th)


def test_device_tensors_on_a_user_stream_and_pol():
    import torch
    s0 = np.stack([scene((603, 797), np.float32, 9), scene((603, 797), np.float32, 10)])
    line, sample = LINE[:603], SAMPLE[:797]
    kw = dict(windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=0.5, line=line, sample=sample)
    host = gradients.Gradients(s0, **kw).histogram
    assert host.dims[0] == "pol" and list(host.pol) == [0, 1] and host.weight.shape[:3] == (2, 2, 2)
    assert isinstance(host.weight, np.ndarray)
    for p in range(2):
        one = gradients.Gradients(s0[p], **kw).histogram
        np.testing.assert_array_equal(host.weight[p], one.weight)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(s0).cuda()  # produced on the user stream, consumed there without any synchronisation
        dev = gradients.Gradients(t, **kw).histogram
        w, r = dev.weight.cpu().numpy(), dev.used_ratio.cpu().numpy()
    np.testing.assert_array_equal(w, host.weight)
    np.testing.assert_array_equal(r, host.used_ratio)


def test_full_size():
    """One 20000 x 20000 float32 raster (streaks, speckle, NaN land), default coordinates and window: windows compared with the
    restatement run on their footprints (with a 64-pixel halo, or the raster's edge)."""
    import torch
    N = 20000
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(11)
    y = torch.arange(N, device=dev, dtype=torch.float32)[:, None]
    x = torch.arange(N, device=dev, dtype=torch.float32)[None, :]
    th = torch.where(y < N / 2, 0.5, -0.8) + torch.where(x < N / 2, 0.0, 0.6)
    t = 0.08 * (1 + 0.3 * torch.sin((x * torch.cos(th) + y * torch.sin(th)) * (2 * np.pi / 24)))
    t *= 1 + 0.2 * torch.randn((N, N), generator=g, device=dev)
    t[:3000, 15000:] = float("nan")
    t[((y - 12000) ** 2 + (x - 5000) ** 2) < 1500 ** 2] = float("nan")
    del th
    h = gradients.Gradients(t, windows_sizes=[1600]).histogram
    w, r = h.weight.cpu().numpy()[0, 0], h.used_ratio.cpu().numpy()[0, 0]
    assert w.shape == (13, 13, 72)
    lgl = ref.coarsen_coords(ref.coarsen_coords(np.arange(N), 2), 2)
    rows, cols = ref.nearest(lgl, np.arange(N)[::1600]), ref.nearest(lgl, np.arange(N)[::1600])
    wpx = ref.window_pixels(1600, lgl, lgl)
    assert wpx == 400
    n_amb = 0
    for i, j in [(0, 0), (0, 12), (12, 12), (6, 6), (7, 3), (1, 10)]:
        r0, c0 = rows[i] - wpx // 2, cols[j] - wpx // 2
        a, b = max(0, 4 * r0 - 64), min(N, 4 * (r0 + wpx) + 64)
        cc, d = max(0, 4 * c0 - 64), min(N, 4 * (c0 + wpx) + 64)
        crop = t[a:b, cc:d].cpu().numpy()
        g2, c, *_ = ref.lg_of(crop, np.arange(a, b), np.arange(cc, d))
        hw, u, amb = ref.gradient_histogram(ref.rolling_window(g2, rows[i] - a // 4, cols[j] - cc // 4, wpx),
                                            ref.rolling_window(c, rows[i] - a // 4, cols[j] - cc // 4, wpx), BINS)
        assert r[i, j] == u
        hw, amb = hw / wpx ** 2, amb / wpx ** 2
        if amb == 0:
            assert_close(w[i, j], hw, 1e-9, 1e-15 * hw.sum())
        else:
            n_amb += 1
            assert np.abs(w[i, j] - hw).sum() <= 2 * amb * (1 + 1e-9) + 1e-12 * hw.sum()
    print(f"full size: 6 windows compared, {n_amb} with an ambiguous pixel")


@pytest.mark.parametrize("device", [False, True])
def test_bin_72_fold_and_lower_edge_on_the_device(device):
    """The deliberate deviation, pinned exactly.  sqrt(negative + 0j) = +2j has angle +pi/2, which rounds to bin 72 (the
    reference raises IndexError); -2j has angle -pi/2, (angle - start) / step == -0.5, which rounds half to even to bin 0.  Both
    sides compute those quotients with the same IEEE operations, so every kept pixel must land in bin 0: equal |g2| make
    m = 2, r = 0.5 and the sum exact."""
    import torch
    g2 = np.sqrt(np.full((9, 13), -4.0 + 0j))
    assert np.angle(g2[0, 0]) == np.pi / 2 and round((np.pi / 2 - BINS[0]) / (BINS[1] - BINS[0])) == 72
    g2[::2] = -2j
    c = np.ones(g2.shape)
    if device:
        g2, c = torch.from_numpy(g2).cuda(), torch.from_numpy(c).cuda()
    h, u = gradients.gradient_histogram(g2, c, BINS)
    h = h.cpu().numpy() if device else h
    assert h[0] == 0.5 * 9 * 13 and (h[1:] == 0).all() and u == 1.0
    # several windows of one launch, the last all +pi/2: bin 0 of each, nothing past the window's own bins
    w, r = gradients._hist(g2, c, (9, 13), [4, 4, 4], [6, 6], 72, normalise=False)
    w = w.cpu().numpy() if device else w
    assert w.shape == (3, 2, 72) and (w[..., 0] == 0.5 * 9 * 13).all() and (w[..., 1:] == 0).all()


def test_bins_outside_numpy_range():
    """A g2 that is not a principal root: angles in (-pi, -pi/2) give numpy's negative indices (-72 .. -1), which wrap as in
    the reference; angles beyond +pi/2 + step/2 give an index past the fold, where the reference raises IndexError."""
    import torch
    rng = np.random.default_rng(12)
    neg = 3.0 * np.exp(1j * rng.uniform(-np.pi + 0.1, -np.pi / 2 - 0.1, (21, 17)))
    c = rng.uniform(0, 1, neg.shape)
    h, u = gradients.gradient_histogram(neg, c, BINS)
    hr, ur, amb = ref.gradient_histogram(neg, c, BINS)
    assert u == ur and hr[36:].sum() > 0
    assert np.abs(h - hr).sum() <= 2 * amb + 1e-12 * hr.sum()
    far = neg.copy()
    far[3, 3] = np.exp(2.5j)
    with pytest.raises(IndexError):
        ref.gradient_histogram(far, c, BINS)
    with pytest.raises(IndexError, match="out of bounds"):
        gradients.gradient_histogram(far, c, BINS)
    with pytest.raises(IndexError, match="out of bounds"):
        gradients.gradient_histogram(torch.from_numpy(far).cuda(), torch.from_numpy(c).cuda(), BINS)


def test_cached_intermediates_on_another_stream():
    """The local gradients of a Gradients2D are computed once, on the stream current at the first `.histogram`; a second
    `.histogram` from another stream waits for them on the device."""
    import torch
    s0 = torch.from_numpy(scene((1203, 1597), np.float32, 13)).cuda()
    torch.cuda.synchronize()
    g = gradients.Gradients2D(s0, window_size=1600, window_step=0.5, line=LINE, sample=SAMPLE)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        first = g.histogram.weight.cpu()
    g2 = gradients.Gradients2D(s0, window_size=1600, window_step=0.5, line=LINE, sample=SAMPLE)
    with torch.cuda.stream(a):
        _ = g2._field.lg  # queued on stream a, nothing synchronised
    with torch.cuda.stream(b):
        second = g2.histogram.weight.cpu()
    assert torch.equal(first, second)
