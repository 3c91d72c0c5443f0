"""Direction histograms that honour a keep mask, on the MI355X (rule 8): `keep_mask` against the numpy
restatement (tests/masked_ref.py) bit for bit; the masked histogram kernel against the UNMASKED one fed a copy of G2 with NaN
written at the masked pixels, bit for bit; `Gradients(..., min_F=, mask=)` against the restatement (keep masks equal, used_ratio
exact, weights to the module's existing 1e-9); routes and runs; the chain to the a-priori wind raster; one 20000 x 20000 raster.
tests/test_masked_gradients_cpu.py asserts, on the restatement alone, the conditions that make these comparisons mean something
(no F within 1e-8 of a threshold, kept shares inside [0.15, 0.95], masked and untouched windows among those compared)."""
import numpy as np
import pytest

import filtering_ref as fr
import gradients_ref as ref
import masked_ref as mr
import streaks_ref as sref
from test_gpu_gradients import compare_histograms
from test_gpu_streaks import check_ancillary, compare_streaks
from test_gpu_streams import _read_back
from test_gpu_streams import torch  # noqa: F401  (fixture)
from util import bits_equal
from xsarsea_amd import _lib, gradients, streaks

pytestmark = pytest.mark.gpu
BINS = ref.angles_bins(72)
NAN = complex(np.nan, np.nan)


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ------------------------------------------------------------------------------------------------------------ keep_mask
def raster_f64(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, shape)
    a[rng.random(shape) < 0.01] = np.nan
    a[rng.random(shape) < 0.01] = np.inf
    a[rng.random(shape) < 0.01] = -np.inf
    a[rng.random(shape) < 0.02] = 0.25      # exactly on the threshold: >= keeps it
    return a


@pytest.mark.parametrize("block", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("shape", [(37, 53), (40, 50), (64, 96), (131, 262)])
def test_keep_mask_is_bit_equal_to_the_restatement(torch, shape, block):
    """float64 + threshold, uint8, bool; remainders trimmed; NaN and +-Inf; with and without and_with; numpy in -> numpy out and
    tensor in -> tensor out.  The shapes reach every load width of the kernel (row bytes divisible by 16, 8, 4 or not at all)."""
    rng = np.random.default_rng(shape[1] + block)
    a = raster_f64(shape, shape[0] + block)
    u = (rng.random(shape) < 0.97).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)   # any non-zero value is usable
    other = (rng.random((shape[0] // block, shape[1] // block)) < 0.7).astype(np.uint8)
    cases = [(a, 0.25), (a, -np.inf), (a, np.inf), (u, None), (u.astype(bool), None)]
    for src, thr in cases:
        for aw in (None, other, other.astype(bool)):
            want = mr.keep_blocks(src, block, thr, and_with=aw)
            got = gradients.keep_mask(src, threshold=thr, block=block, and_with=aw)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8
            np.testing.assert_array_equal(got, want)
            dev = gradients.keep_mask(torch.from_numpy(src).cuda(), threshold=thr, block=block,
                                      and_with=None if aw is None else torch.from_numpy(aw).cuda())
            assert dev.is_cuda and dev.dtype == torch.uint8
            np.testing.assert_array_equal(dev.cpu().numpy(), want)


def test_keep_mask_unaligned_views_and_float32(torch):
    """A device view that starts in the middle of an allocation (its base not 16-byte aligned) and float32 input (widened)."""
    a = raster_f64((41, 53), 5)
    t = torch.from_numpy(a).cuda()[1:]
    np.testing.assert_array_equal(gradients.keep_mask(t, threshold=0.25, block=2).cpu().numpy(), mr.keep_blocks(a[1:], 2, 0.25))
    u = (np.random.default_rng(6).random((41, 53)) < 0.95)
    tu = torch.from_numpy(u).cuda()[1:]
    for b in (1, 4):
        np.testing.assert_array_equal(gradients.keep_mask(tu, block=b).cpu().numpy(), mr.keep_blocks(u[1:], b))
    a32 = a.astype(np.float32)
    np.testing.assert_array_equal(gradients.keep_mask(a32, threshold=0.25, block=2), mr.keep_blocks(a32.astype(np.float64), 2, 0.25))


def test_keep_entry_points_refuse_bad_arguments():
    ctx = _lib.default_context(0)
    src, out = np.ones((8, 8)), np.zeros((4, 4), np.uint8)
    for args in ((8, 8, _lib.MEM_HOST, src.ctypes.data, float("nan"), 2, None, out.ctypes.data),      # NaN threshold
                 (8, 8, _lib.MEM_HOST, src.ctypes.data, 0.5, 0, None, out.ctypes.data),               # block < 1
                 (8, 8, _lib.MEM_HOST, src.ctypes.data, 0.5, 9, None, out.ctypes.data),               # empty output
                 (8, 8, _lib.MEM_HOST, src.view(np.uint8).ctypes.data, None, 0, None, out.ctypes.data),
                 (8, 8, _lib.MEM_HOST, None, 0.5, 2, None, out.ctypes.data)):
        with pytest.raises(_lib.XswError):
            ctx.grad_keep_raw(*args)
    g2, c = np.ones((8, 8), np.complex128), np.ones((8, 8))
    rows = np.array([4], np.int32)
    w, r = np.zeros(72), np.zeros(1)
    with pytest.raises(_lib.XswError, match="keep is NULL"):   # no silent fall-through to the unmasked kernel
        ctx.grad_hist_masked_raw(8, 8, _lib.MEM_HOST, g2.ctypes.data, c.ctypes.data, None, 8, 8, 1, rows.ctypes.data, 1, rows.ctypes.data,
                                 72, BINS[0], BINS[1] - BINS[0], False, w.ctypes.data, r.ctypes.data)


# ------------------------------------------------------------------------------- masked kernel against the unmasked one
def nan_written(g2, keep):
    out = np.array(g2, dtype=np.complex128)
    out[np.asarray(keep) == 0] = NAN
    return out


@pytest.fixture(scope="module")
def local_field():
    """(G2, c, Koch keep masks at 0.3 and 0.7) of one scene with land, from the device."""
    s0 = fr.rain_scene((402, 515), np.float32, 22, 100)
    g2, _g3, c = gradients._local(gradients._r2(s0, True))
    F = gradients.filtering_parameters(s0).F
    return g2, c, {t: gradients.keep_mask(F, threshold=t, block=2) for t in mr.THRESHOLDS}


@pytest.mark.parametrize("n_angles", [72, 90])
@pytest.mark.parametrize("window", [20, 33])
def test_masked_kernel_equals_unmasked_kernel_on_nan(torch, local_field, window, n_angles):
    """Random masks of density 0, 0.1, 0.5, 0.9, 1 and the Koch masks; windows hanging over all four raster edges, an even and
    an odd window side, 72 bins and 90 (two sweeps of the bin accumulator): weights and used_ratio bit-identical."""
    g2, c, koch = local_field
    L, S = g2.shape
    assert koch[0.3].shape == (L, S)
    rows, cols = [-3, 0, 7, L // 2, L - 2, L + 5], [-8, 1, S // 3, S // 2, S - 1, S + 9]
    rng = np.random.default_rng(window + n_angles)
    masks = {f"density {d}": (rng.random((L, S)) < d).astype(np.uint8) for d in (0.0, 0.1, 0.5, 0.9, 1.0)}
    masks.update({f"Koch {t}": k for t, k in koch.items()})
    plain_w, plain_r = gradients._hist(g2, c, window, rows, cols, n_angles)
    assert (plain_r > 0).any()
    for name, keep in masks.items():
        w, r = gradients._hist(g2, c, window, rows, cols, n_angles, keep=keep)
        wn, rn = gradients._hist(nan_written(g2, keep), c, window, rows, cols, n_angles)
        assert bits_equal(w, wn) and bits_equal(r, rn), name
        if name == "density 1.0":
            assert bits_equal(w, plain_w) and bits_equal(r, plain_r)
        if name == "density 0.0":
            assert (w == 0).all() and (r == 0).all()
        if name in ("density 0.5", "Koch 0.7"):
            assert (r < plain_r).any() and (r > 0).any(), name
            dw, dr = gradients._hist(torch.from_numpy(g2).cuda(), torch.from_numpy(c).cuda(), window, rows, cols, n_angles,
                                     keep=torch.from_numpy(keep).cuda())
            assert dw.is_cuda and bits_equal(dw.cpu().numpy(), w) and bits_equal(dr.cpu().numpy(), r), name + " (device route)"
            wb, rb = gradients._hist(g2, c, window, rows, cols, n_angles, keep=keep.astype(bool))
            assert bits_equal(wb, w) and bits_equal(rb, r), name + " (bool)"


def test_gradient_histogram_one_box_with_keep(local_field):
    g2, c, koch = local_field
    box, cb, keep = g2[40:77, 100:153], c[40:77, 100:153], koch[0.7][40:77, 100:153]
    assert 0 < keep.mean() < 1
    h, u = gradients.gradient_histogram(box, cb, BINS, keep=keep)
    hn, un = gradients.gradient_histogram(nan_written(box, keep), cb, BINS)
    assert bits_equal(h, hn) and u == un
    hr, ur, amb = ref.gradient_histogram(mr.nan_where_masked(box, keep), cb, BINS)
    assert u == ur and np.abs(h - hr).sum() <= 2 * amb + 1e-12 * hr.sum()
    # a pixel outside numpy's bin range raises only while it is not masked out
    far = np.array(box)
    far[3, 3] = np.exp(2.5j)
    k2 = np.ones(box.shape, np.uint8)
    with pytest.raises(IndexError, match="out of bounds"):
        gradients.gradient_histogram(far, cb, BINS, keep=k2)
    k2[3, 3] = 0
    gradients.gradient_histogram(far, cb, BINS, keep=k2)


# ------------------------------------------------------------------------------------ Gradients(min_F=, mask=) end to end
def fields_of(g):
    """The distinct _Field objects of a Gradients, in (pol, factor) order."""
    out = []
    for g2d in g.gradients_list:
        if not any(g2d._field is f for f in out):
            out.append(g2d._field)
    return out


def user_mask(shape, seed):
    """A mask on the sigma0 grid: a rectangle and a disc masked out, plus isolated pixels (each removes one 4f x 4f block)."""
    rng = np.random.default_rng(seed)
    L, S = shape
    y, x = np.mgrid[0:L, 0:S]
    m = np.ones(shape, bool)
    m[L // 3: L // 3 + 37, S // 2: S // 2 + 61] = False
    m[(y - 0.75 * L) ** 2 + (x - 0.7 * S) ** 2 < (0.1 * min(L, S)) ** 2] = False
    m[rng.random(shape) < 0.002] = False
    return m


def check_against_restatement(s0, h, g, label, min_F=None, mask=None):
    line, sample = mr.coords(s0.shape)
    W, R, A, at, keeps, R0 = mr.histogram_masked(s0, line, sample, mr.WINDOWS_SIZES, mr.FACTORS, 1, min_F=min_F, mask=mask)
    np.testing.assert_array_equal(h.line, at["line"])
    for f, field, want in zip(mr.FACTORS, fields_of(g), keeps):
        got = host(field.keep)
        assert got.dtype == np.uint8 and got.shape == want.shape
        n_diff = int((got != want).sum())
        print(f"{label} factor {f}: keep mask {got.shape}, kept share {want.mean():.3f}, {n_diff} pixels differ")
        assert n_diff == 0
    masked, untouched = mr.window_groups(R, R0)
    print(f"{label}: {masked} windows nearly masked, {untouched} untouched")

    class H:
        weight, used_ratio = host(h.weight), host(h.used_ratio)
    compare_histograms(H, W, R, A, label)
    return R, R0


@pytest.mark.parametrize("threshold", mr.THRESHOLDS)
@pytest.mark.parametrize("spec", fr.GPU_SCENES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{np.dtype(s[1]).name}")
def test_min_F_matches_the_restatement(spec, threshold):
    shape, dtype, seed, gamma = spec
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    line, sample = mr.coords(shape)
    g = gradients.Gradients(s0, windows_sizes=list(mr.WINDOWS_SIZES), downscales_factors=list(mr.FACTORS), line=line, sample=sample,
                            min_F=threshold)
    h = g.histogram
    R, R0 = check_against_restatement(s0, h, g, f"{shape} {np.dtype(dtype).name} min_F {threshold}", min_F=threshold)
    assert (R < R0).any()


@pytest.mark.parametrize("min_F", [None, 0.7])
@pytest.mark.parametrize("as_uint8", [False, True])
def test_sigma0_grid_mask_matches_the_restatement(min_F, as_uint8):
    shape, dtype, seed, gamma = fr.GPU_SCENES[2]
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    m = user_mask(shape, 7)
    m = m.astype(np.uint8) * 255 if as_uint8 else m
    line, sample = mr.coords(shape)
    g = gradients.Gradients(s0, windows_sizes=list(mr.WINDOWS_SIZES), downscales_factors=list(mr.FACTORS), line=line, sample=sample,
                            mask=m, min_F=min_F)
    R, R0 = check_against_restatement(s0, g.histogram, g, f"mask {'uint8' if as_uint8 else 'bool'} min_F {min_F}", min_F=min_F, mask=m)
    assert (R < R0).any() and (R == R0).any()
    # masking is not NaN in sigma0: the neighbours of a masked pixel keep their gradients
    one = gradients.Gradients2D(s0, window_size=800, line=line, sample=sample, mask=m, min_F=min_F)
    np.testing.assert_array_equal(host(one._field.lg[0]).view(np.float64),
                                  host(gradients.Gradients2D(s0, window_size=800, line=line, sample=sample)._field.lg[0]).view(np.float64))


def test_routes_and_runs_are_bit_identical(torch):
    shape, dtype, seed, gamma = fr.GPU_SCENES[0]
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    m = user_mask(shape, 8)
    line, sample = mr.coords(shape)
    kw = dict(windows_sizes=list(mr.WINDOWS_SIZES), downscales_factors=list(mr.FACTORS), line=line, sample=sample, min_F=0.7)
    hh = gradients.Gradients(s0, mask=m, **kw).histogram
    assert isinstance(hh.weight, np.ndarray)
    t, tm = torch.from_numpy(s0).cuda(), torch.from_numpy(m).cuda()
    a = gradients.Gradients(t, mask=tm, **kw).histogram
    b = gradients.Gradients(t, mask=m, **kw).histogram      # a host mask with a device sigma0: uploaded
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t2 = torch.from_numpy(s0).cuda()                    # produced and consumed on the user stream, nothing synchronised
        c = gradients.Gradients(t2, mask=torch.from_numpy(m).cuda(), **kw).histogram
        cw, cr = c.weight.cpu().numpy(), c.used_ratio.cpu().numpy()
    assert a.weight.is_cuda and a.weight.dtype == torch.float64
    for x in (a, b):
        assert bits_equal(x.weight.cpu().numpy(), hh.weight) and bits_equal(x.used_ratio.cpu().numpy(), hh.used_ratio)
    assert bits_equal(cw, hh.weight) and bits_equal(cr, hh.used_ratio)
    pol = gradients.Gradients(np.stack([s0, s0[::-1].copy()]), mask=m, **kw).histogram      # one mask for all pols
    assert bits_equal(pol.weight[0], hh.weight) and pol.weight.shape[0] == 2
    plain = gradients.Gradients(s0, windows_sizes=list(mr.WINDOWS_SIZES), downscales_factors=list(mr.FACTORS), line=line, sample=sample).histogram
    assert (hh.used_ratio <= plain.used_ratio).all() and (hh.used_ratio < plain.used_ratio).any()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_masked_windows_drop_out_of_the_a_priori_wind(torch):
    """rain_scene -> Gradients(min_F=0.7).histogram -> streaks_direction -> resolve(min_used_ratio=r) -> ancillary_from_streaks.
    r comes from the restatement's used ratios (the middle of their largest gap, at least 0.2 wide): the windows centred on the
    two strongest blobs resolve to NaN, while the same call without min_F keeps them; every stage equals its restatement on the
    device's own histograms; the chain on a user stream without any synchronisation is bit-equal to the synchronised run."""
    shape, dtype, seed, gamma = mr.CHAIN_SCENE
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    line, sample = mr.coords(shape)
    at, blobs = mr.chain_windows()
    _, R, A, _, keeps, R0 = mr.histogram_masked(s0, line, sample, (400,), (1,), windows_at=at, min_F=mr.CHAIN_MIN_F)
    r, gap, below, above = mr.separating_ratio(R[0, 0], R0[0, 0])
    assert gap >= 0.2 and above.sum() >= 3 and all(below[i, j] for i, j in blobs)
    rng = np.random.default_rng(50)
    anc = rng.normal(0, 5, shape) + 1j * rng.normal(0, 5, shape)
    anc[300:330, 100:160] = NAN

    def chain(sig, a, sync, **mask_kw):
        step = torch.cuda.synchronize if sync else (lambda: None)
        g = gradients.Gradients2D(sig, window_size=400, windows_at=at, line=line, sample=sample, **mask_kw)
        h = g.histogram
        step()
        s = streaks.streaks_direction(h)
        step()
        d = s.resolve(a, line, sample, min_used_ratio=r)
        step()
        prior = streaks.ancillary_from_streaks(s, a, line, sample, min_used_ratio=r)
        step()
        return h, s, d, prior

    h, s, d, prior = chain(s0, anc, False, min_F=mr.CHAIN_MIN_F)
    np.testing.assert_array_equal(h.used_ratio, R[0, 0])
    _, _, d_plain, prior_plain = chain(s0, anc, False)
    for i, j in blobs:
        assert np.isnan(d[i, j].real) and not np.isnan(d_plain[i, j].real)
    assert not np.isnan(d[above].real).any() and np.isnan(d[below].real).all()
    assert not bits_equal(prior, prior_plain)
    # each stage against its restatement on the device's own histograms
    want = compare_streaks(s, h.weight[None], h.used_ratio[None], BINS, True, True, "masked chain")
    dw = sref.resolve(s.angle, s.weight, s.used_ratio, sref.at_windows(anc, line, sample, at["line"], at["sample"]), min_used_ratio=r)
    assert bits_equal(d, dw)
    check_ancillary(prior, anc, (dw, at["line"], at["sample"], line, sample), "masked chain")
    assert want["used_ratio"].shape == (3, 3)
    # device tensors: synchronised step by step, then on a user stream with nothing synchronised before the read-back
    t_s0, t_anc = torch.from_numpy(s0).cuda(), torch.from_numpy(anc).cuda()
    torch.cuda.synchronize()
    _, _, d_ref, prior_ref = chain(t_s0, t_anc, True, min_F=mr.CHAIN_MIN_F)
    d_ref, prior_ref = host(d_ref), host(prior_ref)
    assert bits_equal(d_ref, d) and bits_equal(prior_ref, prior)
    P = torch.cuda.Stream()
    with torch.cuda.stream(P):
        b_s0, b_anc = torch.empty_like(t_s0), torch.empty_like(t_anc)
        b_s0.copy_(t_s0, non_blocking=True)
        b_anc.copy_(t_anc, non_blocking=True)
        _, _, d_dev, prior_dev = chain(b_s0, b_anc, False, min_F=mr.CHAIN_MIN_F)
        got_d, got_prior = _read_back(torch, P, d_dev, prior_dev)
    assert bits_equal(got_d, d_ref), "resolved directions on a user stream"
    assert bits_equal(got_prior, prior_ref), "a-priori raster on a user stream"


# ------------------------------------------------------------------------------------------------------------ full size
def test_full_size(torch):
    """20000 x 20000 float32 (the 2000 x 2000 rain tile, 10 x 10), notebook configuration, min_F = 0.7: every window of every
    configuration bit-identical to the unmasked kernel on G2 with NaN written at the masked pixels; the factor-1 keep mask on
    five 48 x 48 crops (four corners and the centre, which lies on a seam) equal to the restatement run on sub-rasters with a
    64-pixel margin on interior sides (the construction of tests/test_gpu_filtering.py::test_full_size)."""
    N, H, T = 20000, 96, 0.7
    tile = torch.from_numpy(fr.full_tile()).cuda()
    t = tile.repeat(N // tile.shape[0], N // tile.shape[1])
    assert tuple(t.shape) == (N, N) and t.dtype == torch.float32
    g = gradients.Gradients(t, windows_sizes=[1600, 3200], downscales_factors=[1, 2], min_F=T)
    h = g.histogram
    plain = gradients.Gradients(t, windows_sizes=[1600, 3200], downscales_factors=[1, 2]).histogram
    assert tuple(h.weight.shape) == (2, 2, 13, 13, 72)
    k = 0
    for a, f in enumerate((1, 2)):
        for b in range(2):
            g2d = g.gradients_list[k]
            k += 1
            g2, c, lgl, lgs = g2d._field.lg
            keep = g2d._field.keep
            assert tuple(keep.shape) == tuple(g2.shape) == (N // (4 * f), N // (4 * f))
            share = float(keep.float().mean())
            w = gradients.window_pixels(g2d.window_size, lgl, lgs)
            rows = gradients.nearest_indexer(lgl, g2d.windows_at["line"])
            cols = gradients.nearest_indexer(lgs, g2d.windows_at["sample"])
            g2n = g2.clone()
            g2n[keep == 0] = NAN
            wn, rn = gradients._hist(g2n, c, w, rows, cols, 72)
            del g2n
            same_w, same_r = bool(torch.equal(h.weight[a, b], wn)), bool(torch.equal(h.used_ratio[a, b], rn))
            lower = int((h.used_ratio[a, b] < plain.used_ratio[a, b]).sum())
            print(f"factor {f} window {w}: kept share {share:.3f}, weights identical {same_w}, used_ratio identical {same_r}, "
                  f"{lower} of 169 windows lost pixels")
            assert same_w and same_r
            assert 0.15 <= share <= 0.95 and lower > 100
    keep = g.gradients_list[0]._field.keep
    L2, L4 = N // 2, N // 4
    ends = {"first": 0, "middle": L2 // 2 - H // 2, "last": L2 - H}
    for wy, wx in [("first", "first"), ("first", "last"), ("last", "first"), ("last", "last"), ("middle", "middle")]:
        hy, hx = ends[wy], ends[wx]
        a0, b0 = max(0, (2 * hy - 64) // 4 * 4), min(N, 2 * (hy + H) + 64)
        c0, d0 = max(0, (2 * hx - 64) // 4 * 4), min(N, 2 * (hx + H) + 64)
        terms = fr.terms(t[a0:b0, c0:d0].cpu().numpy())
        ys, xs = slice(hy - a0 // 2, hy - a0 // 2 + H), slice(hx - c0 // 2, hx - c0 // 2 + H)
        Z = fr.zoom_linear(terms.pop("q4"), (L2, L2), np.arange(hy, hy + H), np.arange(hx, hx + H), origin=(a0 // 4, c0 // 4),
                           in_shape=(L4, L4))
        F = fr.combine({kk: v[ys, xs] for kk, v in terms.items()}, Z)[4]
        with np.errstate(invalid="ignore"):
            assert int((np.abs(F - T) < 1e-8).sum()) == 0, "the restatement's F lies on the threshold in this crop"
        want = mr.keep_blocks(F, 2, T)
        got = keep[hy // 2: hy // 2 + H // 2, hx // 2: hx // 2 + H // 2].cpu().numpy()
        print(f"full size, keep crop {wy} / {wx}: kept share {want.mean():.3f}, {int((got != want).sum())} pixels differ")
        assert 0 < want.mean() < 1
        np.testing.assert_array_equal(got, want)
