"""xsarsea_amd.gradients.filtering_parameters / Mean / smoothing on the MI355X against the CPU restatement
(tests/filtering_ref.py): per pixel on small scenes (float32 / float64, numpy / device tensor on a user stream), bit-identity
between routes and runs, the square root on load, the smallest raster, and one 20000 x 20000 raster compared on crops.

Tolerance of f1..f4, F: absolute 1e-9.  It follows from the module's 1e-12 on r2, G3 and c: the worst amplification is f1
inside its ramp, df1 ~ 25 / P1 * eps, below 1e3 * eps for P1 >= 0.035; f2's 5000 acts on a P2 of about 5e-4; F is 1/2-Lipschitz
in the f vector.  NaN positions are equal, except for f1 and F at ill-conditioned pixels (d = J1 - J**2 <= 1e-9 J1, where the
sign of d is rounding noise); tests/test_filtering_cpu.py asserts on the restatement alone that every scene used here has at most
0.1 % of those, at least 5 % of its pixels inside each filter's ramp and at least 80 % finite outputs."""
import numpy as np
import pytest

import filtering_ref as fr
from xsarsea_amd import _lib, gradients
from xsarsea_amd.gradients import Mean, filtering_parameters, smoothing

pytestmark = pytest.mark.gpu
NAMES = ("f1", "f2", "f3", "f4", "F")
ATOL = 1e-9


def to_numpy(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def assert_close_rel(a, b, rtol):
    a, b = to_numpy(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    err = np.abs(a[m] - b[m])
    print(f"max relative error {np.max(err / np.abs(b[m])):.3g}")
    assert (err <= rtol * np.abs(b[m])).all()


def compare(got, want, label):
    """got: five rasters; want: the restatement's (f1, f2, f3, f4, F, d, J1) on the same grid."""
    d, J1 = want[5], want[6]
    with np.errstate(invalid="ignore"):
        ill = np.isfinite(J1) & (d <= 1e-9 * J1)
    worst = {}
    for name, a, b in zip(NAMES, got, want):
        a = to_numpy(a)
        assert a.shape == b.shape and a.dtype == np.float64, name
        free = ill if name in ("f1", "F") else np.zeros_like(ill)
        np.testing.assert_array_equal(np.isnan(a) | free, np.isnan(b) | free, err_msg=name)
        m = ~np.isnan(a) & ~np.isnan(b)
        assert m.mean() >= 0.5, f"{label}: {name} is mostly NaN here, the comparison would show little"
        worst[name] = float(np.abs(a[m] - b[m]).max())
        assert ((a[m] >= 0) & (a[m] <= 1)).all(), name
    print(f"{label}: max abs error " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; ill-conditioned {int(ill.sum())}")
    for name, v in worst.items():
        assert v <= ATOL, (label, name, v)


@pytest.mark.parametrize("shape", [(203, 317), (64, 65), (5, 40), (41, 3)])
def test_mean_and_smoothing(shape):
    """Against the restatement: 1e-12 relative, equal NaN positions; the last two shapes have an axis shorter than Mean's reach
    of 6, where the reflections repeat."""
    import torch
    x = fr.rain_scene(shape, np.float64, 31, land=min(shape) > 8)
    if min(shape) <= 8:
        x[shape[0] // 2, shape[1] // 2] = np.nan
    for fn, ref in ((Mean, fr.Mean), (smoothing, fr.smoothing)):
        want = ref(x)
        out = fn(x)
        assert isinstance(out, np.ndarray)
        assert_close_rel(out, want, 1e-12)
        dev = fn(torch.from_numpy(x).cuda())
        assert dev.is_cuda and dev.dtype == torch.float64
        np.testing.assert_array_equal(dev.cpu().numpy(), out)
    out32 = Mean(x.astype(np.float32))  # float32 in: widened, float64 out
    assert out32.dtype == np.float64
    assert_close_rel(out32, fr.Mean(x.astype(np.float32)), 1e-12)


def test_mean_nan_footprint():
    """B42's zero taps multiply: one NaN makes 13 x 13 outputs NaN (5 x 5 after B4, widened by the full 9 x 9), one Inf too."""
    x = np.ones((40, 50))
    x[20, 30] = np.nan
    out = Mean(x)
    assert np.isnan(out).sum() == 169 and np.isnan(out[14:27, 24:37]).all()
    np.testing.assert_array_equal(np.isnan(out), np.isnan(fr.Mean(x)))
    x[20, 30] = np.inf
    np.testing.assert_array_equal(np.isnan(Mean(x)), np.isnan(fr.Mean(x)))


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("spec", fr.GPU_SCENES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{np.dtype(s[1]).name}")
def test_filtering_parameters_matches_the_restatement(spec, device):
    import torch
    shape, dtype, seed, gamma = spec
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    line, sample = np.arange(shape[0]) * 10.0 + 5, np.arange(shape[1]) * 10.0 + 5
    want = fr.filtering_parameters(s0)
    if device:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            t = torch.from_numpy(s0).cuda()  # produced on the user stream, consumed there without any synchronisation
            res = filtering_parameters(t, line=line, sample=sample)
            assert all(r.is_cuda and r.dtype == torch.float64 for r in res)
            got = list(torch.stack(list(res)).cpu().numpy())  # dependent torch work on that stream, no device synchronise
    else:
        res = filtering_parameters(s0, line=line, sample=sample)
        assert all(isinstance(r, np.ndarray) for r in res)
        got = list(res)
    f1, f2, f3, f4, F = res  # unpacks as the reference's 5-tuple
    assert len(res) == 5 and res.F is F
    np.testing.assert_array_equal(res.line, fr.coarsen_coords(line, 2))
    np.testing.assert_array_equal(res.sample, fr.coarsen_coords(sample, 2))
    compare(got, want, f"{shape} {np.dtype(dtype).name} {'tensor' if device else 'numpy'}")


def test_routes_and_runs_are_bit_identical():
    import torch
    shape, dtype, seed, gamma = fr.GPU_SCENES[0]
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    host = filtering_parameters(s0)
    t = torch.from_numpy(s0).cuda()
    a, b = filtering_parameters(t), filtering_parameters(t)
    for h, x, y in zip(host, a, b):
        assert torch.equal(x, y) or np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
        np.testing.assert_array_equal(x.cpu().numpy(), h)
        np.testing.assert_array_equal(y.cpu().numpy(), h)

    class Obj:  # an object with .values / .line / .sample
        values, line, sample = s0, np.arange(shape[0]) * 2.0, np.arange(shape[1]) * 3.0
    o = filtering_parameters(Obj())
    np.testing.assert_array_equal(o.F, host.F)
    assert o.line[0] == 1.0 and o.sample[0] == 1.5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_square_root_on_load_is_the_ieee_root(dtype):
    """R2 / local_gradients with the root taken on load give the bits of the existing entry points fed numpy's (IEEE, correctly
    rounded) np.sqrt of the same dtype; negative sigma0 gives NaN.  The existing routes are the public R2 / local_gradients,
    pinned by tests/test_gpu_gradients.py."""
    s0 = fr.rain_scene((203, 317), dtype, 32)
    s0[7, 9] = -0.01
    with np.errstate(invalid="ignore"):
        ampl = np.sqrt(s0)
    assert ampl.dtype == dtype and np.isnan(ampl[7, 9])
    L, S = s0.shape
    call = gradients._Call(s0)
    r2, g3, c = (np.empty((L // 2, S // 2)) for _ in range(3))
    g2 = np.empty((L // 2, S // 2), np.complex128)
    dt = call.xsw_dtype(s0)
    call.ctx.grad_r2_sqrt_raw(L, S, dt, _lib.MEM_HOST, s0.ctypes.data, r2.ctypes.data)
    call.ctx.grad_local_sqrt_raw(L, S, dt, _lib.MEM_HOST, s0.ctypes.data, g2.ctypes.data, g3.ctypes.data, c.ctypes.data)
    np.testing.assert_array_equal(r2, gradients.R2(ampl))
    lg = gradients.local_gradients(ampl)
    np.testing.assert_array_equal(g2.view(np.float64), np.ascontiguousarray(lg.G2).view(np.float64))
    np.testing.assert_array_equal(g3, lg.G3)
    np.testing.assert_array_equal(c, lg.c)
    g3b, cb = np.empty_like(g3), np.empty_like(c)
    call.ctx.grad_local_sqrt_raw(L, S, dt, _lib.MEM_HOST, s0.ctypes.data, None, g3b.ctypes.data, cb.ctypes.data)  # G2 skipped
    np.testing.assert_array_equal(g3b, g3)
    np.testing.assert_array_equal(cb, c)


def test_smallest_raster():
    """4 pixels per axis is the least the reference computes (one-element quarter-resolution axis); below that ValueError."""
    rng = np.random.default_rng(33)
    for shape in ((4, 4), (4, 9), (5, 7), (7, 4), (9, 12)):
        s0 = 0.1 + rng.uniform(0, 0.05, shape)
        compare(list(filtering_parameters(s0)), fr.filtering_parameters(s0), f"{shape}")
    import torch
    for shape in ((3, 8), (8, 3), (2, 2)):
        with pytest.raises(ValueError, match="4 x 4"):
            filtering_parameters(np.full(shape, 0.1))
        with pytest.raises(ValueError, match="4 x 4"):
            filtering_parameters(torch.full(shape, 0.1, device="cuda"))


def test_full_size():
    """One 20000 x 20000 float32 device raster (the 2000 x 2000 rain scene, rolled to keep land off the corners, tiled 10 x 10; its seams are more heterogeneity).
    Seven 96 x 96 half-resolution crops (four corners, two edges, the centre, which lies on a seam) against the restatement run
    on sub-rasters with a 64-pixel margin on interior sides; f2 and F use zoom_linear at the global coordinates."""
    import torch
    N, H = 20000, 96
    tile = torch.from_numpy(fr.full_tile()).cuda()
    t = tile.repeat(N // tile.shape[0], N // tile.shape[1])
    assert tuple(t.shape) == (N, N) and t.dtype == torch.float32
    res = filtering_parameters(t)
    L2, L4 = N // 2, N // 4
    assert all(tuple(r.shape) == (L2, L2) for r in res)
    ends = {"first": 0, "middle": L2 // 2 - H // 2, "last": L2 - H}
    for wy, wx in [("first", "first"), ("first", "last"), ("last", "first"), ("last", "last"), ("first", "middle"),
                   ("middle", "first"), ("middle", "middle")]:
        hy, hx = ends[wy], ends[wx]
        a, b = max(0, (2 * hy - 64) // 4 * 4), min(N, 2 * (hy + H) + 64)
        c, d = max(0, (2 * hx - 64) // 4 * 4), min(N, 2 * (hx + H) + 64)
        terms = fr.terms(t[a:b, c:d].cpu().numpy())
        ys, xs = slice(hy - a // 2, hy - a // 2 + H), slice(hx - c // 2, hx - c // 2 + H)
        Z = fr.zoom_linear(terms.pop("q4"), (L2, L2), np.arange(hy, hy + H), np.arange(hx, hx + H), origin=(a // 4, c // 4),
                           in_shape=(L4, L4))
        want = fr.combine({k: v[ys, xs] for k, v in terms.items()}, Z)
        got = [r[hy:hy + H, hx:hx + H].cpu().numpy() for r in res]
        compare(got, want, f"full size, crop {wy} / {wx}")
