"""GPU: the whole noise flattening (xsw_nesz.hpp: k_nesz_colsum, k_nesz_colmean, k_nesz_center, k_nesz_fit, k_nesz_eval; xsw_dsig.hpp:
k_dsig_flat) at the rasters of tests/nesz_cases.py against the longdouble reference of tests/nesz_chain_ref.py.

Every case runs on the device route (nesz_flatten_raw on device rasters, the output pre-filled with a finite sentinel): NaN exactly
where the reference has NaN, no sentinel left, and on EVERY pixel where the reference is finite |out - reference| / reference within
the case's bound (nesz_chain_ref.bound: the pair's own bound with |y| replaced by kappa * Ymax, the closed form's centring term, and
F = 4 times the restatement's error on the line).  Each test prints its worst error / bound and where it is.

Then the routes: the host route gives the device route's bits; noise rasters and outputs that start 8 bytes off a 16-byte
boundary (float32 noise: 4 off 8), where k_nesz_fit and k_nesz_eval leave their pair accesses, give the aligned call's bits;
dsig_from_nesz (k_dsig_flat) gives the bits of get_dsig on nesz_flattening for every rule and both stores, sigma0 being the noise
times 0.5, 3, 40 cycled by column.  tall_blocks (9.6 Mpx, held one dtype at a time) does all of it in one test per dtype."""
import numpy as np
import pytest

import nesz_cases as nc
import nesz_chain_ref as ref
from test_gpu_dsig import NAMES
from test_gpu_nesz_pair import _device_route
from test_gpu_streams import torch  # noqa: F401 (fixture)
from test_gpu_strips import _same_bits, _up
from util import bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = -7.0  # what _device_route fills the output with
DTYPES = [np.float64, np.float32]
CASES = [(n, dt) for dt in DTYPES for n in nc.names(dt)]
HOST_ROUTE = ["samples_513", "samples_2049", "lines_17x131", "nan_inc_column"]
ALIGNMENT = ["samples_2", "samples_64", "samples_512", "lines_9x130", "lines_33x130"]  # even sample counts


def _id(case):
    return f"{case[0]}-{np.dtype(case[1]).name}"


def _rasters(c):
    """Writable copies of the case's read-only rasters (torch.from_numpy wants writable arrays)."""
    return c.noise.copy(), c.inc.copy()


def _hold(c, got, what):
    """NaN positions, sentinel, bound; returns the worst error / bound."""
    assert got.dtype == np.float64 and got.shape == c.noise.shape, what
    assert not (got == SENTINEL).any(), f"{what}: {int((got == SENTINEL).sum())} pixels were never stored"
    want_nan = np.isnan(c.ref.out)
    bad = np.isnan(got) != want_nan
    assert not bad.any(), f"{what}: NaN positions differ at {int(bad.sum())} pixels, first lines {np.flatnonzero(bad.any(axis=1))[:8].tolist()}"
    ratio, at, n, err = ref.worst_ratio(got, c.ref, c.bound)
    hard = int(np.argmax(c.R))  # the line the float64 sums cost most
    e_hard = np.where(want_nan[hard], 0.0, ref.rel_error(got[hard:hard + 1], ref.Ref(c.ref.out[hard:hard + 1], *c.ref[1:]))[0])
    print(f"\nnesz chain, {what}: worst error / bound {ratio:.3f} at line {at[0]} sample {at[1]} (error {err:.2e}, bound {c.bound[at]:.2e}, "
          f"R of the line {c.R[at[0]]:.2e}), {n} of {got.size} pixels compared; line {hard} of the largest R ({c.R[hard]:.2e}): error at worst "
          f"{e_hard.max():.2e}, {np.max(e_hard / c.bound[hard]):.3f} of its bound")
    assert ratio <= 1.0, f"{what}: the error at line {at[0]} sample {at[1]} is {ratio:.3f} of the bound"
    return ratio


def _sigma0(c):
    factor = np.array([0.5, 3.0, 40.0])[np.arange(c.noise.shape[1]) % 3]
    with np.errstate(all="ignore"):
        return (c.noise.astype(np.float64) * factor[None, :]).astype(c.dtype)


def _fused_equals_the_two_calls(torch, c, names):
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig, nesz_flattening
    t_n, t_i, t_s = _up(*_rasters(c), _sigma0(c))
    flat = nesz_flattening(t_n, t_i)
    for name in names:
        want = get_dsig(name, t_i, t_s, flat)
        got = dsig_from_nesz(name, t_i, t_s, t_n)
        got32 = dsig_from_nesz(name, t_i, t_s, t_n, out_dtype=np.float32)
        for g, w, store in ((got, want, "float64"), (got32, want.to(torch.float32), "float32")):
            bad = _same_bits(torch, g, w)
            assert not bool(bad.any()), f"{c.name} {c.dtype.name} rasters, {name}, {store} store: {int(bad.sum())} pixels differ"
        if np.isfinite(c.ref.out).any():
            assert bool(torch.isfinite(got).any()), (c.name, name)
        del want, got, got32
    return flat.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_device_route_within_the_bound(gpu_ctx, torch, case):
    c = nc.case(*case)
    got = _device_route(gpu_ctx, torch, *_rasters(c))
    _hold(c, got, f"{c.name} {c.dtype.name} device route")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", HOST_ROUTE)
def test_host_route_gives_the_device_routes_bits(gpu_ctx, torch, name, dtype):
    c = nc.case(name, dtype)
    got = _device_route(gpu_ctx, torch, *_rasters(c))
    host = gpu_ctx.nesz_flatten_host(c.noise, c.inc)
    assert np.isfinite(got).any() and bits_equal(host, got), f"{name} {c.dtype.name}: the host route differs from the device route"


def _offset_route(ctx, torch, c, noise_off, out_off):
    """The device route with the noise raster and / or the output starting one element into a fresh allocation."""
    from xsarsea_amd import _lib
    t_n, t_i = _up(*_rasters(c))
    dev, n = t_n.device, c.noise.size
    if noise_off:
        room = torch.empty(n + 1, dtype=t_n.dtype, device=dev)
        view = room[1:].view(c.noise.shape)
        view.copy_(t_n)
        t_n = view
    out_room = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=dev)
    out = out_room[1 if out_off else 0:][:n].view(c.noise.shape)
    item = c.dtype.itemsize
    assert t_n.data_ptr() % (2 * item) == (item if noise_off else 0) and out.data_ptr() % 16 == (8 if out_off else 0)
    assert t_n.is_contiguous() and out.is_contiguous()
    torch.cuda.synchronize()
    ctx.nesz_flatten_raw(*c.noise.shape, _lib.XSW_F32 if c.dtype == np.float32 else _lib.XSW_F64, _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(),
                         out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", ALIGNMENT)
def test_rasters_off_their_pair_alignment_give_the_aligned_bits(gpu_ctx, torch, name, dtype):
    """An even sample count, so only the base address decides between pair and element accesses: the noise raster one element
    into its allocation (float64: 8 mod 16 bytes, float32: 4 mod 8: k_nesz_fit reads element by element), the output 8 mod 16
    bytes (k_nesz_eval stores element by element), and both.  Same values in the same order: the aligned call's bits, and the bound."""
    c = nc.case(name, dtype)
    assert c.noise.shape[1] % 2 == 0
    aligned = _device_route(gpu_ctx, torch, *_rasters(c))
    _hold(c, aligned, f"{name} {c.dtype.name} aligned")
    for noise_off, out_off in ((True, False), (False, True), (True, True)):
        got = _offset_route(gpu_ctx, torch, c, noise_off, out_off)
        what = f"{name} {c.dtype.name}, noise off its pair alignment: {noise_off}, output 8 mod 16 bytes: {out_off}"
        assert bits_equal(got, aligned), what + ": differs from the aligned call"
        _hold(c, got, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("family", ["samples", "lines", "branch"])
def test_fused_dsig_equals_the_two_calls(gpu_ctx, torch, family, dtype):
    """dsig_from_nesz == get_dsig on nesz_flattening, bit for bit, every rule, float64 and float32 stores, on every sweep and branch
    case; nesz_flattening (the public call, on the caller's stream) gives the raw device route's bits."""
    names = [n for n in nc.names(dtype) if (n.split("_")[0] == family) or (family == "branch" and n.split("_")[0] not in ("samples", "lines"))]
    assert len(names) >= 10
    for name in names:
        c = nc.case(name, dtype)
        flat = _fused_equals_the_two_calls(torch, c, NAMES)
        assert bits_equal(flat, _device_route(gpu_ctx, torch, *_rasters(c))), name


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_tall_blocks(gpu_ctx, torch, dtype):
    """147 x 65540: lpb = 10, so every colsum block runs two unrolled groups and two tail lines (the last one group and three), as
    every block does at the workload's size; 129 trips of the fit loop.  Device route within the bound, the host route's bits,
    the fused pass for one rule."""
    c = nc.case("tall_blocks", dtype)
    got = _device_route(gpu_ctx, torch, *_rasters(c))
    _hold(c, got, f"tall_blocks {c.dtype.name} device route")
    host = gpu_ctx.nesz_flatten_host(c.noise, c.inc)
    assert bits_equal(host, got), f"tall_blocks {c.dtype.name}: the host route differs from the device route"
    del host
    flat = _fused_equals_the_two_calls(torch, c, NAMES[:1])
    assert bits_equal(flat, got)
    torch.cuda.empty_cache()
