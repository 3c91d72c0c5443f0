"""GPU: the noise flattening's log10 / exp10 pair (xsw_nesz.hpp: nesz_log10 / nesz_exp10 for float64 rasters, v_log_f32 / v_exp_f32
for float32 ones) against exact arithmetic, on the raster of tests/nesz_ref.py that makes every output of a line a function of
ONE argument: out = 10 ** (((x / 70 + 1 / 2) * 10 log10(v) - 1) / 10) at x = 30, 35, 40.

Bounds (tests/nesz_ref.py, from the header's own statements): float64 rasters 1e-15 (1 + 0.2303 |y|) + r, float32 rasters
2**-23 (1 + 1.15 |t| + 0.345 |y|) + r, r the error of the plain float64 restatement at that argument; on the outputs whose exact
value is a normal number.  The others must not be NaN; the lines of 0, a negative value, +inf and NaN are NaN lines.  The device
route (k_nesz_colsum .. k_nesz_eval on device rasters) is held to the bound; the host route must give its bits; the fused
k_dsig_flat (`dsig_from_nesz`) must give the bits of get_dsig on the flattened noise, as tests/test_gpu_strips.py has it.

Each test prints the worst observed error / bound."""
import numpy as np
import pytest

import nesz_ref as ref
from test_gpu_dsig import NAMES
from test_gpu_streams import torch  # noqa: F401 (fixture)
from test_gpu_strips import _same_bits, _up
from util import bits_equal

pytestmark = pytest.mark.gpu


def _device_route(ctx, torch, noise, inc):
    from xsarsea_amd import _lib
    t_n, t_i = _up(noise, inc)
    out = torch.full(noise.shape, -7.0, dtype=torch.float64, device=t_n.device)
    torch.cuda.synchronize()
    ctx.nesz_flatten_raw(noise.shape[0], noise.shape[1], _lib.XSW_F32 if noise.dtype == np.float32 else _lib.XSW_F64, _lib.MEM_DEVICE,
                         t_n.data_ptr(), t_i.data_ptr(), out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pair_against_exact_arithmetic(gpu_ctx, torch, dtype):
    noise, inc = ref.rasters(dtype)
    got = _device_route(gpu_ctx, torch, noise, inc)
    name = np.dtype(dtype).name
    ref.check_lines(got, dtype, f"{name} device route")
    ratio, at, n = ref.worst_ratio(got, dtype)
    v, kinds = ref.arguments(dtype)
    print(f"\nnesz pair, {name} rasters: worst error / bound {ratio:.3f} at line {at[0]} (v = {v[at[0]]!r}, {kinds[at[0]]}) sample {at[1]}, "
          f"{n} outputs compared, {got.size - n} outside the normal range or NaN lines")
    assert ratio <= 1.0, f"{name}: the error at v = {v[at[0]]!r}, x = {ref.INC[at[1]]} is {ratio:.3f} of the bound"
    host = gpu_ctx.nesz_flatten_host(noise, inc)
    assert bits_equal(host, got), f"{name}: the host route differs from the device route"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_dsig_equals_the_two_calls(gpu_ctx, torch, dtype):
    """dsig_from_nesz == get_dsig on nesz_flattening, bit for bit, every rule, float64 and float32 stores: k_dsig_flat reuses the pair."""
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig, nesz_flattening
    noise, inc = ref.rasters(dtype)
    v = noise[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        sigma0 = (np.where(np.isfinite(v) & (v > 0), v, 1.0)[:, None] * np.array([0.5, 3.0, 40.0])[None, :]).astype(dtype)
    t_n, t_i, t_s = _up(noise, inc, sigma0)
    flat = nesz_flattening(t_n, t_i)
    assert bool(torch.isfinite(flat).any())
    for name in NAMES:
        want = get_dsig(name, t_i, t_s, flat)
        got = dsig_from_nesz(name, t_i, t_s, t_n)
        got32 = dsig_from_nesz(name, t_i, t_s, t_n, out_dtype=np.float32)
        for g, w, store in ((got, want, "float64"), (got32, want.to(torch.float32), "float32")):
            bad = _same_bits(torch, g, w)
            assert not bool(bad.any()), f"{name} {np.dtype(dtype).name} rasters, {store} store: {int(bad.sum())} pixels differ"
        assert bool(torch.isfinite(got).any())
