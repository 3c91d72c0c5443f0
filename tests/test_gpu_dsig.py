"""GPU: dsig_cr on the device -- `get_dsig` / `get_dsig_wspd` on device tensors (k_dsig, k_dsig_wspd) against the reference's
golden outputs and the host functions, and `dsig_from_nesz` (k_dsig_flat, fused with the noise flattening) against the two
calls it replaces, bit for bit, and against the reference.

Tolerances (finite values; NaN positions, infinities and zeros must be equal exactly):
  float64 results  1e-12 relative  (a few ulp of pow / exp at exponents <= 8 is ~1e-14)
  float32 results  1e-6 relative   (same IEEE quotient r on both sides; its rounding amplified by at most 8/2, plus a couple of
                                    ulp of powf against float64-then-round: < 6 ulp ~ 4e-7)
  get_dsig_wspd    1e-12 absolute  (values in [0, 1])
Each test prints the maxima it measured."""
import warnings

import numpy as np
import pytest

from conftest import golden
from test_gpu_streams import _dev, _held_back, _in_flight, _read_back, _staged, delay_cycles, fresh_ctx, torch  # noqa: F401 (fixtures)
from util import bits_equal

pytestmark = pytest.mark.gpu

NAMES = ("gmf_s1_v2", "gmf_rs2_v2", "sarwing_lut_cmodms1ahw", "nc_lut_cmodms1ahw")
RULE_NAMES = NAMES[:3]  # one name per kernel rule
WSPD_NAMES = ("dsig_wspd_rs2_v3", "dsig_wspd_s1_ew_rec_v3", "dsig_wspd_rcm_v3")
# 37 x 203: odd sample count (scalar tail, no vector stores), lines no multiple of XSW_NESZ_LINES; 8 x 512: the aligned vector
# path; 1 x 1; 0 x 5: empty
SHAPES = [(37, 203), (8, 512), (1, 1), (0, 5)]
RTOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-6}


def _host(fn, *args, **kw):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def _rasters(shape, dtype, seed=0, nan_inc_column=False):
    """(noise, inc, sigma0) of one dtype.  Rasters large enough hold: sigma0 with negative values, 0, NaN and +inf; noise with
    0, NaN and one all-NaN line (which the flattening fills with the column means); incidence with NaN pixels and, on request,
    one all-NaN column -- its NaN abscissa poisons every line's fit, in the reference too, so the flattened noise is all NaN:
    the fused tests run with and without it."""
    rng = np.random.default_rng(100 + seed)
    lines, samples = shape
    inc = 20.0 + 25.0 * np.arange(samples) / max(samples, 1) + rng.normal(0, 1e-3, shape)
    noise = 10.0 ** (-2.2 - 0.02 * (inc - 20.0)) * rng.uniform(0.9, 1.1, shape)
    sigma0 = noise * rng.uniform(0.05, 50.0, shape)  # r**8 stays normal in float32
    if lines >= 8 and samples >= 16:
        neg = rng.random(shape) < 0.1
        sigma0[neg] = -sigma0[neg]
        sigma0[1, 3], sigma0[2, 5], sigma0[3, 7] = 0.0, np.nan, np.inf
        sigma0[rng.random(shape) < 0.01] = np.nan
        noise[1, 4], noise[2, 6], noise[3, 7] = 0.0, np.nan, 0.0
        noise[rng.random(shape) < 0.01] = np.nan
        noise[5] = np.nan
        inc[rng.random(shape) < 0.01] = np.nan
        if nan_inc_column:
            inc[:, 9] = np.nan
    return noise.astype(dtype), inc.astype(dtype), sigma0.astype(dtype)


def _up(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(_dev(torch)) for a in arrays]


def _misaligned(torch, t):
    """A contiguous copy of `t` that starts one element off a 16-byte boundary: the `[1:]` view of a longer buffer."""
    off = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    off.copy_(t)
    assert off.data_ptr() % 16 == t.element_size() and off.is_contiguous()
    return off


def _assert_close(got, want, what, rtol=None, atol=0.0):
    """dtype and shape equal; NaN positions, infinities and zeros equal exactly; the other values within the tolerance.
    Returns the largest relative (absolute when atol is given) difference seen."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions"
    special = ~np.isfinite(want) | (want == 0) | ~np.isfinite(got) | (got == 0)
    assert np.array_equal(got[special], want[special], equal_nan=True), what + ": infinities / zeros"
    g, w = got[~special].astype(np.float64), want[~special].astype(np.float64)
    if not g.size:
        return 0.0
    err = np.abs(g - w) if atol else np.abs(g - w) / np.abs(w)
    worst = float(err.max())
    assert worst <= (atol if atol else RTOL[want.dtype] if rtol is None else rtol), (what, worst)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_get_dsig_on_device_tensors_against_the_reference(torch, gpu_ctx, name):
    """The golden inputs of the reference's get_dsig, float64 and cast to float32: dtypes as numpy's, values within the bounds."""
    from xsarsea_amd.windspeed import get_dsig
    d = golden("crosspol_prep.npz")
    for cast, key in ((np.float64, "dsig_"), (np.float32, "dsig32_")):
        inc, s, n = _up(torch, *(d[k].astype(cast) for k in ("dsig_inc", "dsig_sigma0_cr", "dsig_nesz_cr")))
        got = get_dsig(name, inc, s, n)
        assert isinstance(got, torch.Tensor) and got.is_cuda
        worst = _assert_close(got.cpu().numpy(), d[key + name], f"{name} {np.dtype(cast).name}")
        print(f"get_dsig {name} {np.dtype(cast).name} inputs -> {got.dtype}: max rel diff to the reference {worst:.3e}")


@pytest.mark.parametrize("name", WSPD_NAMES)
def test_get_dsig_wspd_on_device_tensors(torch, gpu_ctx, name):
    """Golden inputs against the reference's outputs; then overflowing exponentials, NaN and a broadcast host scalar against
    the host function."""
    from xsarsea_amd.windspeed import get_dsig_wspd
    d = golden("crosspol_prep.npz")
    u, snr = _up(torch, d["dsigw_U"], d["dsigw_SNR"])
    got = get_dsig_wspd(name, u, snr)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    worst = _assert_close(got.cpu().numpy(), d[name], name, atol=1e-12)
    rng = np.random.default_rng(2)
    U = rng.uniform(0.0, 60.0, (9, 33))
    SNR = rng.uniform(-5.0, 25.0, (9, 33))
    U[0, :4] = [np.nan, 1e6, -1e6, 30.0]
    SNR[1, :3] = [np.nan, 1e9, -1e9]
    want = _host(get_dsig_wspd, name, U, SNR)
    t_u, t_snr = _up(torch, U, SNR)
    worst = max(worst, _assert_close(get_dsig_wspd(name, t_u, t_snr).cpu().numpy(), want, name + " special values", atol=1e-12))
    worst = max(worst, _assert_close(get_dsig_wspd(name, t_u, 3.0).cpu().numpy(), _host(get_dsig_wspd, name, U, 3.0), name + " scalar SNR", atol=1e-12))
    assert tuple(get_dsig_wspd(name, t_u[:0], t_snr[:0]).shape) == (0, 33)
    print(f"get_dsig_wspd {name}: max abs diff {worst:.3e}")


@pytest.mark.parametrize("shape", SHAPES)
def test_get_dsig_device_special_values_equal_the_host(torch, gpu_ctx, shape):
    """Every rule and every (sigma0, nesz) dtype pair on rasters with negative / zero / NaN / inf ratios and NaN incidence,
    against the host functions (pinned bitwise to the reference by test_oracle.py); host arrays and scalars mixed in."""
    from xsarsea_amd.windspeed import get_dsig
    worst = {}
    for dt_s in (np.float32, np.float64):
        for dt_n in (np.float32, np.float64):
            noise, inc, sigma0 = _rasters(shape, np.float64, seed=1, nan_inc_column=True)
            sigma0, inc, noise = sigma0.astype(dt_s), inc.astype(dt_s), noise.astype(dt_n)
            t_s, t_i, t_n = _up(torch, sigma0, inc, noise)
            for name in RULE_NAMES:
                want = _host(get_dsig, name, inc, sigma0, noise)
                got = get_dsig(name, t_i, t_s, t_n)
                assert got.is_cuda
                w = _assert_close(got.cpu().numpy(), want, f"{name} {shape} {np.dtype(dt_s).name}/{np.dtype(dt_n).name}")
                key = (name, want.dtype.name)
                worst[key] = max(worst.get(key, 0.0), w)
                if dt_s == dt_n and shape[0] > 1:  # a host incidence row and a scalar noise are broadcast and uploaded
                    row = inc[0]
                    w2 = _assert_close(get_dsig(name, row, t_s, float(noise[0, 0])).cpu().numpy(),
                                       _host(get_dsig, name, row, sigma0, float(noise[0, 0])), f"{name} {shape} broadcast")
                    worst[key] = max(worst[key], w2)
    for key, w in sorted(worst.items()):
        print(f"get_dsig {key[0]} -> {key[1]} {shape}: max rel diff to the host function {w:.3e}")


def test_get_dsig_device_misaligned_rasters(torch, gpu_ctx):
    """Rasters that start one element off a 16-byte boundary: the element-wise loads give the bits of the vector loads."""
    from xsarsea_amd.windspeed import get_dsig
    for dt in (np.float32, np.float64):
        noise, inc, sigma0 = _rasters((8, 512), dt, seed=2, nan_inc_column=True)
        t_n, t_i, t_s = _up(torch, noise, inc, sigma0)
        o_n, o_i, o_s = (_misaligned(torch, t) for t in (t_n, t_i, t_s))
        for name in RULE_NAMES:
            assert bits_equal(get_dsig(name, o_i, o_s, o_n).cpu().numpy(), get_dsig(name, t_i, t_s, t_n).cpu().numpy()), (name, dt)


def _unfused(name, t_i, t_s, t_n):
    from xsarsea_amd.windspeed import get_dsig, nesz_flattening
    return get_dsig(name, t_i, t_s, nesz_flattening(t_n, t_i))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES + ["misaligned"])
def test_fused_equals_the_two_calls_bit_for_bit(torch, gpu_ctx, shape, dtype):
    """dsig_from_nesz on device tensors == get_dsig(name, inc, sigma0, nesz_flattening(noise, inc)) exactly, for every rule;
    out_dtype=float32 == .to(float32) of that.  No tolerance: the flattened noise is the same expression in both."""
    from xsarsea_amd.windspeed import dsig_from_nesz
    for nan_col in (False, True):
        noise, inc, sigma0 = _rasters((8, 512) if shape == "misaligned" else shape, dtype, seed=3, nan_inc_column=nan_col)
        t_n, t_i, t_s = _up(torch, noise, inc, sigma0)
        if shape == "misaligned":
            t_n, t_i, t_s = (_misaligned(torch, t) for t in (t_n, t_i, t_s))
        for name in NAMES:
            want = _unfused(name, t_i, t_s, t_n)
            got = dsig_from_nesz(name, t_i, t_s, t_n)
            got32 = dsig_from_nesz(name, t_i, t_s, t_n, out_dtype=np.float32)
            assert got.is_cuda and got.dtype == torch.float64 and got32.dtype == torch.float32 and got.shape == want.shape
            assert bits_equal(got.cpu().numpy(), want.cpu().numpy()), (name, shape, dtype, nan_col)
            assert bits_equal(got32.cpu().numpy(), want.to(torch.float32).cpu().numpy()), (name, shape, dtype, nan_col, "float32 store")
            if want.numel():
                w = want.cpu().numpy()
                assert np.isnan(w).all() if nan_col and want.numel() > 64 else np.isfinite(w).any()


@pytest.mark.parametrize("name", NAMES)
def test_fused_against_the_reference(torch, gpu_ctx, name):
    """The golden float64 noise rasters: within (p / 2) x 1e-10 (the flattening's documented agreement for float64 rasters) of
    get_dsig on the reference's flattened noise, p the rule's exponent (c, 8, or 2 x 4); an all-NaN noise raster gives NaN."""
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig
    from xsarsea_amd.windspeed.utils import _S1_V2_EXPONENT
    d = golden("crosspol_prep.npz")
    noise, inc = d["nesz_noise"], d["nesz_inc"]
    rng = np.random.default_rng(12)
    sigma0 = d["nesz_flat"] * rng.uniform(0.05, 50.0, noise.shape)
    sigma0[rng.random(noise.shape) < 0.1] *= -1.0
    sigma0[2, 3], sigma0[4, 5] = 0.0, np.nan
    want = _host(get_dsig, name, inc, sigma0, d["nesz_flat"])
    got = dsig_from_nesz(name, *_up(torch, inc, sigma0, noise)).cpu().numpy()
    if name == "gmf_s1_v2":
        rate, centre, floor, span = _S1_V2_EXPONENT
        p = _host(lambda x: floor + span / (1 + np.exp(-rate * (x - centre))), inc)
    else:
        p = np.full(noise.shape, 8.0)
    assert got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want))
    special = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(got[special], want[special], equal_nan=True)
    rel = np.abs(got[~special] - want[~special]) / np.abs(want[~special])
    print(f"dsig_from_nesz {name}: max rel diff to get_dsig on the reference's flattened noise {rel.max():.3e} "
          f"(bound {p[~special].min() / 2 * 1e-10:.2e} .. {p[~special].max() / 2 * 1e-10:.2e})")
    assert np.isfinite(rel).all() and (rel <= p[~special] / 2 * 1e-10).all()
    nan_noise, nan_inc = np.full((3, 8), np.nan), inc[:3, :8]
    want_nan = _host(get_dsig, name, nan_inc, sigma0[:3, :8], d["nesz_flat_allnan"])
    got_nan = dsig_from_nesz(name, *_up(torch, nan_inc, sigma0[:3, :8].copy(), nan_noise)).cpu().numpy()
    assert np.isnan(want_nan).all() and np.isnan(got_nan).all()


def test_host_memory_entries_equal_the_device_rasters(torch, gpu_ctx):
    """xsw_dsig and xsw_dsig_flat with XSW_MEM_HOST (upload, kernels, download) == the device-raster calls, bit for bit."""
    from xsarsea_amd import _lib
    shape = (37, 203)
    p = lambda a: a.ctypes.data
    for dt, xdt in ((np.float32, _lib.XSW_F32), (np.float64, _lib.XSW_F64)):
        noise, inc, sigma0 = _rasters(shape, dt, seed=4)
        t_n, t_i, t_s = _up(torch, noise, inc, sigma0)
        for rule in (0, 1, 2):
            d_el = torch.empty(shape, dtype=torch.float64 if rule == 0 or dt == np.float64 else torch.float32, device=_dev(torch))
            d_fl = torch.empty(shape, dtype=torch.float64, device=_dev(torch))
            d_fl32 = torch.empty(shape, dtype=torch.float32, device=_dev(torch))
            torch.cuda.synchronize()
            gpu_ctx.dsig_raw(rule, *shape, xdt, xdt, _lib.MEM_DEVICE, t_i.data_ptr() if rule == 0 else None, t_s.data_ptr(), t_n.data_ptr(), d_el.data_ptr())
            gpu_ctx.dsig_flat_raw(rule, *shape, xdt, _lib.XSW_F64, _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), d_fl.data_ptr())
            gpu_ctx.dsig_flat_raw(rule, *shape, xdt, _lib.XSW_F32, _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), d_fl32.data_ptr())
            gpu_ctx.synchronize()
            h_el = np.full(shape, 7.0, dtype=d_el.cpu().numpy().dtype)
            h_fl, h_fl32 = np.full(shape, 7.0), np.full(shape, 7.0, dtype=np.float32)
            gpu_ctx.dsig_raw(rule, *shape, xdt, xdt, _lib.MEM_HOST, p(inc) if rule == 0 else None, p(sigma0), p(noise), p(h_el))
            gpu_ctx.dsig_flat_raw(rule, *shape, xdt, _lib.XSW_F64, _lib.MEM_HOST, p(noise), p(inc), p(sigma0), p(h_fl))
            gpu_ctx.dsig_flat_raw(rule, *shape, xdt, _lib.XSW_F32, _lib.MEM_HOST, p(noise), p(inc), p(sigma0), p(h_fl32))
            assert bits_equal(h_el, d_el.cpu().numpy()) and np.isfinite(h_el).any(), (rule, dt)
            assert bits_equal(h_fl, d_fl.cpu().numpy()) and np.isfinite(h_fl).any(), (rule, dt)
            assert bits_equal(h_fl32, d_fl32.cpu().numpy()), (rule, dt)
    U, snr = np.linspace(0.0, 60.0, 77), np.linspace(-5.0, 25.0, 77)
    t_u, t_snr = _up(torch, U, snr)
    d_w, h_w = torch.empty(77, dtype=torch.float64, device=_dev(torch)), np.full(77, 7.0)
    torch.cuda.synchronize()
    gpu_ctx.dsig_wspd_raw(1, 77, _lib.MEM_DEVICE, t_u.data_ptr(), t_snr.data_ptr(), d_w.data_ptr())
    gpu_ctx.synchronize()
    gpu_ctx.dsig_wspd_raw(1, 77, _lib.MEM_HOST, p(U), p(snr), p(h_w))
    assert bits_equal(h_w, d_w.cpu().numpy())


def test_fused_call_on_a_user_stream(torch, gpu_ctx, delay_cycles):
    """dsig_from_nesz under `with torch.cuda.stream(P)`, inputs produced on P behind the delay (the buffers hold another valid
    raster until then): == the synchronised result, bit for bit, and the call returned while the producer was in flight."""
    from xsarsea_amd.windspeed import dsig_from_nesz
    shape = (150, 320)
    real, decoy = _rasters(shape, np.float32, seed=5), _rasters(shape, np.float32, seed=6)
    ref = dsig_from_nesz("gmf_s1_v2", *_up(torch, real[1], real[2], real[0]))
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    P = torch.cuda.Stream(device=_dev(torch))
    with torch.cuda.stream(P):
        pairs = _staged(torch, real, decoy)
        done = _held_back(torch, P, delay_cycles, pairs)
        out = dsig_from_nesz("gmf_s1_v2", pairs[1][0], pairs[2][0], pairs[0][0])
        _in_flight(done)
        got, = _read_back(torch, P, out)
    assert np.isfinite(ref).any() and bits_equal(got, ref)


def test_two_fused_calls_back_to_back_reuse_the_scratch(torch, fresh_ctx):
    """Two xsw_dsig_flat calls of different shapes queued on one context without a synchronisation in between (the second
    grows the scratch, the third fits in it) == each alone on a context of its own."""
    from xsarsea_amd import _lib
    shapes = [(8, 512), (37, 203), (8, 512)]
    ins = [_up(torch, *_rasters(s, np.float32, seed=7 + k)) for k, s in enumerate(shapes)]
    outs = [torch.empty(s, dtype=torch.float64, device=_dev(torch)) for s in shapes]
    torch.cuda.synchronize()
    for (t_n, t_i, t_s), o, s in zip(ins, outs, shapes):
        fresh_ctx.dsig_flat_raw(0, *s, _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), o.data_ptr())
    fresh_ctx.synchronize()
    for (t_n, t_i, t_s), o, s in zip(ins, outs, shapes):
        alone = _lib.Context(0)
        try:
            ref = torch.empty(s, dtype=torch.float64, device=_dev(torch))
            torch.cuda.synchronize()
            alone.dsig_flat_raw(0, *s, _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), ref.data_ptr())
            alone.synchronize()
        finally:
            alone.close()
        assert np.isfinite(ref.cpu().numpy()).any() and bits_equal(o.cpu().numpy(), ref.cpu().numpy()), s


def test_errors_leave_the_context_usable(torch, gpu_ctx):
    from xsarsea_amd import _lib
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig
    shape = (8, 512)
    noise, inc, sigma0 = _rasters(shape, np.float32, seed=9)
    t_n, t_i, t_s = _up(torch, noise, inc, sigma0)
    out = torch.empty(shape, dtype=torch.float64, device=_dev(torch))
    torch.cuda.synchronize()
    f32, dev = _lib.XSW_F32, _lib.MEM_DEVICE
    with pytest.raises(_lib.XswError, match="needs inc"):  # S1_V2 without incidence
        gpu_ctx.dsig_raw(0, *shape, f32, f32, dev, None, t_s.data_ptr(), t_n.data_ptr(), out.data_ptr())
    for rule in (-1, 3):  # a rule out of range
        with pytest.raises(_lib.XswError, match="unknown rule"):
            gpu_ctx.dsig_raw(rule, *shape, f32, f32, dev, t_i.data_ptr(), t_s.data_ptr(), t_n.data_ptr(), out.data_ptr())
        with pytest.raises(_lib.XswError, match="unknown rule"):
            gpu_ctx.dsig_flat_raw(rule, *shape, f32, _lib.XSW_F64, dev, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), out.data_ptr())
        with pytest.raises(_lib.XswError, match="unknown rule"):
            gpu_ctx.dsig_wspd_raw(rule, 8, dev, out.data_ptr(), out.data_ptr(), out.data_ptr())
    with pytest.raises(_lib.XswError):  # a dtype that is none
        gpu_ctx.dsig_raw(1, *shape, 5, f32, dev, None, t_s.data_ptr(), t_n.data_ptr(), out.data_ptr())
    with pytest.raises(_lib.XswError):  # a NULL raster
        gpu_ctx.dsig_flat_raw(1, *shape, f32, _lib.XSW_F64, dev, t_n.data_ptr(), None, t_s.data_ptr(), out.data_ptr())
    with pytest.raises(ValueError):  # shapes that do not broadcast
        get_dsig("gmf_rs2_v2", t_i, t_s[:, :100], t_n)
    with pytest.raises(ValueError):
        dsig_from_nesz("gmf_rs2_v2", t_i, t_s[:5], t_n)
    with pytest.raises(ValueError):  # the host route's message, before any device call
        get_dsig("nope", t_i, t_s, t_n)
    with pytest.raises(IndexError):
        dsig_from_nesz("gmf_rs2_v2", t_i[0], t_s[0], t_n[0])
    # the context still works
    gpu_ctx.dsig_flat_raw(1, *shape, f32, _lib.XSW_F64, dev, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), out.data_ptr())
    gpu_ctx.synchronize()
    assert bits_equal(out.cpu().numpy(), _unfused("gmf_rs2_v2", t_i, t_s, t_n).cpu().numpy())
