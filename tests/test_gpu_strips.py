"""GPU: the strip kernels beyond one line per workgroup, the grid-stride kernels beyond one pass per thread.

k_detrend and k_dsig_flat stream down a block of lines with four lines in flight per lane, a one-line tail loop behind that
unrolled loop and a short last block; at the small rasters of the other modules every workgroup holds ONE line, so only the
tail loop runs there, once.  The rasters of tests/strip_shapes.py give each workgroup six lines (one unrolled group + two
tail lines; the last workgroup fewer), with 16-byte / pair accesses and element-wise; tests/test_host_plan.py keeps them
there.  k_gmf_eval and k_dsig_wspd are capped at 4096 workgroups of 256 threads: n = 2 * 4096 * 256 + 257 sends every thread
through its loop twice and the first 257 a third time; so does k_expand (256 * 16 workgroups) on as many grid codes, and
k_grad_area (65 536 workgroups) at 16 797 700 outputs.  k_grad_keep is a strip kernel on the OUTPUT grid: the keep entries of
tests/strip_shapes.py give each workgroup five or six output rows (three in the last), one entry per instantiation.

References and bounds:
  k_detrend     numpy's IEEE quotient sigma0.astype(float64) / ratio[None, :], rounded once with .astype(float32) for float32
                outputs; no tolerance (float64 bit for bit, float32 bit for bit off NaN and NaN by position).
  k_dsig_flat   (1) the two calls it fuses, get_dsig on nesz_flattening, whose kernels (k_nesz_eval, k_dsig) have no unrolled
                line loop: no tolerance.  (2) get_dsig on the oracle's flattened noise: (p / 2) x 1e-10 relative, p the rule's
                exponent, as tests/test_gpu_dsig.py::test_fused_against_the_reference.
  k_gmf_eval    the same inputs in slices of at most 4096 * 256 elements (one pass per thread): no tolerance; the oracle's
                formulas to 1e-13 relative as tests/test_gpu_api.py::test_forward_gmf_device.
  k_dsig_wspd   the host function, 1e-12 absolute (values in [0, 1]) as tests/test_gpu_dsig.py.
  k_grad_keep   masked_ref.keep_blocks on the inputs of tests/keep_cases.py: no tolerance (uint8 masks).
  k_expand      the same codes in slices of at most 4096 * 256, and the host expansion (expand_host): no tolerance, on the bits.
  k_grad_area   gradients_ref.area: array_equal, as tests/test_gpu_gradients.py::test_area."""
import functools

import numpy as np
import pytest

import keep_cases
import strip_shapes
from test_gpu_dsig import NAMES, WSPD_NAMES, _assert_close, _host, _rasters

pytestmark = pytest.mark.gpu

SENTINEL = -7.0  # what the outputs hold before a call: finite, so a pixel that is never stored differs from its reference
ONE_PASS = 4096 * 256  # elements the grid-stride kernels cover with one pass per thread
N_STRIDE = 2 * ONE_PASS + 257


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _up(*arrays):
    torch, dev = _torch()
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _lines_of(bad):
    """For a failure message: how many pixels of a boolean raster are set, and the first lines that hold one."""
    rows = np.flatnonzero(np.asarray(bad).any(axis=1))
    return f"{int(np.asarray(bad).sum())} pixels differ, first lines {rows[:12].tolist()}"


# ------------------------------------------------------------------------------------------------------------ k_detrend
def _detrend_sigma0(key, dtype):
    """Log-uniform sigma0 as tests/test_gpu_kernel.py::test_detrend_kernel; its eight special values sit in every probe line
    (each position of an unrolled group, the tail lines, the last block) at the first columns, across a quad boundary in the
    second column strip, and in the last columns (the partial quad of the element-wise raster)."""
    lines, samples = strip_shapes.shape(key)
    rng = np.random.default_rng(50)
    s = (10 ** rng.uniform(-6, 1, (lines, samples))).astype(dtype)
    fi = np.finfo(dtype)
    special = np.array([0.0, np.inf, -np.inf, np.nan, fi.tiny, -1.5, fi.max, fi.smallest_subnormal], dtype=dtype)
    for k, line in enumerate(strip_shapes.probe_lines(key)):
        for c0 in (0, 4093, samples - 8):
            s[line, c0:c0 + 8] = np.roll(special, k)
    return s


def _ratio_rows(samples):
    """An ordinary row (fused-multiply path) and the same row with one divisor whose significand is all ones (the host then
    launches the true division for the whole raster)."""
    ratio = 10 ** np.random.default_rng(51).uniform(-3, 3, samples)
    forced = ratio.copy()
    forced[5] = np.float64(2.0) - np.finfo(np.float64).eps
    return {"fused multiply": ratio, "true division": forced}


def _check_detrend(out, ref, what):
    """float64: every pixel bit for bit.  float32: bit for bit where the reference is not NaN, NaN where it is."""
    assert out.dtype == ref.dtype and out.shape == ref.shape, what
    if ref.dtype == np.float64:
        bad = out.view(np.int64) != ref.view(np.int64)
    else:
        nan = np.isnan(ref)
        bad = np.where(nan, ~np.isnan(out), out.view(np.int32) != ref.view(np.int32))
    assert not bad.any(), what + ": " + _lines_of(bad)


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("in_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("key", ["detrend_vec", "detrend_elem"])
def test_detrend_with_several_lines_per_block(gpu_ctx, key, in_dtype, route):
    """out = sigma0 / ratio[sample] at six lines per workgroup (five in the last): float32 and float64 rasters into float32 and
    float64 outputs, the fused-multiply and the true-division instantiation, on device tensors (one launch over the whole
    raster; the outputs start as a sentinel) and on host arrays (line chunks through the workers: chunks of at most 4 Mpx, so
    that route checks the cut at these sizes while its workgroups hold one line)."""
    from xsarsea_amd import _lib
    torch, dev = _torch()
    lines, samples = strip_shapes.shape(key)
    assert strip_shapes.SHAPES[key].grid[2] > 4
    s = _detrend_sigma0(key, in_dtype)
    xdt = {np.float32: _lib.XSW_F32, np.float64: _lib.XSW_F64}
    t_s = _up(s)[0] if route == "device" else None
    for path, ratio in _ratio_rows(samples).items():
        with np.errstate(all="ignore"):
            ref64 = s.astype(np.float64) / ratio[None, :]
            refs = {np.float64: ref64, np.float32: ref64.astype(np.float32)}
        assert np.isinf(refs[np.float32]).sum() > np.isinf(ref64).sum() or in_dtype == np.float64  # the float32 store overflows
        for out_dtype in (np.float32, np.float64):
            if route == "device":
                t_o = torch.full((lines, samples), SENTINEL, dtype=torch.float32 if out_dtype == np.float32 else torch.float64, device=dev)
                torch.cuda.synchronize()
                gpu_ctx.detrend_raw(lines, samples, xdt[in_dtype], xdt[out_dtype], _lib.MEM_DEVICE, t_s.data_ptr(), ratio, t_o.data_ptr())
                gpu_ctx.synchronize()
                out = t_o.cpu().numpy()
                del t_o
            else:
                out = gpu_ctx.detrend_host(s, ratio, out_dtype=out_dtype)
            _check_detrend(out, refs[out_dtype], f"{key} {np.dtype(in_dtype).name} -> {np.dtype(out_dtype).name}, {path}, {route} route")
    del t_s
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- k_dsig_flat
@functools.lru_cache(maxsize=2)
def _dsig_rasters64(key):
    """(noise, inc, sigma0) of tests/test_gpu_dsig.py's recipe in float64, without the all-NaN incidence column; read-only.
    The recipe draws in float64 and casts last, and the column is its last step: see _dsig_rasters."""
    out = _rasters(strip_shapes.shape(key), np.float64, seed=20)
    for a in out:
        a.setflags(write=False)
    return out


def _dsig_rasters(key, dtype, nan_col):
    """What _rasters(shape, dtype, seed=20, nan_inc_column=nan_col) returns, from the one float64 draw of the shape."""
    noise, inc, sigma0 = _dsig_rasters64(key)
    if nan_col:
        inc = inc.copy()
        inc[:, 9] = np.nan
    return noise.astype(dtype), inc.astype(dtype), sigma0.astype(dtype)


def _same_bits(torch, got, want):
    """On the device, through integer views: equal bits, or NaN in both.  Returns the raster of differing pixels."""
    it = torch.int64 if got.dtype == torch.float64 else torch.int32
    assert got.dtype == want.dtype and got.shape == want.shape
    return ~((got.view(it) == want.view(it)) | (torch.isnan(got) & torch.isnan(want)))


@pytest.mark.parametrize("nan_col", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("key", ["dsig_flat_vec", "dsig_flat_elem"])
def test_fused_dsig_with_several_lines_per_block_equals_the_two_calls(gpu_ctx, key, dtype, nan_col):
    """dsig_from_nesz at six lines per workgroup (three in the last) == get_dsig(name, inc, sigma0, nesz_flattening(noise, inc))
    bit for bit, every name, float64 and float32 stores; with the all-NaN incidence column every pixel is NaN.  The recipe puts
    negative / zero / NaN / inf sigma0, NaN noise pixels and an all-NaN noise line into the rasters."""
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig, nesz_flattening
    torch, _dev = _torch()
    assert strip_shapes.SHAPES[key].grid[2] > 4
    t_n, t_i, t_s = _up(*_dsig_rasters(key, dtype, nan_col))
    flat = nesz_flattening(t_n, t_i)
    for name in NAMES:
        want = get_dsig(name, t_i, t_s, flat)
        got = dsig_from_nesz(name, t_i, t_s, t_n)
        got32 = dsig_from_nesz(name, t_i, t_s, t_n, out_dtype=np.float32)
        assert got.dtype == torch.float64 and got32.dtype == torch.float32 and want.dtype == torch.float64
        for g, w, store in ((got, want, "float64"), (got32, want.to(torch.float32), "float32")):
            bad = _same_bits(torch, g, w)
            assert not bool(bad.any()), f"{name} {key} {np.dtype(dtype).name} {store} store, NaN column {nan_col}: " + _lines_of(bad.cpu().numpy())
        if nan_col:
            assert bool(torch.isnan(got).all()) and bool(torch.isnan(got32).all()), name
        else:
            assert bool(torch.isfinite(got).any()) and bool(torch.isinf(got).any()) and bool(torch.isnan(got).any()), name
        del want, got, got32
    del t_n, t_i, t_s, flat
    torch.cuda.empty_cache()


@pytest.mark.parametrize("key", ["dsig_flat_vec", "dsig_flat_elem"])
def test_fused_dsig_with_several_lines_per_block_against_the_reference(gpu_ctx, key):
    """Float64 rasters without the NaN column against get_dsig on the ORACLE's flattened noise (its per-line polyfit, once per
    shape): NaN positions, infinities and zeros equal, the rest within (p / 2) x 1e-10, p the rule's exponent.
    Measured on the MI355X, largest relative difference (the same to two digits at both rasters): gmf_s1_v2 2.1e-14 (bound
    7.3e-11 where p is smallest), gmf_rs2_v2 5.8e-14, sarwing_lut_cmodms1ahw and nc_lut_cmodms1ahw 5.8e-14 (bound 4e-10)."""
    from oracle import crosspol
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig
    from xsarsea_amd.windspeed.utils import _S1_V2_EXPONENT
    torch, _dev = _torch()
    noise, inc, sigma0 = _dsig_rasters(key, np.float64, False)
    flat_ref = _host(crosspol.nesz_flattening, noise, inc)
    t_n, t_i, t_s = _up(noise, inc, sigma0)
    for name in NAMES:
        want = _host(get_dsig, name, inc, sigma0, flat_ref)
        got = dsig_from_nesz(name, t_i, t_s, t_n).cpu().numpy()
        if name == "gmf_s1_v2":
            rate, centre, floor, span = _S1_V2_EXPONENT
            p = _host(lambda x: floor + span / (1 + np.exp(-rate * (x - centre))), inc)
        else:
            p = np.full(noise.shape, 8.0)
        assert got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)), name + ": NaN positions"
        special = ~np.isfinite(want) | (want == 0)
        assert np.array_equal(got[special], want[special], equal_nan=True), name + ": infinities / zeros"
        rel = np.abs(got[~special] - want[~special]) / np.abs(want[~special])
        print(f"dsig_from_nesz {name} {key}: max rel diff to get_dsig on the oracle's flattened noise {rel.max():.3e} "
              f"(bound {p[~special].min() / 2 * 1e-10:.2e} .. {p[~special].max() / 2 * 1e-10:.2e})")
        assert np.isfinite(rel).all() and (rel <= p[~special] / 2 * 1e-10).all(), name
    del t_n, t_i, t_s
    torch.cuda.empty_cache()


def test_fused_dsig_host_entry_with_several_lines_per_block(gpu_ctx):
    """xsw_dsig_flat with XSW_MEM_HOST (upload, one launch over the whole raster, download) == the device-raster call, bit for
    bit, at the raster with pair accesses (the unrolled loop): every rule, float32 and float64 rasters and stores."""
    from xsarsea_amd import _lib
    from util import bits_equal
    torch, dev = _torch()
    key = "dsig_flat_vec"
    shape = strip_shapes.shape(key)
    p = lambda a: a.ctypes.data
    for dt, xdt in ((np.float32, _lib.XSW_F32), (np.float64, _lib.XSW_F64)):
        noise, inc, sigma0 = _dsig_rasters(key, dt, False)
        t_n, t_i, t_s = _up(noise, inc, sigma0)
        for rule in (0, 1, 2):
            for odt, xodt, tdt in ((np.float64, _lib.XSW_F64, torch.float64), (np.float32, _lib.XSW_F32, torch.float32)):
                d_out = torch.full(shape, SENTINEL, dtype=tdt, device=dev)
                torch.cuda.synchronize()
                gpu_ctx.dsig_flat_raw(rule, *shape, xdt, xodt, _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), d_out.data_ptr())
                gpu_ctx.synchronize()
                h_out = np.full(shape, SENTINEL, dtype=odt)
                gpu_ctx.dsig_flat_raw(rule, *shape, xdt, xodt, _lib.MEM_HOST, p(noise), p(inc), p(sigma0), p(h_out))
                want = d_out.cpu().numpy()
                assert np.isfinite(want).any() and not (want == SENTINEL).any(), (rule, dt, odt)
                assert bits_equal(h_out, want), (rule, dt, odt)
                del d_out
        del t_n, t_i, t_s
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------- k_gmf_eval, k_dsig_wspd
@functools.lru_cache(maxsize=1)
def _gmf_inputs():
    rng = np.random.default_rng(52)
    out = rng.uniform(16, 66, N_STRIDE), rng.uniform(0, 1, N_STRIDE), rng.uniform(-360, 360, N_STRIDE)
    for a in out:
        a.setflags(write=False)
    return out


def _gmf_case(name):
    """(inc, wspd, phi or None) of N_STRIDE elements for one GMF: its own wind range, a dense sweep through the low-wind
    branches in each of the three passes, NaN in the second and the third pass."""
    from oracle import gmf as ogmf
    _f, _pol, wr, pr = ogmf.GMFS[name]
    inc, w01, phi = _gmf_inputs()
    wspd = wr[0] + (wr[1] - wr[0]) * w01
    for at in (0, ONE_PASS + 3, 2 * ONE_PASS + 1):
        m = min(1000, N_STRIDE - at)
        wspd[at:at + m] = np.linspace(wr[0], wr[1], 1000)[:m]
    inc = inc.copy()
    inc[ONE_PASS + 5000], wspd[2 * ONE_PASS + 250] = np.nan, np.nan
    return inc, wspd, (phi if pr is not None else None)


def _all_gmfs():
    from oracle import gmf as ogmf
    return sorted(ogmf.GMFS)


@pytest.mark.parametrize("name", _all_gmfs())
def test_gmf_eval_beyond_one_pass_per_thread(gpu_ctx, name):
    """One call over N_STRIDE elements (two passes of the grid-stride loop for every thread, a third for 257 of them) == the
    same elements evaluated in slices of one pass each, bit for bit; gmf_cmod5n and gmf_s1_v2 also against the oracle (measured
    on the MI355X: 4.0e-15 and 3.0e-15 relative, bound 1e-13)."""
    from oracle import gmf as ogmf
    from util import bits_equal
    from xsarsea_amd import _lib
    assert len(_lib.GMF_IDS) == 13 and set(_lib.GMF_IDS) == set(ogmf.GMFS)
    inc, wspd, phi = _gmf_case(name)
    gid = _lib.GMF_IDS[name]
    whole = gpu_ctx.gmf_eval(gid, inc, wspd, phi)
    parts = [gpu_ctx.gmf_eval(gid, inc[a:a + ONE_PASS], wspd[a:a + ONE_PASS], None if phi is None else phi[a:a + ONE_PASS])
             for a in range(0, N_STRIDE, ONE_PASS)]
    assert [len(q) for q in parts] == [ONE_PASS, ONE_PASS, 257]
    sliced = np.concatenate(parts)
    assert np.isfinite(whole[ONE_PASS:]).any() and np.isnan(whole[ONE_PASS + 5000]) and np.isnan(whole[2 * ONE_PASS + 250])
    differ = np.flatnonzero(~((whole == sliced) | (np.isnan(whole) & np.isnan(sliced))))
    assert bits_equal(whole, sliced), f"{name}: {differ.size} elements differ, first {differ[:8].tolist()}"
    if name in ("gmf_cmod5n", "gmf_s1_v2"):
        with np.errstate(all="ignore"):
            ref = ogmf.GMFS[name][0](inc, wspd, phi)
        assert np.array_equal(np.isnan(whole), np.isnan(ref)), name
        ok = np.isfinite(ref) & (ref != 0)
        worst = np.max(np.abs(whole[ok] - ref[ok]) / np.abs(ref[ok]))
        print(f"{name}: max rel diff to the oracle over {N_STRIDE} elements {worst:.3e} (bound 1e-13)")
        assert worst < 1e-13, name


@pytest.mark.parametrize("name", WSPD_NAMES)
def test_get_dsig_wspd_beyond_one_pass_per_thread(gpu_ctx, name):
    """get_dsig_wspd on device tensors of N_STRIDE elements against the host function, 1e-12 absolute; NaN and overflowing
    exponentials in the second and the third pass.  Measured on the MI355X: 2.2e-16 for each of the three rules."""
    from xsarsea_amd.windspeed import get_dsig_wspd
    torch, _dev = _torch()
    rng = np.random.default_rng(53)
    U, SNR = rng.uniform(0.0, 60.0, N_STRIDE), rng.uniform(-5.0, 25.0, N_STRIDE)
    for at in (ONE_PASS + 7, 2 * ONE_PASS + 100):
        U[at:at + 4] = [np.nan, 1e6, -1e6, 30.0]
        SNR[at + 4:at + 7] = [np.nan, 1e9, -1e9]
    want = _host(get_dsig_wspd, name, U, SNR)
    assert np.isnan(want[ONE_PASS:]).sum() == 4 and (want[2 * ONE_PASS:] > 0).any()
    t_u, t_snr = _up(U, SNR)
    got = get_dsig_wspd(name, t_u, t_snr)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    worst = _assert_close(got.cpu().numpy(), want, name, atol=1e-12)
    print(f"get_dsig_wspd {name}: max abs diff over {N_STRIDE} elements {worst:.3e} (bound 1e-12)")


# ---------------------------------------------------------------------------------------------------------- k_grad_keep
def _rows_of(bad, key):
    """For a failure message: the output rows that differ, as (row, workgroup row, row within it)."""
    rpb = strip_shapes.SHAPES[key].grid[2]
    rows = np.flatnonzero(np.asarray(bad).any(axis=1))
    return f"{int(np.asarray(bad).sum())} outputs differ, first rows (row, workgroup row, u) {[(int(y), int(y) // rpb, int(y) % rpb) for y in rows[:12]]}"


@pytest.mark.parametrize("key", keep_cases.KEYS)
def test_keep_mask_with_several_rows_per_block(gpu_ctx, key):
    """gradients.keep_mask at five or six output rows per workgroup (three in the last), one entry of tests/strip_shapes.py per
    instantiation of k_grad_keep, with and without and_with, numpy in -> numpy out and tensor in -> tensor out: bit-equal to
    masked_ref.keep_blocks.  The inputs are tests/keep_cases.py's: in every row of the second workgroup row and of the last one
    single elements decide blocks, at every row, lane and byte of a block in turn (NaN, -inf, one ulp below the threshold, the
    threshold itself; a lone 0x00 among 0x01, 0x80, 0xFF), and and_with holds lone zeros there.  Before each tensor call the
    allocator's free block of the output's size is filled with 7, so an output row that is never stored shows.  keep_f64_b2 runs
    once more as a device view whose base is 8 bytes off a 16-byte boundary, the other way into <double, 8, 0>."""
    import masked_ref as mr
    from xsarsea_amd import gradients
    torch, dev = _torch()
    e = strip_shapes.SHAPES[key]
    c = keep_cases.case(key)
    gx, gy, rpb, last = e.grid
    Lo, So = e.lines // c.block, e.samples // c.block
    assert rpb > 4 and Lo == (gy - 1) * rpb + last
    probes = strip_shapes.probe_lines(key)
    print(f"{key}: k_grad_keep<{e.inst[0]}, {e.inst[1]}, {e.inst[2]}> on {Lo} x {So} outputs, (gx, gy, rpb, last) = {e.grid}; probe rows "
          f"{probes[0]}..{probes[rpb - 1]} (workgroup row 1, u = 0..{rpb - 1}) and {probes[rpb]}..{probes[-1]} (workgroup row {gy - 1}); "
          f"{len(c.bad)} blocks decided by one element, {len(c.holes)} lone zeros of and_with")
    wants = {False: mr.keep_blocks(c.src, c.block, c.threshold), True: mr.keep_blocks(c.src, c.block, c.threshold, and_with=c.and_with)}
    for with_aw in (False, True):
        got = gradients.keep_mask(c.src, threshold=c.threshold, block=c.block, and_with=c.and_with if with_aw else None)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (Lo, So)
        bad = got != wants[with_aw]
        print(f"{key} numpy route, and_with {with_aw}: {int(bad.sum())} outputs differ, {int(bad[probes].sum())} of them in the probe rows")
        assert not bad.any(), f"{key} numpy route, and_with {with_aw}: " + _rows_of(bad, key)
    t_src, t_aw = _up(c.src.copy(), c.and_with.copy())   # (the case's own arrays are read-only)
    for with_aw in (False, True):
        poison = torch.full((Lo, So), 7, dtype=torch.uint8, device=dev)
        del poison
        out = gradients.keep_mask(t_src, threshold=c.threshold, block=c.block, and_with=t_aw if with_aw else None)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (Lo, So)
        got = out.cpu().numpy()
        del out
        bad = got != wants[with_aw]
        print(f"{key} tensor route, and_with {with_aw}: {int(bad.sum())} outputs differ, {int(bad[probes].sum())} of them in the probe rows")
        assert not bad.any(), f"{key} tensor route, and_with {with_aw}: " + _rows_of(bad, key)
    if key == "keep_f64_b2":
        # the same raster as a view that starts 8 bytes off a 16-byte boundary: grad_keep falls back to <double, 8, 0>, here with
        # 2 x 2 blocks and two column strips
        room = torch.empty(t_src.numel() + 1, dtype=t_src.dtype, device=dev)
        view = room[1:].view(t_src.shape)
        view.copy_(t_src)
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        got = gradients.keep_mask(view, threshold=c.threshold, block=c.block, and_with=t_aw).cpu().numpy()
        bad = got != wants[True]
        print(f"{key} tensor route, base 8 bytes off, and_with True: {int(bad.sum())} outputs differ")
        assert not bad.any(), f"{key} tensor route, base 8 bytes off: " + _rows_of(bad, key)
        del room, view
    del t_src, t_aw
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- k_expand
EXPAND_ROUTES = ["co", "co+cross", "cross, no co output", "cross alone"]  # which of (code_co, code_cr, out_co, out_cr) a call is given
EXPAND_SENTINEL = complex(-7.0, -7.0)


def _expand_tables(request, which):
    """(co, cr) table dicts: the low-resolution pair (directions 0..180), or the small golden whose directions run 0..360."""
    from conftest import golden
    from util import lut_dicts, small_luts
    if which == "lowres":
        return lut_dicts(*request.getfixturevalue("lowres_luts"))
    return lut_dicts(*small_luts(golden("kernel_small_phi360_f64.npz")))


def _expand_codes(plane, n_wcr):
    """N_STRIDE co-pol and cross-pol codes made by hand, no inversion: uniformly random grid points of the table with the -phi
    bit on half of them, uniformly random cross-pol indices with XSW_CODE_PICK_CO on a quarter; then, at the start of each of
    the three passes, every special kind beside ordinary partners and beside each other (the co-pol wind a cross-pol code picks
    or scales may itself be NaN, (nan, 0) or foreign)."""
    from xsarsea_amd import _lib
    rng = np.random.default_rng(54)
    cc = rng.integers(0, plane, N_STRIDE).astype(np.uint32) | (rng.integers(0, 2, N_STRIDE).astype(np.uint32) << 30)
    ccr = rng.integers(0, n_wcr, N_STRIDE).astype(np.uint32) | np.where(rng.random(N_STRIDE) < 0.25, _lib.CODE_PICK_CO, 0).astype(np.uint32)
    sp_co = np.array([_lib.CODE_NAN, _lib.CODE_NAN_RE, plane, 0x3FFFFFFF, 0x40000000 | plane, 0x80000000, plane - 1, 0x40000000 | (plane - 1)], np.uint32)
    sp_cr = np.array([_lib.CODE_NAN_RE, _lib.CODE_NO_INDEX, n_wcr, _lib.CODE_PICK_CO | 5, _lib.CODE_PICK_CO | _lib.CODE_NO_INDEX, 0x80000001, _lib.CODE_NAN,
                      n_wcr - 1], np.uint32)
    starts = (100, ONE_PASS + 3, 2 * ONE_PASS + 1)
    for at in starts:
        cc[at:at + 8] = sp_co                       # each special co-pol code with a random cross-pol partner
        ccr[at + 8:at + 16] = sp_cr                 # each special cross-pol code with a random co-pol partner
        cc[at + 16:at + 24], ccr[at + 16:at + 24] = sp_co, sp_cr
        cc[at + 24:at + 32], ccr[at + 24:at + 32] = sp_co, np.roll(sp_cr, 3)
    assert starts[2] + 32 <= N_STRIDE
    return cc, ccr, starts


def _cbits(a):
    """The bits of a complex vector, one row per element."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64).reshape(a.size, -1)


@pytest.mark.parametrize("out_c", [np.complex64, np.complex128])
@pytest.mark.parametrize("tables", ["lowres", "phi360"])
def test_expand_codes_beyond_one_pass_per_thread(gpu_ctx, request, tables, out_c):
    """k_expand is capped at 256 * 16 workgroups of 256 threads: N_STRIDE codes send every thread through its grid-stride loop
    twice and the first 257 a third time.  On the bits: the device expansion of the whole array == the device expansion of the
    same codes in slices of at most one pass == the host expansion (which test_gpu_codes.py pins to the stored winds), for
    co-pol codes alone, co + cross, cross without a co-pol output and cross-pol codes alone, and co + cross once more through
    xsw_expand_codes_on_stream on a side stream.  Outputs start as a sentinel."""
    from test_host_plan import grid_cap
    from xsarsea_amd import _lib
    torch, dev = _torch()
    assert ONE_PASS == grid_cap("expand_codes_on", "expand") * 256 and N_STRIDE > 2 * ONE_PASS
    co, cr = _expand_tables(request, tables)
    gpu_ctx.upload_luts(co=co, cr=cr)
    plane, n_wcr = len(co["wspd"]) * len(co["phi"]), len(cr["wspd"])
    assert (co["phi"][-1] > 180.0) == (tables == "phi360") and n_wcr > 5
    cc, ccr, starts = _expand_codes(plane, n_wcr)
    t_cc, t_ccr = _up(cc.view(np.int32), ccr.view(np.int32))
    od = _lib.XSW_F32 if out_c == np.complex64 else _lib.XSW_F64
    cdt = torch.complex64 if out_c == np.complex64 else torch.complex128
    item = np.dtype(out_c).itemsize
    fresh = lambda: torch.full((N_STRIDE,), EXPAND_SENTINEL, dtype=cdt, device=dev)
    at = lambda t, a, size: None if t is None else t.data_ptr() + a * size
    hp = lambda a: None if a is None else a.ctypes.data
    side = torch.cuda.Stream(device=dev)
    for route in EXPAND_ROUTES + ["co+cross on a side stream"]:
        has_cc, has_cr = route != "cross alone", route != "co"
        want_co = route in ("co", "co+cross", "co+cross on a side stream")
        d_cc, d_cr = (t_cc if has_cc else None), (t_ccr if has_cr else None)
        whole = [fresh() if want_co else None, fresh() if has_cr else None]
        sliced = [fresh() if want_co else None, fresh() if has_cr else None]
        torch.cuda.synchronize()
        if route.endswith("side stream"):
            gpu_ctx.expand_codes_on_stream(side.cuda_stream, N_STRIDE, od, at(d_cc, 0, 4), at(d_cr, 0, 4), at(whole[0], 0, item), at(whole[1], 0, item))
            side.synchronize()
        else:
            gpu_ctx.expand_codes_raw(N_STRIDE, _lib.MEM_DEVICE, od, at(d_cc, 0, 4), at(d_cr, 0, 4), at(whole[0], 0, item), at(whole[1], 0, item))
        lengths = []
        for a in range(0, N_STRIDE, ONE_PASS):
            lengths.append(min(ONE_PASS, N_STRIDE - a))
            gpu_ctx.expand_codes_raw(lengths[-1], _lib.MEM_DEVICE, od, at(d_cc, a, 4), at(d_cr, a, 4), at(sliced[0], a, item), at(sliced[1], a, item))
        gpu_ctx.synchronize()
        assert lengths == [ONE_PASS, ONE_PASS, 257]
        host = [np.full(N_STRIDE, EXPAND_SENTINEL, out_c) if want_co else None, np.full(N_STRIDE, EXPAND_SENTINEL, out_c) if has_cr else None]
        gpu_ctx.expand_codes_raw(N_STRIDE, _lib.MEM_HOST, od, hp(cc if has_cc else None), hp(ccr if has_cr else None), hp(host[0]), hp(host[1]))
        for name, w, s, h in zip(("co", "cr"), whole, sliced, host):
            if w is None:
                continue
            w, s = w.cpu().numpy(), s.cpu().numpy()
            what = f"{tables} {np.dtype(out_c).name} {route}, {name}"
            for other, x in (("one-pass slices", s), ("the host expansion", h)):
                differ = np.flatnonzero((_cbits(w) != _cbits(x)).any(axis=1))
                print(f"{what}: {differ.size} of {N_STRIDE} elements differ from {other}")
                assert differ.size == 0, f"{what} against {other}: first {differ[:8].tolist()} (pass {(differ[:8] // ONE_PASS).tolist()})"
            assert not (h == EXPAND_SENTINEL).any(), what + ": an element was never written"
            for k, a in enumerate(starts):     # every pass holds winds, (nan, nan) and (nan, 0)
                seg = h[a:a + 4096]
                assert np.isfinite(seg.real).any() and (np.isnan(seg.real) & np.isnan(seg.imag)).any() and (np.isnan(seg.real) & (seg.imag == 0)).any(), (what, k)
        if route == "co+cross":
            picked = (ccr & _lib.CODE_PICK_CO) != 0
            assert picked[2 * ONE_PASS:].any() and (~picked[2 * ONE_PASS:]).any() and ((cc >> 30) == 1)[ONE_PASS:].any()
        del whole, sliced
    del t_cc, t_ccr
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- k_grad_area
AREA_ONE_PASS = 65536 * 256  # outputs k_grad_area covers with one pass per thread


def _area_scene(shape, factor, dtype, out_probes):
    """A small random block tiled over `shape` (cheap to build), then made unlike itself where it counts: the f x f inputs of
    every output of `out_probes` (flat output indices) get values found nowhere else, 1000 and up, and one input of the outputs
    next to the first, the middle and the last probe is NaN.  Returns (scene, flat indices of the outputs that are NaN)."""
    rng = np.random.default_rng(55)
    L, S = shape
    So = S // factor
    tile = rng.uniform(0.01, 1.0, (61, 67)).astype(dtype)
    s0 = np.tile(tile, (L // 61 + 1, S // 67 + 1))[:L, :S].copy()
    for k, o in enumerate(out_probes):
        Y, X = divmod(o, So)
        s0[Y * factor:(Y + 1) * factor, X * factor:(X + 1) * factor] = 1000.0 + 8.0 * k + np.arange(factor * factor).reshape(factor, factor)
    nan_at = [out_probes[0] + 5, out_probes[len(out_probes) // 2] + 5, out_probes[-1] - 5]
    for o in nan_at:
        Y, X = divmod(o, So)
        s0[Y * factor + factor - 1, X * factor] = np.nan
    return s0, nan_at


@pytest.mark.parametrize("factor", [2, 1])
def test_area_beyond_one_pass_per_thread(gpu_ctx, factor):
    """k_grad_area is capped at 65 536 workgroups of 256 threads.  factor 2: 8195 x 8201 float32 -> 4097 x 4100 = 16 797 700
    outputs, a remainder trimmed on both axes, 20 484 of them in the second pass.  factor 1 (the raw entry accepts it): 3 x
    5 592 491 = 65536 * 256 + 257 elements, the pure index walk.  array_equal with gradients_ref.area (the same float64 order,
    the same rounding), as test_gpu_gradients.py::test_area.  The scene is a tiled block, so the outputs around the end of the
    first pass, the last output and some inside the second pass hold values found nowhere else: no earlier stretch of the
    output equals the second pass, which a wrong stride would store.  One NaN before, one inside and one at the end of it."""
    import gradients_ref as ref
    from test_host_plan import grid_cap
    from xsarsea_amd import gradients
    assert AREA_ONE_PASS == grid_cap("xsw_grad_area", "grad_area") * 256
    shape = (8195, 8201) if factor == 2 else (3, 5592491)
    Lo, So = shape[0] // factor, shape[1] // factor
    n = Lo * So
    assert n == (16797700 if factor == 2 else AREA_ONE_PASS + 257) and n > AREA_ONE_PASS
    assert factor == 1 or (shape[0] % factor and shape[1] % factor)
    probes = [AREA_ONE_PASS - 4100, AREA_ONE_PASS - 1, AREA_ONE_PASS, AREA_ONE_PASS + 1] + [AREA_ONE_PASS + 17 + 37 * k for k in range(5)] + [n - 1]
    s0, nan_at = _area_scene(shape, factor, np.float32, probes)
    want = ref.area(s0, factor)
    flat = want.reshape(-1)
    assert want.shape == (Lo, So) and want.dtype == np.float32
    assert np.isnan(flat[nan_at]).all() and np.isnan(flat).sum() == 3 and nan_at[0] < AREA_ONE_PASS <= nan_at[1] < nan_at[2]
    for o in probes:  # found nowhere else: the second pass equals no earlier stretch of the output
        assert flat[o] >= 1000.0 and (flat == flat[o]).sum() == 1, o
    assert sum(o >= AREA_ONE_PASS for o in probes) >= 7
    out = gradients._area(s0, factor)
    assert out.dtype == np.float32 and out.shape == (Lo, So)
    differ = np.flatnonzero(~((out.reshape(-1) == flat) | (np.isnan(out.reshape(-1)) & np.isnan(flat))))
    print(f"k_grad_area factor {factor}: {n} outputs, {n - AREA_ONE_PASS} in the second pass; {differ.size} differ from gradients_ref.area, "
          f"{int((differ >= AREA_ONE_PASS).sum())} of them in the second pass")
    assert differ.size == 0, f"first {differ[:8].tolist()}"
    np.testing.assert_array_equal(out, want)
