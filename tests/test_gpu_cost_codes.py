"""GPU: inversion cost and sigma0 residual rasters from stored grid codes (xsw_cost_from_codes / xsw_cost_cr_from_codes, kernels
k_cost_co / k_cost_cr; `CopolCodes.cost`, `.cost_dual`).

The yardstick everywhere is the numpy restatement tests/cost_codes_ref.py (pinned to the minimum of the oracle's dense cost
arrays by tests/test_cost_codes_cpu.py): the codes come from ONE fused dual-pol xsw_invert launch on device rasters, and fed
those codes the new entries must give the restatement's four rasters bit for bit, NaN positions included (float32 outputs: the
restatement rounded once).

sigma0 in dB as the kernels form it (xsw_device.hpp: to_db), which the restatement is handed: a float32 raster in float32
arithmetic with log10 correctly rounded to float32 (a float64 log10 rounded once; not numpy's float32 log10: 10766 of 20504
pixels of the 70 x 333 scene differ in Jsig with that one, none with this one); a float64 raster by 10 * log10(x + 1e-15) with the
DEVICE math library's float64 log10, which is within an ulp of the host's but not the same function (with numpy's log10, 55 of
those 20504 pixels differ in the last bit of the residual) -- so for linear float64 rasters the dB value is taken from the
device through torch, the package's own DB_TORCH route (`_device.to_db`), not from the kernels under test."""
import warnings

import numpy as np
import pytest

import cost_codes_ref as cref
from test_gpu_crosspol_codes import _fused, _scene
from test_gpu_streams import ASYNC, _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from util import lut_dicts, small_luts

from conftest import golden
from oracle import invert as oinv

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output raster
SENTINEL = {np.float32: np.float32(-7.5e37), np.float64: np.float64(-7.5e300)}  # no cost (>= 0 or NaN) and no residual in dB


def _db(x, is_db, torch=None):
    """The dB value the kernels compute from raster `x` (module docstring), as float64."""
    if is_db:
        return x.astype(np.float64)
    with np.errstate(all="ignore"):
        if x.dtype == np.float64:
            from xsarsea_amd import _device
            return _device.to_db(torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))).cpu().numpy()
        y = x + np.float32(1e-15)
        return (np.float32(10.0) * np.log10(y.astype(np.float64)).astype(np.float32)).astype(np.float64)


def _fill(x, scalar):
    """windspeed.py:122-123 in the raster's dtype: what a NULL dsig_cr raster stands for."""
    with np.errstate(all="ignore"):
        return x * x.dtype.type(0) + x.dtype.type(scalar)


def _cost(ctx, torch, _lib, kind, arrs, out_t, is_db=False, want=(1, 1, 1, 1), mem=None, dsig_co=0.1):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays).  kind "co": arrs = (inc, code_co, sigma0_co, anc);
    "cr": (inc, code_co or None, code_cr, sigma0_cr, dsig_cr or None).  Every requested output lies between two guard regions
    and starts as the sentinel: returns [J, Jsig, Jwind, residual] host arrays (None where not requested) after checking that
    the guards are untouched and every pixel was written."""
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    item, sent = np.dtype(out_t).itemsize, SENTINEL[out_t]
    hosts = [None if a is None else np.ascontiguousarray(a) for a in arrs]
    host_route = mem == _lib.MEM_HOST
    if host_route:
        bufs = [np.full(n + 2 * GUARD, sent, out_t) if w else None for w in want]
        ins = [None if a is None else a.ctypes.data for a in hosts]
        outs = [None if b is None else b.ctypes.data + GUARD * item for b in bufs]
    else:
        dev = torch.device("cuda", 0)
        keep = [None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in hosts]
        bufs = [torch.full((n + 2 * GUARD,), float(sent), dtype=torch.float32 if out_t == np.float32 else torch.float64, device=dev) if w else None
                for w in want]
        torch.cuda.synchronize()
        ins = [None if t is None else t.data_ptr() for t in keep]
        outs = [None if b is None else b.data_ptr() + GUARD * item for b in bufs]
    if kind == "co":
        ctx.cost_from_codes_raw(shape[0], shape[1], dt, od, _lib.MEM_HOST if host_route else _lib.MEM_DEVICE, *ins, *outs, dsig_co=dsig_co,
                                sigma0_is_db=is_db)
    else:
        ctx.cost_cr_from_codes_raw(shape[0], shape[1], dt, od, _lib.MEM_HOST if host_route else _lib.MEM_DEVICE, *ins, *outs, dsig_cr_scalar=0.1,
                                   sigma0_is_db=is_db)
    ctx.synchronize()
    res = []
    for b in bufs:
        if b is None:
            res.append(None)
            continue
        h = b if host_route else b.cpu().numpy()
        assert np.all(h[:GUARD] == sent) and np.all(h[-GUARD:] == sent), "a guard region was written"
        assert not np.any(h[GUARD:-GUARD] == sent), "a pixel was not written"
        res.append(h[GUARD:-GUARD].reshape(shape).copy())
    return res


def _differ(a, b):
    return int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def _assert_fields(got, want, out_t, what):
    """Every requested field == the restatement's (rounded once to a float32 output), NaN positions included."""
    counts = {}
    for k, g in zip(cref.FIELDS, got):
        if g is not None:
            with np.errstate(all="ignore"):
                counts[k] = _differ(g, want[k].astype(out_t))
    print(f"{what}: pixels that differ from the restatement {counts}")
    assert not any(counts.values()), f"{what}: {counts}"


def _same(a, b):
    return all((x is None and y is None) or _differ(x, y) == 0 for x, y in zip(a, b))


@pytest.fixture(scope="module")
def default_tab(default_luts):
    return cref.tables(*default_luts)


@pytest.fixture
def default_ctx(gpu_ctx, default_luts):
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    return gpu_ctx


@pytest.mark.parametrize("is_db", [0, 1])
@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_equal_to_the_restatement(default_ctx, torch, default_tab, dtype, out_t, is_db):
    """70 x 333 (ragged last wave) on the default LUTs, every input class: the co-pol cost; the cross-pol cost with dsig_cr as a
    raster and as a scalar; code_co = NULL against the codes of the fused cross-pol-only call."""
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), dtype)
    if is_db:
        s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    s_co_db, s_cr_db = _db(s_vv, is_db, torch), _db(s_vh, is_db, torch)
    for name, d in (("raster", dsig), ("scalar", None)):
        f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, d, anc), np.complex128, False, is_db)
        cc, ccr = f["cc"], f["ccr"]
        assert np.any(cc == _lib.CODE_NAN_RE) and np.any(cc == _lib.CODE_NAN) and np.any(ccr == _lib.CODE_NO_INDEX) and np.any(ccr == _lib.CODE_NAN_RE)
        assert np.any(np.isnan(inc) & (cc == _lib.CODE_NAN_RE)) and np.any(~np.isnan(inc) & (cc == _lib.CODE_NAN_RE))
        assert np.any((cc == _lib.CODE_NAN) & (ccr < _lib.CODE_NO_INDEX)), "no cross-pol-only pixel"
        if d is not None:
            got = _cost(default_ctx, torch, _lib, "co", (inc, cc, s_vv, anc), out_t, is_db)
            _assert_fields(got, cref.cost_co(cc, inc, s_co_db, anc, 0.1, default_tab), out_t, "co-pol")
            assert np.all(np.isnan(got[0]) == (cc >= 0x80000000)), "J is NaN exactly where the code is no grid code"
        got = _cost(default_ctx, torch, _lib, "cr", (inc, cc, ccr, s_vh, d), out_t, is_db)
        _assert_fields(got, cref.cost_cr(cc, ccr, inc, s_cr_db, dsig if d is not None else _fill(s_vh, 0.1), default_tab), out_t, f"cross-pol, dsig {name}")
    ccr = _fused(default_ctx, torch, _lib, (inc, None, s_vh, dsig, None), np.complex128, False, is_db)["ccr"]
    got = _cost(default_ctx, torch, _lib, "cr", (inc, None, ccr, s_vh, dsig), out_t, is_db)
    _assert_fields(got, cref.cost_cr(None, ccr, inc, s_cr_db, dsig, default_tab), out_t, "cross-pol, code_co = NULL")
    assert np.isnan(got[2]).all() and _differ(got[0], got[1]) == 0


@pytest.mark.parametrize("tag", ["phi360_f64", "phi90_f64"])
def test_table_shapes(gpu_ctx, torch, tag):
    """A 0..360 and a 0..90 co-pol LUT (small goldens) besides the default 0..180 one; phi90: Im(anc) keeps its sign."""
    from xsarsea_amd import _lib
    d = golden(f"kernel_small_{tag}.npz")
    lco, lcr = small_luts(d)
    tab = cref.tables(lco, lcr)
    assert tab.phi_180 == (tag != "phi90_f64")
    co, cr = lut_dicts(lco, lcr)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = (np.ascontiguousarray(d[k]) for k in ("inc", "sigma0_vv", "sigma0_vh", "dsig_cr", "anc"))
    s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    f = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, True, is_db=True)
    searched = f["cc"] < 0x80000000
    assert np.any(searched & (anc.imag < 0)) and np.any(searched & (anc.imag > 0))
    _assert_fields(_cost(gpu_ctx, torch, _lib, "co", (inc, f["cc"], s_vv, anc), np.float64, True), cref.cost_co(f["cc"], inc, s_vv, anc, 0.1, tab),
                   np.float64, f"{tag} co-pol")
    _assert_fields(_cost(gpu_ctx, torch, _lib, "cr", (inc, f["cc"], f["ccr"], s_vh, dsig), np.float64, True),
                   cref.cost_cr(f["cc"], f["ccr"], inc, s_vh, dsig, tab), np.float64, f"{tag} cross-pol")


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 64), (1, 65), (3, 257)])
def test_small_shapes(default_ctx, torch, default_tab, shape):
    """One lane, one lane short of a wave, a whole wave, one lane past it, one lane past a 256-pixel block."""
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene(shape, np.float64, 5)
    inc[0, 0], s_vv[0, 0], s_vh[0, 0], dsig[0, 0], anc[0, 0] = 33.0, 0.02, 2e-3, 0.1, 7 + 2j
    inc[-1, -1], s_vv[-1, -1], s_vh[-1, -1], dsig[-1, -1], anc[-1, -1] = 40.0, 0.03, 1e-3, 0.5, 5 - 1j  # a searched pixel in the last lane
    s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, False, is_db=True)
    assert f["cc"][-1, -1] < 0x80000000 and f["ccr"][-1, -1] < _lib.CODE_NO_INDEX
    _assert_fields(_cost(default_ctx, torch, _lib, "co", (inc, f["cc"], s_vv, anc), np.float64, True),
                   cref.cost_co(f["cc"], inc, s_vv, anc, 0.1, default_tab), np.float64, f"{shape} co-pol")
    _assert_fields(_cost(default_ctx, torch, _lib, "cr", (inc, f["cc"], f["ccr"], s_vh, dsig), np.float64, True),
                   cref.cost_cr(f["cc"], f["ccr"], inc, s_vh, dsig, default_tab), np.float64, f"{shape} cross-pol")


def test_nullable_outputs(default_ctx, torch, default_tab):
    """Each output alone (J alone is `parts=False`), and each one left out: what is written equals the all-four run bit for bit,
    and (inside _cost) nothing is written outside the requested rasters."""
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene((9, 333), np.float32, 7)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex64, False)
    for kind, arrs in (("co", (inc, f["cc"], s_vv, anc)), ("cr", (inc, f["cc"], f["ccr"], s_vh, dsig))):
        full = _cost(default_ctx, torch, _lib, kind, arrs, np.float64)
        assert not np.isnan(full[0]).all()
        for k in range(4):
            alone = tuple(int(j == k) for j in range(4))
            got = _cost(default_ctx, torch, _lib, kind, arrs, np.float64, want=alone)
            assert [g is not None for g in got] == [bool(w) for w in alone] and _differ(got[k], full[k]) == 0, f"{kind}: output {k} alone"
            without = tuple(int(j != k) for j in range(4))
            got = _cost(default_ctx, torch, _lib, kind, arrs, np.float64, want=without)
            assert got[k] is None and _same([g for j, g in enumerate(got) if j != k], [g for j, g in enumerate(full) if j != k]), f"{kind}: without output {k}"


def test_foreign_codes(gpu_ctx, torch, default_luts, lowres_luts):
    """Codes of the default co-pol LUT, and random words with bit 31 set, handed to a context that holds the low-resolution LUTs:
    the calls return, every pixel whose code is no code of that LUT is NaN in all outputs, the others equal the restatement on
    the low-resolution tables (test_gpu_crosspol_codes.test_foreign_codes' inputs)."""
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), np.float64, 31)
    codes = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, False)["cc"]
    rnd = np.random.default_rng(3)
    codes[rnd.random(codes.shape) < 0.05] = 0x80000000
    wild = codes == 0x80000000
    codes[wild] |= rnd.integers(0, 1 << 31, int(wild.sum()), dtype=np.uint32)
    lco, lcr = lowres_luts
    co, cr = lut_dicts(lco, lcr)
    gpu_ctx.upload_luts(co=co, cr=cr)
    tab = cref.tables(lco, lcr)
    plane = len(lco.wspd) * len(lco.phi)
    real = codes < 0x80000000
    out_of_range = real & ((codes & 0x3FFFFFFF) >= plane)
    assert out_of_range.sum() > 100 and (real & ~out_of_range).sum() > 100 and wild.sum() > 100
    s_co_db, s_cr_db = oinv.to_db(s_vv), oinv.to_db(s_vh)
    got = _cost(gpu_ctx, torch, _lib, "co", (inc, codes, s_co_db, anc), np.float64, True)
    assert all(np.isnan(g[out_of_range | wild]).all() for g in got)
    _assert_fields(got, cref.cost_co(codes, inc, s_co_db, anc, 0.1, tab), np.float64, "foreign co-pol codes")
    # the cross-pol cost next to foreign co-pol codes (no co-pol wind there), and foreign cross-pol codes
    ccr = _fused(gpu_ctx, torch, _lib, (inc, None, s_cr_db, dsig, None), np.complex128, False, is_db=True)["ccr"]
    ccr[wild] = codes[wild] & np.uint32(0x7FFFFFFF)  # random indices, most of them beyond the table
    ccr[5, 5:9] = [len(lcr.wspd), 0x3FFFFFFE, 0x7FFFFFFE, len(lcr.wspd) - 1]
    got = _cost(gpu_ctx, torch, _lib, "cr", (inc, codes, ccr, s_cr_db, dsig), np.float64, True)
    _assert_fields(got, cref.cost_cr(codes, ccr, inc, s_cr_db, dsig, tab), np.float64, "foreign codes, cross-pol")
    beyond = (ccr != _lib.CODE_NAN_RE) & ((ccr & 0x3FFFFFFF) >= len(lcr.wspd))
    assert beyond.sum() > 100 and all(np.isnan(g[beyond]).all() for g in got)
    assert np.isnan(got[2][out_of_range | wild]).all()


def test_host_route_equals_device_route(default_ctx, torch):
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), np.float32, 23)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex64, True)
    for kind, arrs in (("co", (inc, f["cc"], s_vv, anc)), ("cr", (inc, f["cc"], f["ccr"], s_vh, dsig)), ("cr", (inc, None, f["ccr"], s_vh, None))):
        for out_t, want in ((np.float32, (1, 1, 1, 1)), (np.float64, (1, 0, 0, 1))):
            a = _cost(default_ctx, torch, _lib, kind, arrs, out_t, want=want)
            b = _cost(default_ctx, torch, _lib, kind, arrs, out_t, want=want, mem=_lib.MEM_HOST)
            assert not np.isnan(a[0]).all() and _same(a, b), f"{kind}, {np.dtype(out_t).name}"


def test_error_codes(torch, default_luts):
    """XSW_EINVAL (-1) with a message, before any launch: the outputs keep their fill."""
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a, z = np.full((2, 8), 33.0, np.float32), np.full((2, 8), 5 + 1j, np.complex64)
        c = np.zeros((2, 8), np.uint32)
        o = np.full((2, 8), 77.0, np.float32)
        p = lambda x: None if x is None else x.ctypes.data
        msg = lambda: ctx._lib.xsw_last_error(ctx._h).decode()
        co = lambda outs=(o, None, None, None), dsig_co=0.1, shape=(2, 8): ctx._lib.xsw_cost_from_codes(
            ctx._h, *shape, 0, 0, 0, 0, p(a), p(c), p(a), p(z), dsig_co, *(p(x) for x in outs))
        cr = lambda outs=(o, None, None, None), code_co=None, shape=(2, 8): ctx._lib.xsw_cost_cr_from_codes(
            ctx._h, *shape, 0, 0, 0, 0, p(a), p(code_co), p(c), p(a), None, 0.1, *(p(x) for x in outs))
        assert co() == -1 and "no co-pol LUT" in msg()
        assert cr() == -1 and "no cross-pol LUT" in msg()
        lut_co, lut_cr = lut_dicts(*default_luts)
        ctx.upload_luts(cr=lut_cr)
        assert cr(code_co=c) == -1 and "co-pol" in msg()  # co-pol codes without their LUT
        assert cr() == 0
        ctx.upload_luts(co=lut_co)
        assert co((None,) * 4) == -1 and "no output" in msg()
        assert cr((None,) * 4) == -1 and "no output" in msg()
        assert co(dsig_co=0.0) == -1 and "dsig_co" in msg()
        assert co(dsig_co=float("nan")) == -1 and "dsig_co" in msg()
        assert co(shape=(1 << 31, 1 << 31)) == -1 and "too large" in msg()
        assert cr(shape=(1 << 31, 1 << 31)) == -1 and "too large" in msg()
        o[...] = 77.0
        assert co(shape=(-1, 8)) == -1
        ctx.synchronize()
        assert np.all(o == 77.0), "a refused call wrote its output"
        assert co() == 0 and cr(code_co=c) == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public calls
def _dense_jco_min(lut_co, dsig_co, inc, s_db, anc):
    """J_co.min() of oracle/invert.py:75-96 per pixel (NaN where the co-pol search does not run)."""
    p = oinv.Prepared(lut_co, None, dsig_co)
    out = np.full(inc.shape, np.nan)
    with np.errstate(all="ignore"):
        for i in np.ndindex(inc.shape):
            if np.isnan(inc[i]) or np.isnan(s_db[i]) or np.isnan(np.abs(anc[i])):
                continue
            lut_inc = p.co_lut[:, :, np.argmin(np.abs(p.inc_dim - inc[i]))]
            m_antenna, m_azi = np.real(anc[i]), np.imag(anc[i])
            if p.phi_180:
                m_azi = np.abs(m_azi)
            Jwind_co = ((p.lut_co_antenna - m_antenna) / p.d_antenna) ** 2 + ((p.lut_co_azi - m_azi) / p.d_azi) ** 2
            Jsig_co = ((lut_inc - s_db[i]) / p.dsig_co) ** 2
            out[i] = (Jwind_co + Jsig_co).min()
    return out


@pytest.mark.parametrize("container", ["numpy", "torch"])
def test_public_api(gpu_ctx, torch, container):
    """cc.cost == the restatement; cc.cost(...).J == the oracle's dense J_co.min() on a 16 x 64 crop; cost_dual on codes with and
    without the select agree and equal the restatement; parts=False; out_dtype; dsig_co from invert_copol_codes."""
    from xsarsea_amd import windspeed
    from xsarsea_amd.windspeed import _engine, get_model
    sc = _scene((70, 333), np.float32, 41)
    h_inc, h_vv, h_vh, h_dsig, h_anc = sc
    if container == "torch":
        dev = torch.device("cuda", 0)
        sc = tuple(torch.from_numpy(a).to(dev) for a in sc)
    inc, s_vv, s_vh, dsig, anc = sc
    host = lambda x: x.cpu().numpy() if container == "torch" else x
    # numpy rasters: float32 sigma0 goes to dB by numpy's own log10 on the host; device rasters: by the kernel
    to_db = (lambda x: _db(x, False)) if container == "torch" else (lambda x: oinv.to_db(x).astype(np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, dsig_co=0.2, model="gmf_cmod5n", resolution="low")
        lut_co, lut_cr = cc.lut_co, _engine.lut_source(get_model("gmf_s1_v2"), dict(resolution="low"))
        tab = cref.tables(lut_co, lut_cr)
        codes = host(cc.codes).view(np.uint32)
        cost = cc.cost(s_vv, anc)
        assert isinstance(cost, windspeed.InversionCost) and cost["J"] is cost.J
        got = [host(cost[k]) for k in ("J", "Jsig", "Jwind", "residual_db")]
        assert all(g.dtype == np.float64 and g.shape == (70, 333) for g in got)
        _assert_fields(got, cref.cost_co(codes, h_inc, to_db(h_vv), h_anc, 0.2, tab), np.float64, f"{container} cost")
        crop = (slice(0, 16), slice(0, 64))
        dense = _dense_jco_min(lut_co, 0.2, h_inc[crop].astype(np.float64), to_db(h_vv)[crop], h_anc[crop].astype(np.complex128))
        assert np.isfinite(dense).sum() > 500 and _differ(got[0][crop], dense) == 0, "J is not the minimum of the dense J_co"
        only_j = cc.cost(s_vv, anc, parts=False, out_dtype=np.float32)
        assert only_j.Jsig is None and only_j.Jwind is None and only_j.residual_db is None
        assert host(only_j.J).dtype == np.float32 and _differ(host(only_j.J), got[0].astype(np.float32)) == 0
        other = cc.cost(s_vv, anc, dsig_co=0.1, parts=False)
        assert _differ(host(other.J), cref.cost_co(codes, h_inc, to_db(h_vv), h_anc, 0.1, tab)["J"]) == 0
        for d in (dsig, 0.1):
            kw = dict(dsig_cr=d, model="gmf_s1_v2", resolution="low")
            sel, raw = cc.dual(s_vh, codes=True, dual_select=True, **kw), cc.dual(s_vh, codes=True, dual_select=False, **kw)
            assert np.any(host(sel).view(np.uint32) != host(raw).view(np.uint32))
            a, b = cc.cost_dual(s_vh, sel, **kw), cc.cost_dual(s_vh, raw, **kw)
            ga, gb = ([host(c[k]) for k in ("J", "Jsig", "Jwind", "residual_db")] for c in (a, b))
            assert _same(ga, gb), "cost_dual depends on the select"
            want = cref.cost_cr(codes, host(raw).view(np.uint32), h_inc, to_db(h_vh), h_dsig if d is dsig else _fill(h_vh, 0.1), tab)
            _assert_fields(ga, want, np.float64, f"{container} cost_dual, dsig_cr {'raster' if d is dsig else d}")
        j = cc.cost_dual(s_vh, raw, parts=False, **kw)
        assert j.Jsig is None and _differ(host(j.J), ga[0]) == 0


def test_user_stream_without_an_intermediate_sync(gpu_ctx, torch, delay_cycles):
    """invert_copol_codes, .dual(codes=True), .cost and .cost_dual back to back on a user stream whose producer is held back: all
    return while it is in flight, the result is consumed on that stream and equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _scene((48, 260), np.float32, 51), _scene((48, 260), np.float32, 52)
    kw = dict(model="gmf_cmod5n", resolution="low", **ASYNC)
    cr = dict(model="gmf_s1_v2", resolution="low")

    def call(b):
        cc = windspeed.invert_copol_codes(b[0], b[1], ancillary_wind=b[4], **kw)
        ccr = cc.dual(b[2], dsig_cr=b[3], codes=True, **cr)
        co, du = cc.cost(b[1], b[4]), cc.cost_dual(b[2], ccr, dsig_cr=b[3], **cr)
        return co.J, co.residual_db, du.J, du.Jwind

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = _staged(torch, list(sc), list(dec))
        ref = call([src for _, src in pairs])  # landed rasters, synchronised: LUTs installed, work lists sized
        torch.cuda.synchronize()
        ref = [r.cpu().numpy() for r in ref]
        wrong = [r.cpu().numpy() for r in call([buf for buf, _ in pairs])]  # the decoy scene: what a read that overtakes the producer gives
        assert _differ(wrong[0], ref[0]) > 1000
        P = torch.cuda.Stream(device=torch.device("cuda", 0))
        with torch.cuda.stream(P):
            done = _held_back(torch, P, delay_cycles, pairs)
            res = call([buf for buf, _ in pairs])
            _in_flight(done)
            got = _read_back(torch, P, *res)
    assert not np.isnan(ref[0]).all() and _same(got, ref)
