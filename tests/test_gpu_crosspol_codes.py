"""GPU: the cross-pol step from stored co-pol codes (xsw_cross_from_codes / k_cross_from_codes; `invert_copol_codes`,
`CopolCodes`).

The yardstick everywhere is the existing FUSED kernel: one dual-pol xsw_invert launch on device rasters that writes
out_code_co, out_code_cr and out_cr.  Fed that launch's out_code_co, the new entry must reproduce out_code_cr and out_cr bit for
bit, NaN kinds included."""
import warnings

import numpy as np
import pytest

import crosspol_codes_ref as ref
from test_gpu_codes import _bits, _device_run
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import ASYNC, _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from util import bits_equal, lut_dicts

from oracle import invert as oinv
from oracle import lut as olut

pytestmark = pytest.mark.gpu


def _fused(ctx, torch, _lib, arrs, out_c, dual_select, is_db=False):
    """The yardstick: {cc, ccr (uint32), cr (complex)} of one fused launch (cross-pol only when arrs[1] is None)."""
    o = _device_run(ctx, torch, _lib, arrs, out_c, {"complex", "codes"}, dual_select=dual_select, is_db=is_db)
    h = {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}
    return dict(cc=None if h["cc"] is None else h["cc"].view(np.uint32), ccr=h["ccr"].view(np.uint32), cr=h["cr"])


def _cross(ctx, torch, _lib, inc, code_co, s_cr, dsig, out_c, dual_select, is_db=False, mem=None):
    """xsw_cross_from_codes on device rasters (or, mem = MEM_HOST, on the host arrays): (code_cr uint32, out_cr)."""
    f32 = inc.dtype == np.float32
    dt, od = (_lib.XSW_F32 if f32 else _lib.XSW_F64), (_lib.XSW_F32 if out_c == np.complex64 else _lib.XSW_F64)
    hosts = [np.ascontiguousarray(a) if a is not None else None for a in (inc, code_co, s_cr, dsig)]
    if mem == _lib.MEM_HOST:
        code, out = np.full(inc.shape, 0x12345678, np.uint32), np.empty(inc.shape, out_c)
        hp = lambda a: None if a is None else a.ctypes.data
        ctx.cross_from_codes_raw(inc.shape[0], inc.shape[1], dt, od, _lib.MEM_HOST, hp(hosts[0]), hp(hosts[1]), hp(hosts[2]), hp(hosts[3]),
                                 code.ctypes.data, out.ctypes.data, dsig_cr_scalar=0.1, sigma0_is_db=is_db, dual_select=dual_select)
        return code, out
    dev = torch.device("cuda", 0)
    t = [None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in hosts]
    code = torch.full(inc.shape, 0x12345678, dtype=torch.int32, device=dev)
    out = torch.empty(inc.shape, dtype=torch.complex64 if out_c == np.complex64 else torch.complex128, device=dev)
    torch.cuda.synchronize()
    p = lambda x: None if x is None else x.data_ptr()
    ctx.cross_from_codes_raw(inc.shape[0], inc.shape[1], dt, od, _lib.MEM_DEVICE, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(code), p(out),
                             dsig_cr_scalar=0.1, sigma0_is_db=is_db, dual_select=dual_select)
    ctx.synchronize()
    return code.cpu().numpy().view(np.uint32), out.cpu().numpy()


def _assert_same(got, want, what):
    assert not np.any(got[0] == 0x12345678), f"{what}: a cross-pol code was not written"
    bad = np.flatnonzero(got[0].ravel() != want["ccr"].ravel())
    assert bad.size == 0, f"{what}: {bad.size} cross-pol codes differ from the fused launch, first at {bad[:5]}"
    assert np.array_equal(_bits(got[1]), _bits(want["cr"])), f"{what}: out_cr differs from the fused launch"


def _scene(shape, dtype, seed=11):
    """synthetic_scene with every input class in it (early NaNs, no co-pol search, no cross-pol search by either input)."""
    inc, s_vv, s_vh, dsig, anc = synthetic_scene(max(shape[0], 8), max(shape[1] + 8, 80), dtype, seed)  # columns 0..2 are NaN incidence
    inc, s_vv, s_vh, dsig, anc = (np.ascontiguousarray(a[:shape[0], 8:8 + shape[1]]) for a in (inc, s_vv, s_vh, dsig, anc))
    r = np.random.default_rng(seed)
    for a in (inc, anc, s_vv, s_vh, dsig):
        a[r.random(shape) < 0.04] = np.nan
    return inc, s_vv, s_vh, dsig, anc


@pytest.mark.parametrize("is_db", [0, 1])
@pytest.mark.parametrize("dual_select", [False, True])
@pytest.mark.parametrize("out_c", [np.complex64, np.complex128])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_equal_to_the_fused_launch(gpu_ctx, torch, default_luts, dtype, out_c, dual_select, is_db):
    """70 x 333 (ragged last wave) on the default LUTs: dsig_cr as a raster and as a scalar, and code_co = NULL against the fused
    cross-pol-only call."""
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), dtype)
    if is_db:
        s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    for name, d in (("raster", dsig), ("scalar", None)):
        want = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, d, anc), out_c, dual_select, is_db)
        assert np.any(want["cc"] == _lib.CODE_NAN_RE) and np.any(want["cc"] == _lib.CODE_NAN) and np.any(want["ccr"] == _lib.CODE_NO_INDEX)
        got = _cross(gpu_ctx, torch, _lib, inc, want["cc"], s_vh, d, out_c, dual_select, is_db)
        _assert_same(got, want, f"dsig {name}")
    want = _fused(gpu_ctx, torch, _lib, (inc, None, s_vh, dsig, None), out_c, dual_select, is_db)
    _assert_same(_cross(gpu_ctx, torch, _lib, inc, None, s_vh, dsig, out_c, dual_select, is_db), want, "code_co = NULL")


@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (3, 64)])
def test_small_shapes(gpu_ctx, torch, default_luts, shape):
    """One lane, one lane past a wave, whole waves: lane masking and the cooperative fallback (NaN dsig next to inf sigma0)."""
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = _scene(shape, np.float64, 5)
    if shape != (1, 1):
        inc[0, :4], s_vv[0, :4], s_vh[0, :4], dsig[0, :4], anc[0, :4] = 33.0, 0.02, [np.inf, 1e-3, 0.0, 1e-3], [0.1, np.inf, 0.1, 0.0], 7 + 2j
        inc[-1, -1], s_vv[-1, -1], s_vh[-1, -1], dsig[-1, -1], anc[-1, -1] = 40.0, 0.02, np.inf, 0.5, 5 - 1j  # undecided in the last lane
    else:
        inc[0, 0], s_vv[0, 0], s_vh[0, 0], dsig[0, 0], anc[0, 0] = 33.0, 0.02, 2e-3, 0.1, 7 + 2j
    for sel in (False, True):
        want = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, sel)
        _assert_same(_cross(gpu_ctx, torch, _lib, inc, want["cc"], s_vh, dsig, np.complex128, sel), want, f"{shape} select={sel}")


def _route_lut(route, lcr):
    """The cross-pol dB LUT that sends the search down `route` (xsw_device.hpp: invert_strip's conditions).  The built ones sit on
    binary-fraction axes with values quantised to binary fractions, so that plateaus give exact ties."""
    if route == "scan":        # monotone, inverse table: search_cr_scan
        return lcr
    rng = np.random.default_rng(8)
    inc_ax = np.array([24.0, 32.0, 40.0, 48.0])
    n_w = 65536 if route == "interval" else 256   # 65536 rows: no inverse table (xsw_lutplan.hpp: CrPlan) -> search_cr_interval
    w = np.arange(n_w) * (2.0 ** -10 if route == "interval" else 0.25)
    q = 2.0 ** -6 if route == "interval" else 2.0 ** -2
    vals = -36.0 + np.floor(16.0 * np.log2(1.0 + w) / 6.0 / q) * q + np.arange(4)[:, None] * 0.5
    if route == "noisy":       # not monotone: search_cr_lanes, near-ties to the cooperative scan
        vals = vals + np.round(rng.normal(0, 1.0, vals.shape) / q) * q
    if route == "nan":         # one NaN entry: not finite, every pixel goes to the cooperative scan
        vals[1, 100] = np.nan
    return olut.Lut(vals, inc_ax, w, None, "dB", "x", "cr", "VH")


def _count_ties(lcr, inc, s_db, dsig, picks):
    tab, n = ref.tables(None, lcr), 0
    for i in picks:
        row = tab["cr_lut"][:, np.argmin(np.abs(tab["inc_cr_dim"] - inc.ravel()[i]))]
        J = ((row - s_db.ravel()[i]) / dsig.ravel()[i]) ** 2.0
        n += int(np.sum(J == np.nanmin(J)) > 1)
    return n


@pytest.mark.parametrize("route", ["scan", "interval", "noisy", "nan"])
def test_every_search_route(gpu_ctx, torch, default_luts, route):
    """Each cross-pol search route, chosen by the LUT, with exact ties in it: pixels without a co-pol wind whose sigma0 (in dB) is
    a table value of a plateau, or exactly midway between two neighbouring table values -- the first index wins, as in the fused
    launch (numpy's argmin)."""
    from xsarsea_amd import _lib
    lco, lcr0 = default_luts
    lcr = _route_lut(route, lcr0)
    co, cr = lut_dicts(lco, lcr)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), np.float64, 21)
    s_vv, s_db = oinv.to_db(s_vv), oinv.to_db(s_vh)
    if route != "scan":
        s_db = np.clip(s_db + 4.0, -36.0, -8.0)
    # exact ties: rows 60.. hold cross-only pixels on an incidence of the LUT's axis, dsig a power of two
    rng = np.random.default_rng(2)
    tie = np.zeros(inc.shape, bool)
    tie[60:, 8:] = True
    vals, inc_ax = np.asarray(lcr.values), np.asarray(lcr.incidence)
    r_i = rng.integers(0, len(inc_ax), inc.shape)
    k = rng.integers(1, vals.shape[1] - 2, inc.shape)
    v0, v1 = vals[r_i, k], vals[r_i, k + 1]
    mid = np.where(v1 > v0, (v0 + v1) / 2, v0)
    mid = np.where(np.isnan(mid), -20.0, mid)
    inc[tie], s_vv[tie], s_db[tie], dsig[tie] = inc_ax[r_i][tie], np.nan, mid[tie], 0.125
    picks = np.flatnonzero(tie.ravel())[::23]
    assert _count_ties(lcr, inc, s_db, dsig, picks) >= 5, "the tie pixels are not tied"
    for sel in (False, True):
        want = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_db, dsig, anc), np.complex128, sel, is_db=True)
        _assert_same(_cross(gpu_ctx, torch, _lib, inc, want["cc"], s_db, dsig, np.complex128, sel, is_db=True), want, f"{route} select={sel}")
    want = _fused(gpu_ctx, torch, _lib, (inc, None, s_db, dsig, None), np.complex128, False, is_db=True)
    _assert_same(_cross(gpu_ctx, torch, _lib, inc, None, s_db, dsig, np.complex128, False, is_db=True), want, f"{route} cross-only")


def test_select_near_five_metres_per_second(gpu_ctx, torch, default_luts):
    """The near-5 m/s select cases of test_sign_choice_and_dual_select_near_ties through the new entry."""
    from oracle import gmf
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    phis = [0.0, 0.3, 1.0, 37.0, 90.0, 179.0, 179.7, 180.0]
    ims = [0.0, -0.0, 1e-300, -1e-300, 1e-17, -1e-17, 1e-10, -1e-10, 1e-8, -1e-8, 1e-3, -1e-3, None, "neg"]
    rows = []
    for w in (2.0, 4.9, 8.0):
        for ph in phis:
            for im in ims:
                for wd in (4.9, 5.0, 5.1, 12.0):
                    a_im = w * np.sin(np.radians(ph)) * (1 if im is None else -1) if im in (None, "neg") else im
                    rows.append((35.0, w, ph, w * np.cos(np.radians(ph)), a_im, wd))
    r = np.array(rows)
    inc = r[:, 0].reshape(1, -1).copy()
    s_vv = oinv.to_db(gmf.gmf_cmod5n(inc, r[:, 1].reshape(1, -1), r[:, 2].reshape(1, -1)))
    s_vh = oinv.to_db(gmf.GMFS["gmf_s1_v2"][0](inc, r[:, 5].reshape(1, -1)))
    anc = (r[:, 3] + 1j * r[:, 4]).reshape(1, -1)
    dsig = np.full(inc.shape, 0.01)
    for sel in (False, True):
        want = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, sel, is_db=True)
        if sel:
            pc = (want["ccr"] & _lib.CODE_PICK_CO) != 0
            assert pc.sum() > 50 and (~pc).sum() > 50
        _assert_same(_cross(gpu_ctx, torch, _lib, inc, want["cc"], s_vh, dsig, np.complex128, sel, is_db=True), want, f"select={sel}")


def test_foreign_codes(gpu_ctx, torch, default_luts, lowres_luts):
    """Codes taken with the default co-pol LUT handed to a context that holds the low-resolution one (normally sized buffers:
    the kernel's own bounds check): the call returns, every pixel whose index is out of range there is XSW_CODE_NAN_RE, every
    other one equals the restatement run on the low-resolution tables."""
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), np.float64, 31)
    codes = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, False)["cc"]
    lco, lcr = lowres_luts
    co, cr = lut_dicts(lco, lcr)
    gpu_ctx.upload_luts(co=co, cr=cr)
    plane = len(lco.wspd) * len(lco.phi)
    real = codes < _lib.CODE_NAN
    out_of_range = real & ((codes & 0x3FFFFFFF) >= plane)
    assert out_of_range.sum() > 100 and (real & ~out_of_range).sum() > 100
    s_db = oinv.to_db(s_vh)
    tab = ref.tables(lco, lcr)
    for sel in (False, True):
        got = _cross(gpu_ctx, torch, _lib, inc, codes, s_db, dsig, np.complex128, sel, is_db=True)
        want = ref.cross_from_codes(codes, inc, s_db, dsig, tab, dual_select=sel)
        assert np.all(got[0][out_of_range] == _lib.CODE_NAN_RE)
        assert np.array_equal(got[0], want[0]), f"select={sel}: codes differ from the restatement"
        assert bits_equal(got[1], want[1]), f"select={sel}: winds differ from the restatement"


def test_host_route_equals_device_route(gpu_ctx, torch, default_luts):
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    inc, s_vv, s_vh, dsig, anc = _scene((531, 700), np.float32, 23)
    want = _fused(gpu_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex64, True)
    for d in (dsig, None):
        a = _cross(gpu_ctx, torch, _lib, inc, want["cc"], s_vh, d, np.complex64, True)
        b = _cross(gpu_ctx, torch, _lib, inc, want["cc"], s_vh, d, np.complex64, True, mem=_lib.MEM_HOST)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        if d is not None:
            _assert_same(b, want, "host route")
    # only one of the two outputs asked for
    t = np.empty(inc.shape, np.complex64)
    gpu_ctx.cross_from_codes_raw(531, 700, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_HOST, inc.ctypes.data, want["cc"].ctypes.data, s_vh.ctypes.data,
                                 dsig.ctypes.data, None, t.ctypes.data, dual_select=True)
    assert np.array_equal(_bits(t), _bits(want["cr"]))
    # cross-pol only (code_co = NULL): the absent input stays absent on the host route
    inc, _, s_vh, dsig, _ = _scene((5, 67), np.float32, 29)
    a = _cross(gpu_ctx, torch, _lib, inc, None, s_vh, dsig, np.complex64, True)
    b = _cross(gpu_ctx, torch, _lib, inc, None, s_vh, dsig, np.complex64, True, mem=_lib.MEM_HOST)
    assert not np.any(b[0] == 0x12345678) and np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_error_codes(torch, default_luts):
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a = np.zeros((2, 8), np.float32)
        c = np.zeros((2, 8), np.uint32)
        call = lambda *args: ctx._lib.xsw_cross_from_codes(ctx._h, 2, 8, *args)
        p = lambda x: x.ctypes.data
        assert call(0, 0, 0, 0, 0, p(a), None, p(a), None, 0.1, p(c), None) == -3  # XSW_ENOLUT: no cross-pol LUT
        ctx.upload_luts(cr=lut_dicts(None, default_luts[1])[1])
        assert call(0, 0, 0, 0, 0, p(a), p(c), p(a), None, 0.1, p(c), None) == -3  # codes but no co-pol LUT
        assert call(0, 0, 0, 0, 0, p(a), None, p(a), None, 0.1, None, None) == -1  # XSW_EINVAL: no output
        assert call(0, 0, 0, 0, 0, None, None, p(a), None, 0.1, p(c), None) == -1
        assert call(0, 0, 0, 0, 0, p(a), None, None, None, 0.1, p(c), None) == -1
        assert call(7, 0, 0, 0, 0, p(a), None, p(a), None, 0.1, p(c), None) == -1
        assert call(0, 0, 0, 0, 0, p(a), None, p(a), None, 0.1, p(c), None) == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public calls
@pytest.mark.parametrize("container", ["numpy", "torch"])
def test_public_api(gpu_ctx, torch, container):
    """invert_copol_codes(...).wind() == invert_from_model mono; .dual(...) == the second output of the dual call; two cross-pol
    models in sequence on one CopolCodes each match their own fused call."""
    from xsarsea_amd import windspeed
    sc = _scene((70, 333), np.float32, 41)
    if container == "torch":
        dev = torch.device("cuda", 0)
        sc = tuple(torch.from_numpy(a).to(dev) for a in sc)
    inc, s_vv, s_vh, dsig, anc = sc
    host = lambda x: x.cpu().numpy() if container == "torch" else x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
        mono = windspeed.invert_from_model(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
        assert bits_equal(host(cc.wind()), host(mono)), "wind()"
        for cr_model, d in (("gmf_s1_v2", dsig), ("gmf_rs2_v2", 0.1), ("gmf_s1_v2", 0.2)):
            got = cc.dual(s_vh, dsig_cr=d, model=cr_model, resolution="low")
            want = windspeed.invert_from_model(inc, s_vv, s_vh, ancillary_wind=anc, dsig_cr=d, model=("gmf_cmod5n", cr_model), resolution="low")
            assert bits_equal(host(got), host(want[1])), f"dual, {cr_model}, dsig_cr {'raster' if d is dsig else d}"
            assert bits_equal(host(cc.wind()), host(want[0]))
    codes = host(cc.dual(s_vh, dsig_cr=dsig, model="gmf_s1_v2", resolution="low", codes=True))
    assert codes.shape == (70, 333) and codes.dtype == (np.int32 if container == "torch" else np.uint32)
    assert host(cc.codes).dtype == (np.int32 if container == "torch" else np.uint32)


class _Cai:
    """A device array that is no torch tensor: only `shape` and `__cuda_array_interface__`."""

    def __init__(self, t):
        self._keep, self.shape, self.__cuda_array_interface__ = t, tuple(t.shape), t.__cuda_array_interface__


def test_codes_as_a_plain_device_array(gpu_ctx, torch):
    """A CopolCodes built by hand from `__cuda_array_interface__` arrays (no torch tensors) gives the same winds."""
    from xsarsea_amd import windspeed
    dev = torch.device("cuda", 0)
    inc, s_vv, s_vh, dsig, anc = (torch.from_numpy(a).to(dev) for a in _scene((9, 130), np.float32, 43))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
        want = cc.wind().cpu().numpy(), cc.dual(s_vh, dsig_cr=dsig, model="gmf_s1_v2", resolution="low").cpu().numpy()
        torch.cuda.synchronize()
        by_hand = windspeed.CopolCodes(_Cai(inc), _Cai(cc.codes), cc.lut_co, ancillary_meta=((9, 130), np.dtype(np.complex64)))
        got = by_hand.wind().cpu().numpy(), by_hand.dual(_Cai(s_vh), dsig_cr=_Cai(dsig), model="gmf_s1_v2", resolution="low").cpu().numpy()
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])


def test_user_stream_without_an_intermediate_sync(gpu_ctx, torch, delay_cycles):
    """invert_copol_codes and .dual back to back on a user stream whose producer is held back: both return while it is in flight,
    and the result equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _scene((48, 260), np.float32, 51), _scene((48, 260), np.float32, 52)
    kw = dict(model="gmf_cmod5n", resolution="low", **ASYNC)

    def call(b):
        cc = windspeed.invert_copol_codes(b[0], b[1], ancillary_wind=b[4], **kw)
        return cc.wind(), cc.dual(b[2], dsig_cr=b[3], model="gmf_s1_v2", resolution="low")

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = _staged(torch, list(sc), list(dec))
        ref_co, ref_dual = call([src for _, src in pairs])  # landed rasters, synchronised: LUTs installed, work lists sized
        torch.cuda.synchronize()
        ref_co, ref_dual = ref_co.cpu().numpy(), ref_dual.cpu().numpy()
        P = torch.cuda.Stream(device=torch.device("cuda", 0))
        with torch.cuda.stream(P):
            done = _held_back(torch, P, delay_cycles, pairs)
            res = call([buf for buf, _ in pairs])
            _in_flight(done)
            got = _read_back(torch, P, *res)
    assert bits_equal(got[0], ref_co) and bits_equal(got[1], ref_dual)
