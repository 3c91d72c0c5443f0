"""GPU: wind uncertainty rasters from stored grid codes (xsw_uncertainty_from_codes / xsw_uncertainty_cr_from_codes, kernels
k_unc_co / k_unc_cr; `CopolCodes.uncertainty`, `.uncertainty_dual`).

The yardstick everywhere is the numpy restatement tests/uncertainty_ref.py (its stencil pinned to the reference's dense cost
arrays by tests/test_uncertainty_cpu.py).  Real outputs and flags must equal it bit for bit, NaN positions included; float32
outputs are the restatement rounded once.  Only IEEE + - * / sqrt in float64 follow the stencil, so there is no tolerance.
sigma0 in dB is handed to the restatement as the kernels form it (tests/test_gpu_cost_codes.py: `_db`).

On the CPU, with the C oracle's solutions, the restatement gives 0.979 of the 20504 pixels of `_scene((70, 333), dtype)` that
have a grid code an estimate (96 on a direction border, 330 not convex), for float32 and float64 rasters alike."""
import itertools
import warnings

import numpy as np
import pytest

import cost_codes_ref as cref
import uncertainty_ref as uref
from test_gpu_cost_codes import _db, _differ, _fill, default_ctx, default_tab  # noqa: F401 (fixtures)
from test_gpu_crosspol_codes import _fused, _scene
from test_gpu_streams import ASYNC, _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from util import lut_dicts, small_luts

from conftest import golden
from oracle import invert as oinv
from oracle import lut as olut

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output raster
SENTINEL = {np.float32: np.float32(-7.5e37), np.float64: np.float64(-7.5e300), np.uint8: np.uint8(0xA5)}  # no std, correlation or flag
FIELDS = {"co": ("wspd_std", "dir_std", "corr", "flag"), "cr": ("wspd_std", "flag")}


def _unc(ctx, torch, _lib, kind, arrs, out_t, is_db=False, want=None, mem=None, dsig_co=0.1):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays).  kind "co": arrs = (inc, code_co, sigma0_co, anc) ->
    [wspd_std, dir_std, corr, flag]; "cr": (inc, code_co or None, code_cr, sigma0_cr, dsig_cr or None) -> [wspd_std, flag].
    Every requested output lies between two guard regions and starts as its sentinel; returns host arrays (None where not
    requested) after checking that the guards are untouched and every pixel was written."""
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    types = [out_t] * (3 if kind == "co" else 1) + [np.uint8]
    want = (1,) * len(types) if want is None else want
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    # an empty raster: one-element inputs, so that no pointer is NULL
    hosts = [None if a is None else np.ascontiguousarray(a if n else np.zeros(1, a.dtype)) for a in arrs]
    host_route = mem == _lib.MEM_HOST
    if host_route:
        bufs = [np.full(n + 2 * GUARD, SENTINEL[t], t) if w else None for t, w in zip(types, want)]
        ins = [None if a is None else a.ctypes.data for a in hosts]
        outs = [None if b is None else b.ctypes.data + GUARD * b.itemsize for b in bufs]
    else:
        dev = torch.device("cuda", 0)
        tt = {np.float32: torch.float32, np.float64: torch.float64, np.uint8: torch.uint8}
        keep = [None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in hosts]
        bufs = [torch.full((n + 2 * GUARD,), SENTINEL[t].item(), dtype=tt[t], device=dev) if w else None for t, w in zip(types, want)]
        torch.cuda.synchronize()
        ins = [None if t is None else t.data_ptr() for t in keep]
        outs = [None if b is None else b.data_ptr() + GUARD * b.element_size() for b in bufs]
    m = _lib.MEM_HOST if host_route else _lib.MEM_DEVICE
    if kind == "co":
        ctx.uncertainty_from_codes_raw(shape[0], shape[1], dt, od, m, *ins, *outs, dsig_co=dsig_co, sigma0_is_db=is_db)
    else:
        ctx.uncertainty_cr_from_codes_raw(shape[0], shape[1], dt, od, m, *ins, *outs, dsig_cr_scalar=0.1, sigma0_is_db=is_db)
    ctx.synchronize()
    res = []
    for b, t in zip(bufs, types):
        if b is None:
            res.append(None)
            continue
        h = b if host_route else b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL[t]) and np.all(h[-GUARD:] == SENTINEL[t]), "a guard region was written"
        assert not np.any(h[GUARD:n + GUARD] == SENTINEL[t]), "a pixel was not written"
        res.append(h[GUARD:n + GUARD].reshape(shape).copy())
    return res


def _assert_fields(kind, got, want, out_t, what):
    """Every requested field == the restatement's (reals rounded once to a float32 output), NaN positions included."""
    counts = {}
    for k, g in zip(FIELDS[kind], got):
        if g is not None:
            with np.errstate(all="ignore"):
                counts[k] = _differ(g, want[k] if k == "flag" else want[k].astype(out_t))
            assert g.dtype == (np.uint8 if k == "flag" else out_t)
    print(f"{what}: pixels that differ from the restatement {counts}")
    assert not any(counts.values()), f"{what}: {counts}"


def _same(a, b):
    return all((x is None and y is None) or _differ(x, y) == 0 for x, y in zip(a, b))


@pytest.mark.parametrize("is_db", [0, 1])
@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_equal_to_the_restatement(default_ctx, torch, default_tab, dtype, out_t, is_db):  # noqa: F811
    """70 x 333 (ragged last wave) on the default LUTs, every input class, codes from one fused dual-pol launch: co-pol;
    cross-pol with dsig_cr as a raster and as a scalar; code_co = NULL against the codes of the fused cross-pol-only call."""
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), dtype)
    if is_db:
        s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    s_co_db, s_cr_db = _db(s_vv, is_db, torch), _db(s_vh, is_db, torch)
    for name, d in (("raster", dsig), ("scalar", None)):
        f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, d, anc), np.complex128, False, is_db)
        cc, ccr = f["cc"], f["ccr"]
        assert np.any(cc == _lib.CODE_NAN_RE) and np.any(cc == _lib.CODE_NAN) and np.any(ccr == _lib.CODE_NO_INDEX) and np.any(ccr == _lib.CODE_NAN_RE)
        if d is not None:
            got = _unc(default_ctx, torch, _lib, "co", (inc, cc, s_vv, anc), out_t, is_db)
            want = uref.unc_co(cc, inc, s_co_db, anc, 0.1, default_tab)
            _assert_fields("co", got, want, out_t, "co-pol")
            grid = cc < 0x80000000
            share = np.mean(got[3][grid] == 0)
            print(f"flag-0 share among the {grid.sum()} pixels with a grid code: {share:.4f}; flags {np.unique(got[3], return_counts=True)}")
            assert share >= 0.75
            assert np.array_equal(got[3] == _lib.UNC_NO_SOLUTION, ~grid) and all(np.array_equal(np.isnan(g), got[3] != 0) for g in got[:3])
            assert np.any(got[3] == _lib.UNC_NOT_CONVEX) and np.any(got[3] == _lib.UNC_PHI_BORDER)
        got = _unc(default_ctx, torch, _lib, "cr", (inc, cc, ccr, s_vh, d), out_t, is_db)
        _assert_fields("cr", got, uref.unc_cr(cc, ccr, inc, s_cr_db, dsig if d is not None else _fill(s_vh, 0.1), default_tab), out_t, f"cross-pol, dsig {name}")
        searched = (ccr != _lib.CODE_NAN_RE) & ((ccr & _lib.CODE_NO_INDEX) != _lib.CODE_NO_INDEX)
        assert np.array_equal(got[1] == _lib.UNC_NO_SOLUTION, ~searched) and np.mean(got[1][searched] == 0) >= 0.75
    ccr = _fused(default_ctx, torch, _lib, (inc, None, s_vh, dsig, None), np.complex128, False, is_db)["ccr"]
    got = _unc(default_ctx, torch, _lib, "cr", (inc, None, ccr, s_vh, dsig), out_t, is_db)
    _assert_fields("cr", got, uref.unc_cr(None, ccr, inc, s_cr_db, dsig, default_tab), out_t, "cross-pol, code_co = NULL")
    assert not np.isnan(got[0]).all()


# ------------------------------------------------------------------------------------------------ every grid point of a table
def _synthetic_luts(n_w, n_phi, n_wcr):
    """Smooth dB tables on NON-uniform axes (n_phi = 9: phi_pad = 12, so rows alternate between 8- and 4-entry offsets in a
    64-byte line); with n_w or n_phi below 3 every grid point lies on a border."""
    inc_ax = np.array([20.0, 30.0, 45.0])
    w = np.cumsum(0.5 + 0.25 * (np.arange(n_w) % 3)) - 0.25
    phi = 180.0 * (np.arange(n_phi) / max(n_phi - 1, 1)) ** 1.3 if n_phi > 1 else np.array([0.0])
    wcr = np.cumsum(0.75 + 0.5 * (np.arange(n_wcr) % 2))
    co = -22.0 + 9.0 * np.log10(1.0 + w)[None, :, None] + 2.0 * np.cos(np.deg2rad(2.0 * phi))[None, None, :] * (1.0 + 0.1 * w)[None, :, None] \
        - 0.15 * (inc_ax - 20.0)[:, None, None]
    cr = -36.0 + 12.0 * np.log10(1.0 + wcr)[None, :] - 0.05 * (inc_ax - 20.0)[:, None]
    return (olut.Lut(co, inc_ax, w, phi, "dB", "x", "co", "VV"), olut.Lut(cr, inc_ax, wcr, None, "dB", "x", "cr", "VH"))


def _table_luts(name):
    if name.startswith("golden_"):
        return small_luts(golden(f"kernel_small_{name[7:]}_f64.npz"))
    n_w, n_phi, n_wcr = {"nonuniform_11x9": (11, 9, 13), "degenerate_2x9": (2, 9, 2), "degenerate_9x2": (9, 2, 2), "degenerate_9x1": (9, 1, 1)}[name]
    return _synthetic_luts(n_w, n_phi, n_wcr)


TABLES = ["golden_phi180", "golden_phi360", "golden_phi90", "nonuniform_11x9", "degenerate_2x9", "degenerate_9x2", "degenerate_9x1"]


@pytest.mark.parametrize("name", TABLES)
def test_every_grid_point(gpu_ctx, torch, name):
    """Code rasters that enumerate every (iw, ip) x both values of bit 30 x three incidences (below the axis, between two nodes,
    at the last node), and every icr likewise: every border and corner combination.  sigma0 and the a-priori follow the code's
    own grid point smoothly, so that interior points are mostly convex."""
    from xsarsea_amd import _lib
    lco, lcr = _table_luts(name)
    co, cr = lut_dicts(lco, lcr)
    gpu_ctx.upload_luts(co=co, cr=cr)
    tab = cref.tables(lco, lcr)
    n_w, n_phi, n_wcr = len(lco.wspd), len(lco.phi), len(lcr.wspd)
    plane = n_w * n_phi
    ax = np.asarray(lco.incidence, dtype=np.float64)
    incs = [ax[0] - 1.0, 0.5 * (ax[0] + ax[1]) + 0.3 * (ax[1] - ax[0]), ax[-1]]
    shape = (6, plane)
    flat = np.arange(plane, dtype=np.uint32)
    code = np.stack([flat | np.uint32(bit << 30) for _ in incs for bit in (0, 1)])
    inc = np.repeat(np.array(incs), 2)[:, None] * np.ones((1, plane))
    iw, ip = np.divmod(np.arange(plane), n_phi)
    j = (np.arange(6) // 2)[:, None] * plane + np.arange(plane)[None, :]  # the two rows of a bit-30 pair see the same rasters
    i_inc = np.argmin(np.abs(ax[None, :] - np.array(incs)[:, None]), axis=1).repeat(2)
    s_co = lco.values[i_inc[:, None], iw[None, :], ip[None, :]] + 0.05 * np.sin(0.37 * j)
    w, phi = np.asarray(lco.wspd)[iw], np.asarray(lco.phi)[ip]
    anc = (w * np.exp(1j * np.deg2rad(phi)))[None, :] * (1.0 + 0.02 * np.cos(0.11 * j)) + 0.1j * np.sin(0.23 * j)
    degenerate = name.startswith("degenerate")

    got = _unc(gpu_ctx, torch, _lib, "co", (inc, code, s_co, anc), np.float64, True)
    want = uref.unc_co(code, inc, s_co, anc, 0.1, tab)
    _assert_fields("co", got, want, np.float64, f"{name} co-pol")
    on_w, on_p = (iw == 0) | (iw == n_w - 1), (ip == 0) | (ip == n_phi - 1)
    assert np.array_equal(got[3] & 6, np.broadcast_to(2 * on_w + 4 * on_p, shape)) and not np.any(got[3] & 1)
    if degenerate:
        assert np.all(got[3] != 0) and all(np.isnan(g).all() for g in got[:3])
    else:
        seen = set(got[3].ravel().tolist())
        assert {0, 2, 4, 6} <= seen and np.mean(got[3][:, ~(on_w | on_p)] == 0) > 0.5, seen
        assert _differ(got[0][0], got[0][1]) == 0  # bit 30 does not enter

    icr = (np.arange(plane) % n_wcr).astype(np.uint32)
    ccr = np.stack([icr | np.uint32(bit << 30) for _ in incs for bit in (0, 1)])  # XSW_CODE_PICK_CO set in every other row
    i_inc_cr = np.argmin(np.abs(np.asarray(lcr.incidence)[None, :] - np.array(incs)[:, None]), axis=1).repeat(2)
    s_cr = lcr.values[i_inc_cr[:, None], icr[None, :]] + 0.05 * np.sin(0.29 * j)
    dsig = 0.1 + 0.05 * (1.0 + np.sin(0.13 * j))
    for cco in (code, None):
        got = _unc(gpu_ctx, torch, _lib, "cr", (inc, cco, ccr, s_cr, dsig), np.float64, True)
        _assert_fields("cr", got, uref.unc_cr(cco, ccr, inc, s_cr, dsig, tab), np.float64, f"{name} cross-pol, code_co {'given' if cco is not None else 'NULL'}")
        on = (icr == 0) | (icr == n_wcr - 1)
        assert np.array_equal(got[1] & 2, np.broadcast_to(2 * on, shape).astype(np.uint8)) and not np.any(got[1] & 5)
        if degenerate:
            assert np.all(got[1] == 2)
        else:
            assert np.mean(got[1][:, ~on] == 0) > 0.5


# ------------------------------------------------------------------------------------------------ shapes, codes, routes, outputs
@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (3, 64), (0, 5)])
def test_small_shapes(default_ctx, torch, default_tab, shape):  # noqa: F811
    """One lane, one lane past a wave, whole waves, no pixel at all (the calls return and write nothing)."""
    from xsarsea_amd import _lib
    if 0 in shape:
        z = np.zeros(shape)
        for kind, arrs in (("co", (z, z.astype(np.uint32), z, z.astype(np.complex128))), ("cr", (z, z.astype(np.uint32), z.astype(np.uint32), z, z))):
            assert all(g.shape == shape for g in _unc(default_ctx, torch, _lib, kind, arrs, np.float64, True))
            assert all(g.shape == shape for g in _unc(default_ctx, torch, _lib, kind, arrs, np.float32, True, mem=_lib.MEM_HOST))
        return
    inc, s_vv, s_vh, dsig, anc = _scene(shape, np.float64, 5)
    inc[0, 0], s_vv[0, 0], s_vh[0, 0], dsig[0, 0], anc[0, 0] = 33.0, 0.02, 2e-3, 0.1, 7 + 2j
    inc[-1, -1], s_vv[-1, -1], s_vh[-1, -1], dsig[-1, -1], anc[-1, -1] = 40.0, 0.03, 1e-3, 0.5, 5 - 1j  # a searched pixel in the last lane
    s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, False, is_db=True)
    assert f["cc"][-1, -1] < 0x80000000 and f["ccr"][-1, -1] < _lib.CODE_NO_INDEX
    got = _unc(default_ctx, torch, _lib, "co", (inc, f["cc"], s_vv, anc), np.float64, True)
    _assert_fields("co", got, uref.unc_co(f["cc"], inc, s_vv, anc, 0.1, default_tab), np.float64, f"{shape} co-pol")
    assert got[3][-1, -1] == 0 and got[3][0, 0] == 0
    _assert_fields("cr", _unc(default_ctx, torch, _lib, "cr", (inc, f["cc"], f["ccr"], s_vh, dsig), np.float64, True),
                   uref.unc_cr(f["cc"], f["ccr"], inc, s_vh, dsig, default_tab), np.float64, f"{shape} cross-pol")


def test_foreign_codes(default_ctx, torch, default_tab, default_luts):  # noqa: F811
    """Words that are no code of the installed LUT (bit 31 set, an index at or beyond the table, with or without bit 30), cross-pol
    indices beyond the table, a NaN incidence next to a valid code: flag 1, NaN, and no table is read (the indices would lie
    far outside)."""
    from xsarsea_amd import _lib
    lco, lcr = default_luts
    plane, n_wcr = len(lco.wspd) * len(lco.phi), len(lcr.wspd)
    inc, s_vv, s_vh, dsig, anc = _scene((9, 333), np.float64, 31)
    s_vv, s_vh = oinv.to_db(s_vv), oinv.to_db(s_vh)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex128, False, is_db=True)
    cc, ccr = f["cc"].copy(), f["ccr"].copy()
    ok = np.flatnonzero(((cc < 0x80000000) & ((ccr & _lib.CODE_NO_INDEX) < n_wcr) & (ccr != _lib.CODE_NAN_RE)).ravel())
    assert ok.size > 200
    bad_co = [0x80000000, plane, plane + 7, 0x40000000 | plane, 0xC0000001, 0x3FFFFFFF, 0xBFFFFFFF]
    pick = ok[10:10 + len(bad_co)]
    cc.ravel()[pick] = bad_co
    nan_inc = ok[40:44]
    inc = inc.copy()
    inc.ravel()[nan_inc] = np.nan
    got = _unc(default_ctx, torch, _lib, "co", (inc, cc, s_vv, anc), np.float64, True)
    _assert_fields("co", got, uref.unc_co(cc, inc, s_vv, anc, 0.1, default_tab), np.float64, "foreign co-pol codes")
    for at in (pick, nan_inc):
        assert np.all(got[3].ravel()[at] == 1) and all(np.isnan(g.ravel()[at]).all() for g in got[:3])
    bad_cr = [n_wcr, n_wcr + 1, 0x3FFFFFFE, 0x40000000 | n_wcr, 0x7FFFFFFE, 0xBFFFFFFF]
    pick_cr = ok[60:60 + len(bad_cr)]
    ccr.ravel()[pick_cr] = bad_cr
    got = _unc(default_ctx, torch, _lib, "cr", (inc, cc, ccr, s_vh, dsig), np.float64, True)
    _assert_fields("cr", got, uref.unc_cr(cc, ccr, inc, s_vh, dsig, default_tab), np.float64, "foreign codes, cross-pol")
    for at in (pick_cr, nan_inc):
        assert np.all(got[1].ravel()[at] == 1) and np.isnan(got[0].ravel()[at]).all()
    assert np.all(got[1].ravel()[pick] != 1)  # a foreign co-pol code: no a-priori term, the cross-pol pixel keeps its estimate or its own flag


def test_host_route_equals_device_route(default_ctx, torch):  # noqa: F811
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene((70, 333), np.float32, 23)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex64, True)
    for kind, arrs in (("co", (inc, f["cc"], s_vv, anc)), ("cr", (inc, f["cc"], f["ccr"], s_vh, dsig)), ("cr", (inc, None, f["ccr"], s_vh, None))):
        for out_t, want in ((np.float32, None), (np.float64, (1, 0, 0, 1) if kind == "co" else (0, 1))):
            a = _unc(default_ctx, torch, _lib, kind, arrs, out_t, want=want)
            b = _unc(default_ctx, torch, _lib, kind, arrs, out_t, want=want, mem=_lib.MEM_HOST)
            assert np.any(a[-1] == 0) and _same(a, b), f"{kind}, {np.dtype(out_t).name}"


def test_every_subset_of_outputs(default_ctx, torch):  # noqa: F811
    """Each of the 15 (co-pol) and 3 (cross-pol) non-empty subsets writes the bits of the all-outputs run and (inside _unc)
    nothing else; no output at all is XSW_EINVAL."""
    from xsarsea_amd import _lib
    inc, s_vv, s_vh, dsig, anc = _scene((9, 333), np.float32, 7)
    f = _fused(default_ctx, torch, _lib, (inc, s_vv, s_vh, dsig, anc), np.complex64, False)
    for kind, arrs in (("co", (inc, f["cc"], s_vv, anc)), ("cr", (inc, f["cc"], f["ccr"], s_vh, dsig))):
        n = len(FIELDS[kind])
        full = _unc(default_ctx, torch, _lib, kind, arrs, np.float64)
        assert np.any(full[-1] == 0) and np.any(full[-1] != 0)
        for want in itertools.product((0, 1), repeat=n):
            if not any(want):
                with pytest.raises(_lib.XswError, match=r"\(-1\).*no output"):
                    _unc(default_ctx, torch, _lib, kind, arrs, np.float64, want=want)
                continue
            got = _unc(default_ctx, torch, _lib, kind, arrs, np.float64, want=want)
            assert [g is not None for g in got] == [bool(w) for w in want]
            assert _same(got, [g if w else None for g, w in zip(full, want)]), f"{kind}: outputs {want}"


def test_error_codes(torch, default_luts):
    """XSW_EINVAL (-1) with a message, before any launch: the outputs keep their fill."""
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a, z = np.full((2, 8), 33.0, np.float32), np.full((2, 8), 5 + 1j, np.complex64)
        c = np.zeros((2, 8), np.uint32)
        o, fl = np.full((2, 8), 77.0, np.float32), np.full((2, 8), 0xA5, np.uint8)
        p = lambda x: None if x is None else x.ctypes.data
        msg = lambda: ctx._lib.xsw_last_error(ctx._h).decode()
        co = lambda outs=(o, None, None, fl), dsig_co=0.1, shape=(2, 8), ins=(a, c, a, z), dtype=0, mem=0: ctx._lib.xsw_uncertainty_from_codes(
            ctx._h, *shape, dtype, 0, mem, 0, *(p(x) for x in ins), dsig_co, *(p(x) for x in outs))
        cr = lambda outs=(o, fl), code_co=None, shape=(2, 8), code_cr=c: ctx._lib.xsw_uncertainty_cr_from_codes(
            ctx._h, *shape, 0, 0, 0, 0, p(a), p(code_co), p(code_cr), p(a), None, 0.1, *(p(x) for x in outs))
        assert co() == -1 and "no co-pol LUT" in msg()
        assert cr() == -1 and "no cross-pol LUT" in msg()
        lut_co, lut_cr = lut_dicts(*default_luts)
        ctx.upload_luts(cr=lut_cr)
        assert cr(code_co=c) == -1 and "co-pol" in msg()  # co-pol codes without their LUT
        assert cr() == 0
        ctx.upload_luts(co=lut_co)
        assert co((None,) * 4) == -1 and "no output" in msg()
        assert cr((None,) * 2) == -1 and "no output" in msg()
        assert co(dsig_co=0.0) == -1 and "dsig_co" in msg()
        assert co(dsig_co=float("nan")) == -1 and "dsig_co" in msg()
        assert co(shape=(1 << 31, 1 << 31)) == -1 and "too large" in msg()
        assert cr(shape=(1 << 31, 1 << 31)) == -1 and "too large" in msg()
        for k in range(4):
            assert co(ins=tuple(None if j == k else x for j, x in enumerate((a, c, a, z)))) == -1 and "NULL" in msg()
        assert cr(code_cr=None) == -1 and "NULL" in msg()
        assert co(dtype=2) == -1 and co(mem=7) == -1
        o[...], fl[...] = 77.0, 0xA5
        assert co(shape=(-1, 8)) == -1
        ctx.synchronize()
        assert np.all(o == 77.0) and np.all(fl == 0xA5), "a refused call wrote its output"
        assert co() == 0 and cr(code_co=c) == 0
        assert np.all(fl != 0xA5)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public calls
@pytest.mark.parametrize("container", ["numpy", "torch"])
def test_public_api(gpu_ctx, torch, container):
    """cc.uncertainty / cc.uncertainty_dual == the raw entries on the rasters the engine forms == the restatement; out_dtype;
    dsig_co from invert_copol_codes; codes with and without the select give the same cross-pol result."""
    from xsarsea_amd import _lib, windspeed
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
    raw_s = (lambda x: (x, False)) if container == "torch" else (lambda x: (oinv.to_db(x), True))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, dsig_co=0.2, model="gmf_cmod5n", resolution="low")
        lut_co, lut_cr = cc.lut_co, _engine.lut_source(get_model("gmf_s1_v2"), dict(resolution="low"))
        tab = cref.tables(lut_co, lut_cr)
        codes = host(cc.codes).view(np.uint32)
        u = cc.uncertainty(s_vv, anc)
        assert isinstance(u, windspeed.InversionUncertainty) and u["flag"] is u.flag
        got = [host(u[k]) for k in FIELDS["co"]]
        assert all(g.shape == (70, 333) for g in got) and [g.dtype for g in got] == [np.float64] * 3 + [np.uint8]
        _assert_fields("co", got, uref.unc_co(codes, h_inc, to_db(h_vv), h_anc, 0.2, tab), np.float64, f"{container} uncertainty")
        assert np.mean(got[3][codes < 0x80000000] == 0) > 0.5
        co, cr = lut_dicts(lut_co, lut_cr)
        gpu_ctx.upload_luts(co=co, cr=cr)
        s, is_db = raw_s(h_vv)
        assert _same(got, _unc(gpu_ctx, torch, _lib, "co", (h_inc, codes, s, h_anc), np.float64, is_db, dsig_co=0.2)), "not the raw entry's bits"
        u32 = cc.uncertainty(s_vv, anc, dsig_co=0.1, out_dtype=np.float32)
        got32 = [host(u32[k]) for k in FIELDS["co"]]
        assert got32[0].dtype == np.float32
        _assert_fields("co", got32, uref.unc_co(codes, h_inc, to_db(h_vv), h_anc, 0.1, tab), np.float32, f"{container} uncertainty, float32, dsig_co 0.1")
        for d in (dsig, 0.1):
            kw = dict(dsig_cr=d, model="gmf_s1_v2", resolution="low")
            sel, raw = cc.dual(s_vh, codes=True, dual_select=True, **kw), cc.dual(s_vh, codes=True, dual_select=False, **kw)
            assert np.any(host(sel).view(np.uint32) != host(raw).view(np.uint32))
            a, b = cc.uncertainty_dual(s_vh, sel, **kw), cc.uncertainty_dual(s_vh, raw, **kw)
            assert a.dir_std is None and a.corr is None
            ga, gb = ([host(c[k]) for k in FIELDS["cr"]] for c in (a, b))
            assert _same(ga, gb), "uncertainty_dual depends on the select"
            h_d = h_dsig if d is dsig else _fill(h_vh, 0.1)
            _assert_fields("cr", ga, uref.unc_cr(codes, host(raw).view(np.uint32), h_inc, to_db(h_vh), h_d, tab), np.float64,
                           f"{container} uncertainty_dual, dsig_cr {'raster' if d is dsig else d}")
            s, is_db = raw_s(h_vh)
            assert _same(ga, _unc(gpu_ctx, torch, _lib, "cr", (h_inc, codes, host(raw).view(np.uint32), s, h_d), np.float64, is_db)), "not the raw entry's bits"
        f32 = cc.uncertainty_dual(s_vh, raw, out_dtype=np.float32, **kw)
        assert host(f32.wspd_std).dtype == np.float32 and _differ(host(f32.wspd_std), ga[0].astype(np.float32)) == 0 and _differ(host(f32.flag), ga[1]) == 0


def test_user_stream_without_an_intermediate_sync(gpu_ctx, torch, delay_cycles):  # noqa: F811
    """invert_copol_codes, .dual(codes=True), .uncertainty and .uncertainty_dual back to back on a user stream whose producer is
    held back: all return while it is in flight, the result is consumed on that stream and equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _scene((48, 260), np.float32, 51), _scene((48, 260), np.float32, 52)
    kw = dict(model="gmf_cmod5n", resolution="low", **ASYNC)
    cr = dict(model="gmf_s1_v2", resolution="low")

    def call(b):
        cc = windspeed.invert_copol_codes(b[0], b[1], ancillary_wind=b[4], **kw)
        ccr = cc.dual(b[2], dsig_cr=b[3], codes=True, **cr)
        co, du = cc.uncertainty(b[1], b[4]), cc.uncertainty_dual(b[2], ccr, dsig_cr=b[3], **cr)
        return co.wspd_std, co.dir_std, co.corr, co.flag, du.wspd_std, du.flag

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
