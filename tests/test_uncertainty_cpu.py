"""CPU: the wind uncertainty from stored grid codes -- its numpy restatement (tests/uncertainty_ref.py) against the reference's
dense cost arrays and a closed form, the argument checks of `CopolCodes.uncertainty` / `.uncertainty_dual` (no library call),
the binding of xsw_uncertainty_from_codes / xsw_uncertainty_cr_from_codes and the engine's hand-over to them.

The restatement is the yardstick of the GPU tests (tests/test_gpu_uncertainty.py), so it is pinned here first: the codes are
built from the oracle's own answer (`invert_numpy(return_idx=True)`), the dense J_co / J_cr arrays of oracle/invert.py:92-96
and :117-122 are formed again per pixel, and the restatement's stencil must be their 3 x 3 (3) block around the arg-min, bit for
bit.  What follows the stencil is + - * / sqrt in float64, written once in the restatement and once in the kernels."""
import os
import re
import threading

import numpy as np
import pytest

import cost_codes_ref as cref
import crosspol_codes_ref as ref
import uncertainty_ref as uref
from conftest import REPO, golden
from test_cost_codes_cpu import _codes
from test_crosspol_codes_cpu import _DeviceArray, _inject, no_library  # noqa: F401 (fixture)
from test_from_codes_plan import SCALAR, check_common, code_bytes, parent_inputs, scene
from test_gpu_kernel import synthetic_scene
from util import bits_equal, small_luts

from oracle import invert as oinv
from oracle import lut as olut


def _dense_blocks(p, inc, s_co_db, s_cr_db, dsig, anc, idx, wind_co, inner_co, inner_cr):
    """Per pixel: the 3 x 3 block of the dense J_co (oracle/invert.py:92-96) around its arg-min where inner_co, the 3 entries of
    the dense J_cr (:117-122) around its arg-min where inner_cr; NaN elsewhere."""
    n = inc.size
    bco, bcr = np.full((n, 3, 3), np.nan), np.full((n, 3), np.nan)
    inc, s_co_db, s_cr_db, dsig, anc = (np.asarray(a).ravel() for a in (inc, s_co_db, s_cr_db, dsig, anc))
    idx, wind_co = idx.reshape(-1, 3), wind_co.ravel()
    with np.errstate(all="ignore"):
        for i in range(n):
            if inner_co[i]:
                lut_inc = p.co_lut[:, :, np.argmin(np.abs(p.inc_dim - inc[i]))]
                m_antenna, m_azi = np.real(anc[i]), np.imag(anc[i])
                if p.phi_180:
                    m_azi = np.abs(m_azi)
                Jwind_co = ((p.lut_co_antenna - m_antenna) / p.d_antenna) ** 2 + ((p.lut_co_azi - m_azi) / p.d_azi) ** 2
                Jsig_co = ((lut_inc - s_co_db[i]) / p.dsig_co) ** 2
                J_co = Jwind_co + Jsig_co
                iw, ip = np.unravel_index(np.argmin(J_co), J_co.shape)
                assert (iw, ip) == (idx[i, 0], idx[i, 1])
                bco[i] = J_co[iw - 1:iw + 2, ip - 1:ip + 2]
            if inner_cr[i]:
                lut_cr_inc = p.cr_lut[:, np.argmin(np.abs(p.inc_cr_dim - inc[i]))]
                Jwind_cr = ((p.wspd_cr - np.abs(wind_co[i])) / p.dwspd_fg) ** 2.0
                Jsig_cr = ((lut_cr_inc - s_cr_db[i]) / dsig[i]) ** 2.0
                J_cr = Jsig_cr + Jwind_cr if not np.isnan(np.abs(wind_co[i])) else Jsig_cr
                k = int(np.argmin(J_cr))
                assert k == idx[i, 2]
                bcr[i] = J_cr[k - 1:k + 2]
    return bco, bcr


def _check_scene(scene_, lco, lcr):
    """Pins the two stencils on one scene; returns (co-pol flags, cross-pol flags)."""
    inc, s_vv, s_vh, dsig, anc = scene_
    p = cref.tables(lco, lcr)
    s_co_db, s_cr_db = oinv.to_db(s_vv), oinv.to_db(s_vh)
    wind_co, _, idx = oinv.invert_numpy(p, inc, s_co_db, s_cr_db, dsig, anc, return_idx=True)
    tab = ref.tables(lco, lcr)
    code_co = ref.co_codes(idx, wind_co, tab)
    code_cr, _ = ref.cross_from_codes(code_co, inc, s_cr_db, dsig, tab)
    code_sel, _ = ref.cross_from_codes(code_co, inc, s_cr_db, dsig, tab, dual_select=True)

    f_co, iw, ip, J_co = uref.stencil_co(code_co, inc, s_co_db, anc, 0.1, p)
    f_cr, icr, J_cr = uref.stencil_cr(code_co, code_cr, inc, s_cr_db, dsig, p)
    flat = idx.reshape(-1, 3)
    assert np.array_equal(f_co == uref.NO_SOLUTION, flat[:, 0] < 0) and np.array_equal(f_cr == uref.NO_SOLUTION, flat[:, 2] < 0)
    assert np.array_equal(iw[f_co == 0], flat[f_co == 0, 0]) and np.array_equal(ip[f_co == 0], flat[f_co == 0, 1])
    assert np.array_equal(icr[f_cr == 0], flat[f_cr == 0, 2])
    nw, nphi, ncr = len(lco.wspd), len(lco.phi), len(lcr.wspd)
    have = flat[:, 0] >= 0
    assert np.array_equal((f_co & uref.WSPD_BORDER) != 0, have & ((flat[:, 0] == 0) | (flat[:, 0] == nw - 1)))
    assert np.array_equal((f_co & uref.PHI_BORDER) != 0, have & ((flat[:, 1] == 0) | (flat[:, 1] == nphi - 1)))
    assert np.array_equal((f_cr & uref.WSPD_BORDER) != 0, (flat[:, 2] == 0) | (flat[:, 2] == ncr - 1))
    bco, bcr = _dense_blocks(p, inc, s_co_db, s_cr_db, dsig, anc, idx, wind_co, f_co == 0, f_cr == 0)
    assert (f_co == 0).sum() > 100 and (f_cr == 0).sum() > 100
    assert bits_equal(J_co, bco), "co-pol: the restatement's stencil is not the 3 x 3 block of the dense J_co around its arg-min"
    assert bits_equal(J_cr, bcr), "cross-pol: the restatement's stencil is not the block of the dense J_cr around its arg-min"

    co = uref.unc_co(code_co, inc, s_co_db, anc, 0.1, p)
    cr = uref.unc_cr(code_co, code_cr, inc, s_cr_db, dsig, p)
    for u, fields in ((co, uref.FIELDS_CO), (cr, ("wspd_std",))):
        for k in fields:
            assert np.array_equal(np.isnan(u[k]), u["flag"] != 0), f"{k} is NaN exactly where a flag is set"
            assert np.all(u[k][u["flag"] == 0] > 0) or k == "corr"
    assert np.all(np.abs(co["corr"][co["flag"] == 0]) < 1.0)  # det > 0
    assert np.array_equal(co["flag"] & 7, f_co.reshape(inc.shape)) and np.all((co["flag"] == uref.NOT_CONVEX) <= (f_co.reshape(inc.shape) == 0))
    # bit 30 of a co-pol code and XSW_CODE_PICK_CO of a cross-pol code do not enter
    flipped = np.where(code_co < 0x80000000, code_co ^ np.uint32(0x40000000), code_co)
    assert np.any(flipped != code_co)
    other = uref.unc_co(flipped, inc, s_co_db, anc, 0.1, p)
    assert all(bits_equal(other[k], co[k]) for k in co)
    assert np.any((code_sel != ref.CODE_NAN_RE) & ((code_sel & ref.CODE_PICK_CO) != 0))
    sel = uref.unc_cr(code_co, code_sel, inc, s_cr_db, dsig, p)
    assert all(bits_equal(sel[k], cr[k]) for k in cr)
    return co["flag"], cr["flag"]


SHARES = {}  # tag -> flags, filled by the parametrised test and read by the one after it


@pytest.mark.parametrize("tag", ["phi180_f64", "phi360_f64", "phi90_f64"])
def test_stencil_is_the_dense_block_on_small_goldens(tag):
    """The restatement gives an estimate (flag 0) for 0.76, 0.79 and 0.33 of the 960 pixels (phi90: 551 solutions sit on the border
    of its 10-point direction axis); cross-pol 0.98."""
    d = golden(f"kernel_small_{tag}.npz")
    lco, lcr = small_luts(d)
    f_co, f_cr = _check_scene(_inject((d["inc"], d["sigma0_vv"], d["sigma0_vh"], d["dsig_cr"], d["anc"])), lco, lcr)
    share_co, share_cr = np.mean(f_co == 0), np.mean(f_cr == 0)
    print(f"{tag}: flag-0 share co-pol {share_co:.3f}, cross-pol {share_cr:.3f}; co-pol flag values {sorted(set(f_co.ravel().tolist()))}")
    assert share_co >= 0.25 and share_cr >= 0.25
    SHARES[tag] = f_co


def test_every_flag_value_occurs_on_a_golden():
    for tag in ("phi180_f64", "phi360_f64", "phi90_f64"):
        if tag not in SHARES:  # (run alone)
            d = golden(f"kernel_small_{tag}.npz")
            inc, s_vv, s_vh, dsig, anc = _inject((d["inc"], d["sigma0_vv"], d["sigma0_vh"], d["dsig_cr"], d["anc"]))
            lco, lcr = small_luts(d)
            p = cref.tables(lco, lcr)
            wind_co, _, idx = oinv.invert_numpy(p, inc, oinv.to_db(s_vv), oinv.to_db(s_vh), dsig, anc, return_idx=True)
            SHARES[tag] = uref.unc_co(ref.co_codes(idx, wind_co, ref.tables(lco, lcr)), inc, oinv.to_db(s_vv), anc, 0.1, p)["flag"]
    seen = set().union(*(set(f.ravel().tolist()) for f in SHARES.values()))
    assert {0, 1, 2, 4, 8} <= seen, seen
    assert 6 in set(SHARES["phi180_f64"].ravel().tolist())  # a corner: both borders


def test_stencil_is_the_dense_block_on_a_default_lut_scene(default_luts):
    """synthetic_scene(16, 96) on the default LUTs (+ the injected classes): the restatement gives 0.94 of 1536 pixels an estimate."""
    f_co, f_cr = _check_scene(_inject(synthetic_scene(16, 96, np.float64, 11)), *default_luts)
    print(f"default LUTs: flag-0 share co-pol {np.mean(f_co == 0):.3f}, cross-pol {np.mean(f_cr == 0):.3f}")
    assert np.mean(f_co == 0) >= 0.75 and np.mean(f_cr == 0) >= 0.75


def test_cross_pol_closed_form():
    """A cross-pol LUT linear in the wind speed, lut = c0 + c1 w on a uniform axis of step h, next to a co-pol wind: J_cr(w) =
    ((c0 + c1 w - s) / dsig)^2 + ((w - |wind_co|) / 2)^2 is a parabola, whose second difference is its second derivative at any
    step: Jww = 2 c1^2 / dsig^2 + 1/2, wspd_std = sqrt(2 / Jww).  Every table entry, axis value and input is a binary fraction,
    so the three J are the parabola's values with at most 8 roundings each (two subtractions, a division, the halving, two
    squares, the sum: 7): |dJ| <= 8 eps max|J|.  The second difference (Jp - 2 J0 + Jm) / h^2 adds them four times over and
    rounds five times more, the square root halves the relative error and rounds twice:
        |d std| / std <= (4 * 8 eps max|J| / h^2 + 5 eps Jww) / (2 Jww) + 2 eps."""
    eps = np.finfo(np.float64).eps
    c0, c1, h, dsig = -30.0, 0.5, 0.25, 0.25
    wcr = np.arange(40) * h
    inc_ax = np.array([30.0, 40.0])
    lcr = olut.Lut(np.stack([c0 + c1 * wcr, c0 + 1.0 + c1 * wcr]), inc_ax, wcr, None, "dB", "x", "cr", "VH")
    w_co, phi = np.arange(12) * 2.0, np.array([0.0, 90.0, 180.0])
    lco = olut.Lut(np.zeros((2, 12, 3)), inc_ax, w_co, phi, "dB", "x", "co", "VV")
    p = cref.tables(lco, lcr)
    icr = np.arange(40, dtype=np.uint32)[None, :].repeat(3, 0)
    code_co = (np.array([2, 5, 9], np.uint32) * 3)[:, None].repeat(40, 1)  # (iw, ip = 0): |wind_co| = w_co[iw] exactly
    assert np.array_equal(np.abs(p.wspd_dim[[2, 5, 9]] * np.exp(1j * np.deg2rad(0.0))), w_co[[2, 5, 9]])
    inc = np.full((3, 40), 31.0)
    s_db = np.full((3, 40), -24.5) + np.arange(3)[:, None] * 2.0
    u = uref.unc_cr(code_co, icr, inc, s_db, np.full((3, 40), dsig), p)
    assert np.all(u["flag"][:, 1:-1] == 0) and np.all(u["flag"][:, [0, -1]] == uref.WSPD_BORDER)
    Jww = 2.0 * c1 ** 2 / dsig ** 2 + 0.5
    want = np.sqrt(2.0 / Jww)
    maxJ = np.nanmax(cref.cost_cr(code_co, icr, inc, s_db, np.full((3, 40), dsig), p)["J"])
    tol = (4 * 8 * eps * maxJ / h ** 2 + 5 * eps * Jww) / (2 * Jww) + 2 * eps
    err = np.max(np.abs(u["wspd_std"][:, 1:-1] - want) / want)
    print(f"closed form: wspd_std {want:.6f} m/s, max relative error {err:.3e}, bound {tol:.3e} (max J {maxJ:.3e})")
    assert err <= tol
    # without a co-pol wind the a-priori term leaves: Jww = 2 c1^2 / dsig^2
    only = uref.unc_cr(None, icr, inc, s_db, np.full((3, 40), dsig), p)
    Jww = 2.0 * c1 ** 2 / dsig ** 2
    tol = (4 * 8 * eps * maxJ / h ** 2 + 5 * eps * Jww) / (2 * Jww) + 2 * eps
    assert np.max(np.abs(only["wspd_std"][:, 1:-1] - np.sqrt(2.0 / Jww)) / np.sqrt(2.0 / Jww)) <= tol


# ------------------------------------------------------------------------------------------------ the public calls' checks
def test_uncertainty_refuses_mismatched_arguments(no_library, xr_env):  # noqa: F811
    from xsarsea_amd import windspeed
    cc = _codes()
    vv, anc = np.full((6, 10), 1e-2, np.float32), np.full((6, 10), 5 + 1j, np.complex64)
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty(vv[:, :9], anc)
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty(vv, anc[:3])
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty(np.full((2, 6, 10), 1e-2, np.float32), anc)
    with pytest.raises(ValueError, match="dtype"):
        cc.uncertainty(vv.astype(np.float64), anc)
    with pytest.raises(ValueError, match="dtype"):
        cc.uncertainty(vv, anc.astype(np.complex128))
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty(_DeviceArray((6, 10)), anc)
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty(vv, _DeviceArray((6, 10), "<c8"))
    dev = windspeed.CopolCodes(_DeviceArray((6, 10)), _DeviceArray((6, 10), "<i4"), lut_co=None)
    with pytest.raises(ValueError, match="container"):
        dev.uncertainty(vv, anc)
    with pytest.raises(ValueError, match="both needed"):
        cc.uncertainty(vv, None)
    with pytest.raises(TypeError, match="xarray"):
        cc.uncertainty(xr_env.xr.DataArray(vv, dims=("line", "sample")), anc)
    with pytest.raises(TypeError, match="xarray"):
        cc.uncertainty(vv, xr_env.xr.DataArray(anc, dims=("line", "sample")))
    with pytest.raises(ValueError, match="dsig_co"):
        cc.uncertainty(vv, anc, dsig_co=0.0)
    with pytest.raises(ValueError, match="dsig_co"):
        cc.uncertainty(vv, anc, dsig_co=float("nan"))
    with pytest.raises(ValueError, match="out_dtype"):
        cc.uncertainty(vv, anc, out_dtype=np.int32)
    bare = windspeed.CopolCodes(np.full((6, 10), 33.0, np.float32), np.zeros((6, 10), np.uint32), lut_co=None)
    with pytest.raises(ValueError, match="shape"):
        bare.uncertainty(vv, np.full((7, 10), 5 + 1j, np.complex64))


def test_uncertainty_dual_refuses_mismatched_arguments(no_library, xr_env):  # noqa: F811
    from xsarsea_amd import windspeed
    cc = _codes()
    vh, ccr = np.full((6, 10), 1e-3, np.float32), np.zeros((6, 10), np.uint32)
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty_dual(vh[:, :9], ccr, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty_dual(vh, ccr[:, :9], model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty_dual(vh, ccr, dsig_cr=np.full((6, 3), 0.1, np.float32), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="both needed"):
        cc.uncertainty_dual(vh, None, model="gmf_s1_v2")
    with pytest.raises(TypeError, match="uint32"):
        cc.uncertainty_dual(vh, ccr.astype(np.int64), model="gmf_s1_v2")
    with pytest.raises(TypeError, match="uint32"):
        cc.uncertainty_dual(vh, ccr.astype(np.float32), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty_dual(_DeviceArray((6, 10)), ccr, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty_dual(vh, _DeviceArray((6, 10), "<i4"), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty_dual(vh, ccr, dsig_cr=_DeviceArray((6, 10)), model="gmf_s1_v2")
    dev = windspeed.CopolCodes(_DeviceArray((6, 10)), _DeviceArray((6, 10), "<i4"), lut_co=None)
    with pytest.raises(ValueError, match="container"):
        dev.uncertainty_dual(vh, _DeviceArray((6, 10), "<i4"), model="gmf_s1_v2")
    da = xr_env.xr.DataArray(vh, dims=("line", "sample"))
    with pytest.raises(TypeError, match="xarray"):
        cc.uncertainty_dual(da, ccr, model="gmf_s1_v2")
    with pytest.raises(TypeError, match="xarray"):
        cc.uncertainty_dual(vh, xr_env.xr.DataArray(ccr, dims=("line", "sample")), model="gmf_s1_v2")
    with pytest.raises(TypeError, match="xarray"):
        cc.uncertainty_dual(vh, ccr, dsig_cr=da, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        cc.uncertainty_dual(vh.astype(np.float64), ccr, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        cc.uncertainty_dual(vh, ccr, dsig_cr=np.full((6, 10), 0.1, np.float64), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        dev.uncertainty_dual(_DeviceArray((6, 10), "<f8"), _DeviceArray((6, 10), "<i4"), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="cross-pol"):
        cc.uncertainty_dual(vh, ccr, model="gmf_cmod5n")
    with pytest.raises(ValueError, match="out_dtype"):
        cc.uncertainty_dual(vh, ccr, model="gmf_s1_v2", resolution="low", out_dtype="complex64")


def test_cost_and_uncertainty_share_their_checks(monkeypatch):
    """dsig_co=None takes the CopolCodes' own for both calls, and both hand the engine the same plan."""
    from xsarsea_amd.windspeed import _engine
    seen = []
    monkeypatch.setattr(_engine, "cost_from_codes", lambda lut, plan, *a, **k: seen.append(("cost", plan.shape, plan.code, plan.is_db, k["dsig_co"])) or [None] * 4)
    monkeypatch.setattr(_engine, "uncertainty_from_codes", lambda lut, plan, *a, **k: seen.append(("unc", plan.shape, plan.code, plan.is_db, k["dsig_co"])) or [None] * 4)
    vv, anc = np.full((6, 10), 1e-2, np.float32), np.full((6, 10), 5 + 1j, np.complex64)
    for kw in (dict(), dict(dsig_co=0.5)):
        _codes(dsig_co=0.25).cost(vv, anc, **kw)
        _codes(dsig_co=0.25).uncertainty(vv, anc, **kw)
    _codes().uncertainty(vv, anc)
    assert [s[0] for s in seen] == ["cost", "unc", "cost", "unc", "unc"]
    assert seen[0][1:] == seen[1][1:] and seen[2][1:] == seen[3][1:] and [s[4] for s in seen] == [0.25, 0.25, 0.5, 0.5, 0.1]


def test_entries_are_declared_and_bound():
    from xsarsea_amd import _lib, windspeed
    txt = open(os.path.join(REPO, "include", "xsw.h")).read()
    for entry, method in (("xsw_uncertainty_from_codes", "uncertainty_from_codes_raw"), ("xsw_uncertainty_cr_from_codes", "uncertainty_cr_from_codes_raw")):
        assert entry in _lib.EXPORTS
        assert callable(getattr(_lib.Context, method))
        assert re.search(rf"\bint\s+{entry}\s*\(\s*xsw_ctx\s*\*", txt)
        assert hasattr(_lib.load(), entry)
    assert re.search(r"#define\s+XSW_VERSION\s+4\b", txt)
    for name, value in (("NO_SOLUTION", 1), ("WSPD_BORDER", 2), ("PHI_BORDER", 4), ("NOT_CONVEX", 8)):
        assert re.search(rf"#define\s+XSW_UNC_{name}\s+{value}u?\b", txt) and getattr(_lib, f"UNC_{name}") == value == getattr(uref, name)
    assert sorted(windspeed.InversionUncertainty.FLAGS.values()) == [1, 2, 4, 8]
    assert windspeed.InversionUncertainty is windspeed.crosspol.InversionUncertainty and "InversionUncertainty" in windspeed.__all__
    u = windspeed.InversionUncertainty(1, 2, 3, 4)
    assert (u["wspd_std"], u["dir_std"], u["corr"], u["flag"]) == (1, 2, 3, 4) and windspeed.InversionUncertainty(1).dir_std is None
    assert "mirror" in windspeed.CopolCodes.uncertainty.__doc__ and "wrap" in windspeed.CopolCodes.uncertainty.__doc__


# ------------------------------------------------------------------------------------------------ the engine's hand-over
class _Recorder:
    """A `Context` without xsw_ctx_create (tests/test_from_codes_plan.py): a lock, a lut_key and the two *_raw methods, which
    record their arguments and copy the host buffers behind the addresses they are given."""

    def __init__(self, log):
        self.lock, self.lut_key, self.log = threading.RLock(), (None, None), log

    def _record(self, call, names, lines, samples, dtype, out_dtype, mem, inputs, outputs, **scalars):
        import ctypes
        n, es = int(lines) * int(samples), 4 if dtype == 0 else 8
        size = {"code_co": 4, "code_cr": 4, "anc": 2 * es}
        self.log.append(dict(call=call, lines=int(lines), samples=int(samples), dtype=dtype, out_dtype=out_dtype, mem=mem, outputs=outputs,
                             bytes={k: None if q is None else ctypes.string_at(int(q), n * size.get(k, es)) for k, q in zip(names, inputs)}, **scalars))

    def uncertainty_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_co, anc, out_wspd_std, out_dir_std=None,
                                   out_corr=None, out_flag=None, dsig_co=0.1, sigma0_is_db=False):
        self._record("unc", ("inc", "code_co", "sigma0", "anc"), lines, samples, dtype, out_dtype, mem, (inc, code_co, sigma0_co, anc),
                     (out_wspd_std, out_dir_std, out_corr, out_flag), dsig_co=dsig_co, is_db=sigma0_is_db)

    def uncertainty_cr_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, code_cr, sigma0_cr, dsig_cr, out_wspd_std,
                                      out_flag=None, dsig_cr_scalar=0.1, sigma0_is_db=False):
        self._record("unc_cr", ("inc", "code_co", "code_cr", "sigma0", "dsig_cr"), lines, samples, dtype, out_dtype, mem,
                     (inc, code_co, code_cr, sigma0_cr, dsig_cr), (out_wspd_std, out_flag), dsig_cr_scalar=dsig_cr_scalar, is_db=sigma0_is_db)


@pytest.fixture
def recorder(monkeypatch):
    from xsarsea_amd import _lib, options
    from xsarsea_amd.windspeed import _engine
    keep = options.db_on_device
    log = []
    ctx = _Recorder(log)
    monkeypatch.setattr(_lib, "default_context", lambda device=0, replica=0: ctx)
    monkeypatch.setattr(_engine, "ensure_luts", lambda c, lut_co, lut_cr: log.append(dict(call="ensure_luts", luts=(lut_co, lut_cr))))
    yield log
    options.db_on_device = keep


@pytest.mark.parametrize("db_on_device", ["auto", False])
@pytest.mark.parametrize("dsig_kind", ["scalar", "raster"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_engine_hands_the_cost_calls_rasters_to_the_library(recorder, dt, dsig_kind, db_on_device):
    """The two engine functions form their inputs as cost_from_codes / cost_cr_from_codes do (tests/test_from_codes_plan.py pins
    those), and hand over three real rasters of out_dtype + a uint8 flag raster (cross-pol: one + one), all of the plan's shape."""
    from xsarsea_amd import _lib, options
    from xsarsea_amd.windspeed import _engine, _plan
    options.db_on_device = db_on_device
    shape = (6, 10)
    inc, s, anc, dsig, cc, ccr = scene(shape, dt, dsig_kind)
    kdt, is_db, scalar, want = parent_inputs(shape, db_on_device, inc, s, dsig, anc)
    meta = lambda a: a if (a is None or np.isscalar(a)) else _plan.meta(a)
    luts = (object(), object())
    for out_dtype in (np.float64, np.float32):
        plan = _plan.CallPlan(_plan.meta(inc), _plan.meta(s), None, None, _plan.meta(anc), device=False)
        del recorder[:]
        outs = _engine.uncertainty_from_codes(luts[0], plan, cc, inc, s, anc, dsig_co=SCALAR, out_dtype=out_dtype)
        assert recorder[0] == dict(call="ensure_luts", luts=(luts[0], None)) and len(recorder) == 2
        rec = recorder[1]
        check_common(rec, shape, dt, is_db)
        full_anc = np.ascontiguousarray(np.broadcast_to(anc, shape), dtype=np.complex64 if dt == np.float32 else np.complex128)
        assert rec["call"] == "unc" and rec["bytes"] == dict(inc=want["inc"], sigma0=want["sigma0"], code_co=code_bytes(cc), anc=full_anc.tobytes())
        assert rec["out_dtype"] == (_lib.XSW_F32 if out_dtype == np.float32 else _lib.XSW_F64) and rec["dsig_co"] == SCALAR
        assert [(o.shape, o.dtype) for o in outs] == [(shape, np.dtype(out_dtype))] * 3 + [(shape, np.dtype(np.uint8))]
        assert rec["outputs"] == tuple(o.ctypes.data for o in outs)

        plan = _engine.cross_plan(shape, meta(inc), meta(s), meta(anc), meta(s), meta(dsig), device=False)
        del recorder[:]
        outs = _engine.uncertainty_cr_from_codes(*luts, plan, cc, ccr, inc, s, dsig, out_dtype=out_dtype)
        assert recorder[0] == dict(call="ensure_luts", luts=luts) and len(recorder) == 2
        rec = recorder[1]
        check_common(rec, shape, dt, is_db)
        assert rec["call"] == "unc_cr" and rec["bytes"] == dict(want, code_co=code_bytes(cc), code_cr=code_bytes(ccr))
        assert rec["out_dtype"] == (_lib.XSW_F32 if out_dtype == np.float32 else _lib.XSW_F64) and rec["dsig_cr_scalar"] == scalar
        assert [(o.shape, o.dtype) for o in outs] == [(shape, np.dtype(out_dtype)), (shape, np.dtype(np.uint8))]
        assert rec["outputs"] == tuple(o.ctypes.data for o in outs)


def test_an_empty_raster_makes_no_call(recorder):
    from xsarsea_amd.windspeed import _engine, _plan
    inc, s, anc = np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros((0, 5), np.complex64)
    plan = _plan.CallPlan(_plan.meta(inc), _plan.meta(s), None, None, _plan.meta(anc), device=False)
    outs = _engine.uncertainty_from_codes(None, plan, np.zeros((0, 5), np.uint32), inc, s, anc)
    assert recorder == [] and outs[0].shape == (0, 5) and outs[3].dtype == np.uint8
