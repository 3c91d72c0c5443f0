"""CPU: the inversion cost from stored grid codes -- its numpy restatement (tests/cost_codes_ref.py) against the minimum of the
oracle's dense cost arrays, the argument checks of `CopolCodes.cost` / `.cost_dual` (no library call), and the binding of
xsw_cost_from_codes / xsw_cost_cr_from_codes.

The restatement is the yardstick of the GPU tests (tests/test_gpu_cost_codes.py), so it is pinned here first: the codes are
built from the oracle's own answer (`invert_numpy(return_idx=True)`), the dense J_co / J_cr arrays of oracle/invert.py:92-96
and :117-122 are formed again per pixel, and the restatement's J must be their minimum -- the element the arg-min picked --
bit for bit."""
import os
import re

import numpy as np
import pytest

import cost_codes_ref as cref
import crosspol_codes_ref as ref
from conftest import REPO, golden
from test_crosspol_codes_cpu import _DeviceArray, _inject, no_library  # noqa: F401 (fixture)
from test_gpu_kernel import synthetic_scene
from util import bits_equal, small_luts

from oracle import invert as oinv


def _dense_minima(p, inc, s_co_db, s_cr_db, dsig, anc, idx, wind_co):
    """Per pixel: (J_co.min(), J_cr.min()) of the dense arrays oracle/invert.py:92-96 / :117-122 forms, NaN where that search did
    not run (idx < 0); also asserts that the minimum is the element at the oracle's arg-min."""
    shape = inc.shape
    jco, jcr = np.full(inc.size, np.nan), np.full(inc.size, np.nan)
    inc, s_co_db, s_cr_db, dsig, anc = (np.asarray(a).ravel() for a in (inc, s_co_db, s_cr_db, dsig, anc))
    idx, wind_co = idx.reshape(-1, 3), wind_co.ravel()
    with np.errstate(all="ignore"):
        for i in range(inc.size):
            if idx[i, 0] >= 0:
                lut_inc = p.co_lut[:, :, np.argmin(np.abs(p.inc_dim - inc[i]))]
                m_antenna, m_azi = np.real(anc[i]), np.imag(anc[i])
                if p.phi_180:
                    m_azi = np.abs(m_azi)
                Jwind_co = ((p.lut_co_antenna - m_antenna) / p.d_antenna) ** 2 + ((p.lut_co_azi - m_azi) / p.d_azi) ** 2
                Jsig_co = ((lut_inc - s_co_db[i]) / p.dsig_co) ** 2
                J_co = Jwind_co + Jsig_co
                assert np.argmin(J_co) == idx[i, 0] * J_co.shape[-1] + idx[i, 1]
                jco[i] = J_co.min()
                assert jco[i] == J_co.ravel()[np.argmin(J_co)]
            if idx[i, 2] >= 0:
                lut_cr_inc = p.cr_lut[:, np.argmin(np.abs(p.inc_cr_dim - inc[i]))]
                Jwind_cr = ((p.wspd_cr - np.abs(wind_co[i])) / p.dwspd_fg) ** 2.0
                Jsig_cr = ((lut_cr_inc - s_cr_db[i]) / dsig[i]) ** 2.0
                J_cr = Jsig_cr + Jwind_cr if not np.isnan(np.abs(wind_co[i])) else Jsig_cr
                assert np.argmin(J_cr) == idx[i, 2]
                jcr[i] = J_cr.min()
    return jco.reshape(shape), jcr.reshape(shape)


def _all_nan(c, mask):
    return all(np.isnan(c[k][mask]).all() for k in cref.FIELDS)


def _check_scene(scene, lco, lcr):
    inc, s_vv, s_vh, dsig, anc = scene
    p = cref.tables(lco, lcr)
    s_co_db, s_cr_db = oinv.to_db(s_vv), oinv.to_db(s_vh)
    wind_co, _, idx = oinv.invert_numpy(p, inc, s_co_db, s_cr_db, dsig, anc, return_idx=True)
    tab = ref.tables(lco, lcr)
    code_co = ref.co_codes(idx, wind_co, tab)
    code_cr, _ = ref.cross_from_codes(code_co, inc, s_cr_db, dsig, tab)
    code_sel, _ = ref.cross_from_codes(code_co, inc, s_cr_db, dsig, tab, dual_select=True)
    assert np.array_equal(np.where((code_cr == ref.CODE_NAN_RE) | (code_cr == ref.CODE_NO_INDEX), -1, code_cr.astype(np.int64)), idx[..., 2])
    jco, jcr = _dense_minima(p, inc, s_co_db, s_cr_db, dsig, anc, idx, wind_co)

    co = cref.cost_co(code_co, inc, s_co_db, anc, 0.1, p)
    cr = cref.cost_cr(code_co, code_cr, inc, s_cr_db, dsig, p)
    assert bits_equal(co["J"], jco), "co-pol: the restatement's J is not the minimum of the dense J_co"
    assert bits_equal(cr["J"], jcr), "cross-pol: the restatement's J is not the minimum of the dense J_cr"
    with np.errstate(all="ignore"):
        assert bits_equal(co["Jwind"] + co["Jsig"], co["J"])  # :96
        have_co = ~np.isnan(cr["Jwind"])
        assert bits_equal(np.where(have_co, cr["Jsig"] + cr["Jwind"], cr["Jsig"]), cr["J"])  # :119-122
    # XSW_CODE_PICK_CO does not enter the cost
    sel = cref.cost_cr(code_co, code_sel, inc, s_cr_db, dsig, p)
    assert np.any((code_sel != ref.CODE_NAN_RE) & ((code_sel & ref.CODE_PICK_CO) != 0))
    assert all(bits_equal(sel[k], cr[k]) for k in cref.FIELDS)
    # cross-pol only (no co-pol codes): J = Jsig wherever a cross-pol search ran
    only = cref.cost_cr(None, code_cr, inc, s_cr_db, dsig, p)
    assert bits_equal(only["J"], only["Jsig"]) and np.isnan(only["Jwind"]).all() and bits_equal(only["Jsig"], cr["Jsig"])

    # every unsearched class is NaN in all four fields, and occurs
    early_inc = np.isnan(inc)
    early_anc = ~early_inc & (code_co == ref.CODE_NAN_RE)
    no_co = code_co == ref.CODE_NAN
    no_cr_s0 = ~early_inc & ~early_anc & np.isnan(s_cr_db)
    no_cr_dsig = ~early_inc & ~early_anc & ~np.isnan(s_cr_db) & np.isnan(dsig)
    for name, m, fields in (("early NaN by incidence", early_inc, (co, cr)), ("early NaN by ancillary wind", early_anc, (co, cr)),
                            ("no co-pol search", no_co, (co,)), ("no cross-pol search by sigma0_cr", no_cr_s0, (cr,)),
                            ("no cross-pol search by dsig_cr", no_cr_dsig, (cr,))):
        assert m.any(), f"no pixel of class: {name}"
        for c in fields:
            assert _all_nan(c, m), f"{name}: a field is not NaN"
    assert np.all(code_cr[no_cr_s0 | no_cr_dsig] == ref.CODE_NO_INDEX) and np.all(code_cr[early_inc | early_anc] == ref.CODE_NAN_RE)
    searched_co = ~early_inc & ~early_anc & ~no_co
    assert not np.isnan(co["J"][searched_co]).any() and not np.isnan(cr["Jsig"][~early_inc & ~early_anc & ~no_cr_s0 & ~no_cr_dsig]).any()
    # foreign codes: bit 31 set without being a NaN code, an index beyond the table
    plane = len(lco.wspd) * len(lco.phi)
    foreign = code_co.copy()
    pick = np.flatnonzero(searched_co.ravel())[:6]
    foreign.ravel()[pick] = [0x80000000, 0x80000005, plane, plane + 7, 0x40000000 | plane, 0xC0000001]
    fco = cref.cost_co(foreign, inc, s_co_db, anc, 0.1, p)
    fm = np.zeros(inc.size, bool)
    fm[pick] = True
    fm = fm.reshape(inc.shape)
    assert _all_nan(fco, fm) and all(bits_equal(fco[k][~fm], co[k][~fm]) for k in cref.FIELDS)
    fcr = cref.cost_cr(foreign, code_cr, inc, s_cr_db, dsig, p)  # no co-pol wind there: J = Jsig
    assert np.isnan(fcr["Jwind"][fm]).all() and bits_equal(fcr["J"][fm], fcr["Jsig"][fm])
    bad_cr = code_cr.copy()
    bad_cr.ravel()[pick[:2]] = [len(lcr.wspd), 0x3FFFFFFE]  # an index beyond the cross-pol table
    assert _all_nan(cref.cost_cr(code_co, bad_cr, inc, s_cr_db, dsig, p), fm & (bad_cr != code_cr))


@pytest.mark.parametrize("tag", ["phi180_f64", "phi360_f64", "phi90_f64"])
def test_restatement_is_the_minimum_on_small_goldens(tag):
    d = golden(f"kernel_small_{tag}.npz")
    lco, lcr = small_luts(d)
    assert cref.tables(lco, lcr).phi_180 == (tag != "phi90_f64")  # (:152-156 is true of a 0..360 axis too: phi90 alone keeps Im(anc) signed)
    _check_scene(_inject((d["inc"], d["sigma0_vv"], d["sigma0_vh"], d["dsig_cr"], d["anc"])), lco, lcr)


def test_restatement_is_the_minimum_on_a_default_lut_scene(default_luts):
    """synthetic_scene(16, 96) on the default LUTs (+ the injected classes): 1536 dense cost arrays."""
    _check_scene(_inject(synthetic_scene(16, 96, np.float64, 11)), *default_luts)


# ------------------------------------------------------------------------------------------------ the public calls' checks
def _codes(shape=(6, 10), dtype=np.float32, **kw):
    from xsarsea_amd import windspeed
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    return windspeed.CopolCodes(np.full(shape, 33.0, dtype), np.zeros(shape, np.uint32), lut_co=None, sigma0_meta=(shape, np.dtype(dtype)),
                                ancillary_meta=(shape, np.dtype(cdt)), **kw)


def test_cost_refuses_mismatched_arguments(no_library, xr_env):  # noqa: F811
    from xsarsea_amd import windspeed
    cc = _codes()
    vv, anc = np.full((6, 10), 1e-2, np.float32), np.full((6, 10), 5 + 1j, np.complex64)
    with pytest.raises(ValueError, match="shape"):
        cc.cost(vv[:, :9], anc)
    with pytest.raises(ValueError, match="shape"):
        cc.cost(vv, anc[:3])
    with pytest.raises(ValueError, match="shape"):
        cc.cost(np.full((2, 6, 10), 1e-2, np.float32), anc)  # would broadcast the codes
    with pytest.raises(ValueError, match="dtype"):
        cc.cost(vv.astype(np.float64), anc)  # not the raster the search saw
    with pytest.raises(ValueError, match="dtype"):
        cc.cost(vv, anc.astype(np.complex128))
    with pytest.raises(ValueError, match="container"):
        cc.cost(_DeviceArray((6, 10)), anc)
    with pytest.raises(ValueError, match="container"):
        cc.cost(vv, _DeviceArray((6, 10), "<c8"))
    dev = windspeed.CopolCodes(_DeviceArray((6, 10)), _DeviceArray((6, 10), "<i4"), lut_co=None)
    with pytest.raises(ValueError, match="container"):
        dev.cost(vv, anc)
    da = xr_env.xr.DataArray(vv, dims=("line", "sample"))
    with pytest.raises(TypeError, match="xarray"):
        cc.cost(da, anc)
    with pytest.raises(TypeError, match="xarray"):
        cc.cost(vv, xr_env.xr.DataArray(anc, dims=("line", "sample")))
    with pytest.raises(ValueError, match="dsig_co"):
        cc.cost(vv, anc, dsig_co=0.0)
    with pytest.raises(ValueError, match="dsig_co"):
        cc.cost(vv, anc, dsig_co=float("nan"))
    with pytest.raises(ValueError, match="out_dtype"):
        cc.cost(vv, anc, out_dtype=np.int32)
    # a CopolCodes built by hand without the ancillary wind's (shape, dtype): the shape is still checked against the codes
    bare = windspeed.CopolCodes(np.full((6, 10), 33.0, np.float32), np.zeros((6, 10), np.uint32), lut_co=None)
    with pytest.raises(ValueError, match="shape"):
        bare.cost(vv, np.full((7, 10), 5 + 1j, np.complex64))


def test_cost_dual_refuses_mismatched_arguments(no_library, xr_env):  # noqa: F811
    from xsarsea_amd import windspeed
    cc = _codes()
    vh, ccr = np.full((6, 10), 1e-3, np.float32), np.zeros((6, 10), np.uint32)
    with pytest.raises(ValueError, match="shape"):
        cc.cost_dual(vh[:, :9], ccr, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.cost_dual(vh, ccr[:, :9], model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.cost_dual(vh, ccr, dsig_cr=np.full((6, 3), 0.1, np.float32), model="gmf_s1_v2")
    with pytest.raises(TypeError, match="uint32"):
        cc.cost_dual(vh, ccr.astype(np.int64), model="gmf_s1_v2")
    with pytest.raises(TypeError, match="uint32"):
        cc.cost_dual(vh, ccr.astype(np.float32), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.cost_dual(_DeviceArray((6, 10)), ccr, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.cost_dual(vh, _DeviceArray((6, 10), "<i4"), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.cost_dual(vh, ccr, dsig_cr=_DeviceArray((6, 10)), model="gmf_s1_v2")
    dev = windspeed.CopolCodes(_DeviceArray((6, 10)), _DeviceArray((6, 10), "<i4"), lut_co=None)
    with pytest.raises(ValueError, match="container"):
        dev.cost_dual(vh, _DeviceArray((6, 10), "<i4"), model="gmf_s1_v2")
    da = xr_env.xr.DataArray(vh, dims=("line", "sample"))
    with pytest.raises(TypeError, match="xarray"):
        cc.cost_dual(da, ccr, model="gmf_s1_v2")
    with pytest.raises(TypeError, match="xarray"):
        cc.cost_dual(vh, xr_env.xr.DataArray(ccr, dims=("line", "sample")), model="gmf_s1_v2")
    with pytest.raises(TypeError, match="xarray"):
        cc.cost_dual(vh, ccr, dsig_cr=da, model="gmf_s1_v2")
    # the dtype / dB-route check `.dual` makes
    with pytest.raises(ValueError, match="dtype"):
        cc.cost_dual(vh.astype(np.float64), ccr, model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        cc.cost_dual(vh, ccr, dsig_cr=np.full((6, 10), 0.1, np.float64), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        dev.cost_dual(_DeviceArray((6, 10), "<f8"), _DeviceArray((6, 10), "<i4"), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="cross-pol"):
        cc.cost_dual(vh, ccr, model="gmf_cmod5n")
    with pytest.raises(ValueError, match="out_dtype"):
        cc.cost_dual(vh, ccr, model="gmf_s1_v2", resolution="low", out_dtype="complex64")


def test_dsig_co_defaults_to_the_stored_value(monkeypatch):
    """dsig_co=None takes the CopolCodes' own (what invert_copol_codes was given), else 0.1; an explicit value wins."""
    from xsarsea_amd.windspeed import _engine
    seen = []
    monkeypatch.setattr(_engine, "cost_from_codes", lambda *a, **k: seen.append(k["dsig_co"]) or [None] * 4)
    vv, anc = np.full((6, 10), 1e-2, np.float32), np.full((6, 10), 5 + 1j, np.complex64)
    _codes(dsig_co=0.25).cost(vv, anc)
    _codes().cost(vv, anc)
    _codes(dsig_co=0.25).cost(vv, anc, dsig_co=0.5)
    assert seen == [0.25, 0.1, 0.5]


def test_invert_copol_codes_stores_its_dsig_co(monkeypatch):
    from xsarsea_amd import windspeed
    from xsarsea_amd.windspeed import _engine
    monkeypatch.setattr(_engine, "lut_source", lambda m, kw: None)
    monkeypatch.setattr(_engine, "invert_numpy", lambda lco, lcr, inc, *a, **k: (np.zeros(np.shape(inc), np.uint32), None))
    inc, vv, anc = np.full((4, 5), 33.0), np.full((4, 5), 1e-2), np.full((4, 5), 5 + 1j)
    assert windspeed.invert_copol_codes(inc, vv, ancillary_wind=anc, dsig_co=0.3, model="gmf_cmod5n").dsig_co == 0.3
    assert windspeed.invert_copol_codes(inc, vv, ancillary_wind=anc, model="gmf_cmod5n").dsig_co == 0.1


def test_entries_are_declared_and_bound():
    from xsarsea_amd import _lib, windspeed
    txt = open(os.path.join(REPO, "include", "xsw.h")).read()
    for entry, method in (("xsw_cost_from_codes", "cost_from_codes_raw"), ("xsw_cost_cr_from_codes", "cost_cr_from_codes_raw")):
        assert entry in _lib.EXPORTS
        assert callable(getattr(_lib.Context, method))
        assert re.search(rf"\bint\s+{entry}\s*\(\s*xsw_ctx\s*\*", txt)
        assert hasattr(_lib.load(), entry)
    assert re.search(r"#define\s+XSW_VERSION\s+4\b", txt)
    assert windspeed.InversionCost is windspeed.crosspol.InversionCost and "InversionCost" in windspeed.__all__
    c = windspeed.InversionCost(1, 2, 3, 4)
    assert (c["J"], c["Jsig"], c["Jwind"], c["residual_db"]) == (1, 2, 3, 4) and windspeed.InversionCost(1).Jsig is None
