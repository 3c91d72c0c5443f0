"""CPU: the cross-pol step from stored co-pol codes -- its numpy restatement (tests/crosspol_codes_ref.py) against the oracle's
dual-pol output, the argument checks of `CopolCodes.dual` (no library call), and the binding of xsw_cross_from_codes.

The restatement is what the GPU tests of the foreign-code route compare the kernel with, so it is pinned here first: co-pol
codes are built from the oracle's own co-pol answer (grid indices, and the sign of the stored solution), the restatement runs
windspeed.py:252-278 (+ the select :426-428) from them, and the result must be the oracle's dual output bit for bit."""
import os
import re

import numpy as np
import pytest

import crosspol_codes_ref as ref
from conftest import REPO, golden
from test_gpu_kernel import synthetic_scene
from util import bits_equal, oracle_full, small_luts

from oracle import invert as oinv


def _inject(scene):
    """Copies of (inc, s_vv, s_vh, dsig, anc) with one short run of every input class written into otherwise valid pixels."""
    inc, s_vv, s_vh, dsig, anc = (np.array(a, copy=True) for a in scene)
    ok = ~(np.isnan(inc) | np.isnan(s_vv) | np.isnan(s_vh) | np.isnan(dsig) | np.isnan(anc.real) | np.isnan(anc.imag))
    rows = [r for r in range(inc.shape[0]) if ok[r].sum() >= 8][:5]
    assert len(rows) == 5, "the scene has too few fully valid rows to inject into"
    cols = [np.flatnonzero(ok[r])[2:5] for r in rows]
    inc[rows[0], cols[0]] = np.nan     # early NaN by incidence (:198-201)
    anc[rows[1], cols[1]] = np.nan     # early NaN by ancillary wind (:204-207)
    s_vv[rows[2], cols[2]] = np.nan    # no co-pol search: XSW_CODE_NAN, cross-pol only
    s_vh[rows[3], cols[3]] = np.nan    # no cross-pol search: sigma0_cr
    dsig[rows[4], cols[4]] = np.nan    # no cross-pol search: dsig_cr
    return inc, s_vv, s_vh, dsig, anc


def _assert_every_class(code_co, inc, s_cr_db, dsig, code_cr, code_sel):
    """Input coverage, stated on the restatement's own inputs and outputs."""
    early = code_cr == ref.CODE_NAN_RE
    no_index = ~early & ((code_cr & ref.CODE_NO_INDEX) == ref.CODE_NO_INDEX)
    classes = {
        "early NaN by inc": np.isnan(inc) & early,
        "early NaN by ancillary": ~np.isnan(inc) & (code_co == ref.CODE_NAN_RE) & early,
        "co XSW_CODE_NAN (cross-only)": (code_co == ref.CODE_NAN) & ~early & ~no_index,
        "NO_INDEX by NaN sigma0_cr": no_index & np.isnan(s_cr_db) & ~np.isnan(dsig),
        "NO_INDEX by NaN dsig": no_index & ~np.isnan(s_cr_db) & np.isnan(dsig),
        "PICK_CO set": (code_sel != ref.CODE_NAN_RE) & ((code_sel & ref.CODE_PICK_CO) != 0),
        "PICK_CO clear": (code_sel != ref.CODE_NAN_RE) & ((code_sel & ref.CODE_PICK_CO) == 0),
    }
    for name, m in classes.items():
        assert m.any(), f"no pixel of class: {name}"


def _restated(scene, lco, lcr, o):
    inc, _, s_vh, dsig, _ = scene
    tab = ref.tables(lco, lcr)
    code_co = ref.co_codes(o[2], o[0], tab)
    s_cr_db = oinv.to_db(s_vh)
    raw = ref.cross_from_codes(code_co, inc, s_cr_db, dsig, tab)
    sel = ref.cross_from_codes(code_co, inc, s_cr_db, dsig, tab, dual_select=True)
    _assert_every_class(code_co, np.asarray(inc, np.float64), np.asarray(s_cr_db, np.float64), np.asarray(dsig, np.float64), raw[0], sel[0])
    return code_co, raw, sel


@pytest.mark.parametrize("tag", ["phi180_f64", "phi360_f64", "phi180_f32", "phi90_f64"])
def test_restatement_equals_oracle_on_small_goldens(tag):
    """Small-LUT golden scenes (+ the injected classes): wind_dual before and after the select, and the cross-pol index,
    equal the numpy oracle's bit for bit."""
    d = golden(f"kernel_small_{tag}.npz")
    lco, lcr = small_luts(d)
    scene = _inject((d["inc"], d["sigma0_vv"], d["sigma0_vh"], d["dsig_cr"], d["anc"]))
    o = oracle_full(*scene, lco, lcr, fast_c=False)
    _, raw, sel = _restated(scene, lco, lcr, o)
    assert bits_equal(raw[1], o[1]), "wind_dual before the select"
    with np.errstate(all="ignore"):
        want = np.where((np.abs(o[0]) < 5) | (np.abs(o[1]) < 5), o[0], o[1])  # windspeed.py:426-428
    assert bits_equal(sel[1], want), "wind_dual after the select"
    icr = np.where((raw[0] == ref.CODE_NAN_RE) | (raw[0] == ref.CODE_NO_INDEX), -1, raw[0].astype(np.int64))
    assert np.array_equal(icr, o[2][..., 2])


def test_restatement_equals_oracle_on_a_default_lut_scene(default_luts):
    """synthetic_scene(70, 333) on the default LUTs (+ the injected classes), every pixel against the numpy oracle: wind_dual
    before and after the select bit for bit, and the cross-pol index."""
    lco, lcr = default_luts
    scene = _inject(synthetic_scene(70, 333, np.float64, 11))
    o = oracle_full(*scene, lco, lcr, fast_c=False)
    _, raw, sel = _restated(scene, lco, lcr, o)
    assert bits_equal(raw[1], o[1]), "wind_dual before the select"
    with np.errstate(all="ignore"):
        want = np.where((np.abs(o[0]) < 5) | (np.abs(o[1]) < 5), o[0], o[1])  # windspeed.py:426-428
    assert bits_equal(sel[1], want), "wind_dual after the select"
    icr = np.where((raw[0] == ref.CODE_NAN_RE) | (raw[0] == ref.CODE_NO_INDEX), -1, raw[0].astype(np.int64))
    assert np.array_equal(icr, o[2][..., 2]), "cross-pol index differs from the oracle's"


def test_foreign_codes_are_early_nans(lowres_luts, default_luts):
    """A code whose index lies outside the LUT the restatement is given (a code of a larger LUT), or with bit 31 set without
    being one of the two NaN codes, reads no table and gives XSW_CODE_NAN_RE / (nan, 0)."""
    lco, lcr = lowres_luts
    tab = ref.tables(lco, lcr)
    plane = tab["n_wspd"] * tab["n_phi"]
    big = len(default_luts[0].wspd) * len(default_luts[0].phi)
    code = np.array([0, plane - 1, plane, big - 1, 0x40000000 | plane, 0x80000000, 0x80000005, ref.CODE_NAN, ref.CODE_NAN_RE], np.uint32)
    inc = np.full(code.shape, 33.0)
    c, w = ref.cross_from_codes(code, inc, np.full(code.shape, -25.0), np.full(code.shape, 0.1), tab)
    foreign = np.array([False, False, True, True, True, True, True, False, True])
    assert np.array_equal(c == ref.CODE_NAN_RE, foreign)
    assert np.all(np.isnan(w.real[foreign])) and np.all(w.imag[foreign] == 0.0) and not np.any(np.isnan(w.real[~foreign]))


# ------------------------------------------------------------------------------------------------ the public call's checks
class _DeviceArray:
    """Stands for an array in device memory (`__cuda_array_interface__`); nothing ever reads it."""

    def __init__(self, shape, typestr="<f4"):
        self.shape = tuple(shape)
        self.__cuda_array_interface__ = dict(shape=self.shape, typestr=typestr, data=(0, False), version=3)


@pytest.fixture
def no_library(monkeypatch):
    from xsarsea_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def test_dual_refuses_mismatched_arguments(no_library, xr_env):
    from xsarsea_amd import windspeed
    inc = np.full((6, 10), 33.0, np.float32)
    codes = np.zeros((6, 10), np.uint32)
    cc = windspeed.CopolCodes(inc, codes, lut_co=None)
    vh = np.full((6, 10), 1e-3, np.float32)
    with pytest.raises(ValueError, match="shape"):
        cc.dual(vh[:, :9], model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.dual(np.full((2, 6, 10), 1e-3, np.float32), model="gmf_s1_v2")  # would broadcast the codes
    with pytest.raises(ValueError, match="shape"):
        cc.dual(vh, dsig_cr=np.full((6, 3), 0.1, np.float32), model="gmf_s1_v2")
    # mixed containers, either way round
    with pytest.raises(ValueError, match="container"):
        cc.dual(_DeviceArray((6, 10)), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="container"):
        cc.dual(vh, dsig_cr=_DeviceArray((6, 10)), model="gmf_s1_v2")
    dev = windspeed.CopolCodes(_DeviceArray((6, 10)), _DeviceArray((6, 10), "<i4"), lut_co=None)
    assert dev.on_device
    with pytest.raises(ValueError, match="container"):
        dev.dual(vh, model="gmf_s1_v2")
    # xarray / dask containers are not handled by the new calls
    da = xr_env.xr.DataArray(vh, dims=("line", "sample"))
    with pytest.raises(TypeError, match="xarray"):
        cc.dual(da, model="gmf_s1_v2")
    with pytest.raises(TypeError, match="xarray"):
        cc.dual(vh, dsig_cr=da, model="gmf_s1_v2")
    with pytest.raises(TypeError, match="xarray"):
        windspeed.invert_copol_codes(da, da, ancillary_wind=da, model="gmf_cmod5n")
    # cross-pol rasters whose dtype would change how the fused call computes its co-pol step (other co-pol codes)
    with pytest.raises(ValueError, match="dtype"):
        cc.dual(vh.astype(np.float64), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        cc.dual(vh, dsig_cr=np.full((6, 10), 0.1, np.float64), model="gmf_s1_v2")
    with pytest.raises(ValueError, match="dtype"):
        dev.dual(_DeviceArray((6, 10), "<f8"), model="gmf_s1_v2")
    cc64 = windspeed.CopolCodes(inc.astype(np.float64), codes, lut_co=None)
    with pytest.raises(ValueError, match="dtype"):
        cc64.dual(vh, model="gmf_s1_v2")  # a float32 sigma0 next to float64 rasters: another dB route
    # a co-pol model is no cross-pol model
    with pytest.raises(ValueError, match="cross-pol"):
        cc.dual(vh, model="gmf_cmod5n")


def test_entry_is_declared_and_bound():
    from xsarsea_amd import _lib
    assert "xsw_cross_from_codes" in _lib.EXPORTS
    assert callable(getattr(_lib.Context, "cross_from_codes_raw"))
    txt = open(os.path.join(REPO, "include", "xsw.h")).read()
    assert re.search(r"\bint\s+xsw_cross_from_codes\s*\(\s*xsw_ctx\s*\*", txt)
    assert hasattr(_lib.load(), "xsw_cross_from_codes")
