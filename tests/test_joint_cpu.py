"""CPU: the joint dual-pol inversion from stored co-pol codes -- its numpy restatement tests/joint_ref.py,
the exactness claim k_joint_from_codes relies on, the argument checks of `CopolCodes.joint` / `invert_joint` (no library call),
and the binding of xsw_joint_from_codes.

The restatement forms the DENSE joint cost per pixel and takes numpy's arg-min; it is the yardstick of tests/test_gpu_joint.py.
Here it is held to what the kernel's windowed scan assumes: with J_ub the joint cost at the co-pol solution, the dense arg-min
lies among the candidates with Jwind_co <= J_ub on speed rows with Jsig_cr <= J_ub (`joint(..., pruned=True)` asserts it pixel
by pixel), on the three small goldens and on 1500 pixels of the section's recipe on the default tables; and to the classes that
make the GPU comparison meaningful (most joint points differ from the co-pol ones; some lie below the cross-pol speed axis)."""
import os
import re

import numpy as np
import pytest

import crosspol_codes_ref as ref
import joint_ref as jref
from conftest import REPO, golden
from test_crosspol_codes_cpu import _DeviceArray, no_library  # noqa: F401 (fixture)
from util import bits_equal, small_luts

from oracle import invert as oinv
from oracle import lut as olut


def _copol_codes(p, tab, inc, s_co_db, anc):
    """The co-pol oracle solution as grid codes (no cross-pol search)."""
    nan = np.full(np.shape(inc), np.nan)
    wind_co, _, idx = oinv.invert_numpy(p, inc, s_co_db, nan, nan, anc, return_idx=True)
    return ref.co_codes(idx, wind_co, tab)


def _flat(code):
    return code.astype(np.int64) & 0x3FFFFFFF


@pytest.mark.parametrize("tag", ["phi180_f64", "phi360_f64", "phi90_f64"])
def test_argmin_lies_in_the_pruned_set_on_small_goldens(tag):
    """Every pixel of the 24 x 40 scenes; also with a poor a-priori (large windows), and the joint cost never exceeds J_ub."""
    d = golden(f"kernel_small_{tag}.npz")
    lco, lcr = small_luts(d)
    p, tab = oinv.Prepared(lco, lcr), ref.tables(lco, lcr)
    inc, dsig = d["inc"], d["dsig_cr"]
    s_co_db, s_cr_db = oinv.to_db(d["sigma0_vv"]), oinv.to_db(d["sigma0_vh"])
    for scale in (1.0, 0.3, 2.5):
        anc = d["anc"] * scale
        cc = _copol_codes(p, tab, inc, s_co_db, anc)
        r = jref.joint(cc, inc, s_co_db, anc, 0.1, s_cr_db, dsig, p, pruned=True)
        searched = r["n_pruned"] >= 0
        assert searched.sum() > 400, "too few searched pixels"
        assert np.all(r["n_pruned"][searched] >= 1)
        at_co = jref.joint(cc, inc, s_co_db, anc, 0.1, s_cr_db, np.where(np.isnan(dsig), np.nan, np.inf), p)  # Jsig_cr = 0: J_co at the co-pol point
        assert np.all(r["Jwind"][searched] + r["Jsig_co"][searched] >= at_co["J"][searched]), "J_co at the joint point is below the co-pol minimum"
        with np.errstate(all="ignore"):
            assert bits_equal((r["Jwind"] + r["Jsig_co"]) + r["Jsig_cr"], np.where(searched, r["J"], np.nan))


@pytest.fixture(scope="module")
def recipe_run(default_luts):
    lco, lcr = default_luts
    p, tab = oinv.Prepared(lco, lcr), ref.tables(lco, lcr)
    inc, s_co, s_cr, dsig, anc = jref.recipe(np.random.default_rng(19), 1500, p)
    cc = _copol_codes(p, tab, inc, s_co, anc)
    return p, cc, (inc, s_co, s_cr, dsig, anc), jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p, pruned=True)


def test_argmin_lies_in_the_pruned_set_on_the_recipe(recipe_run):
    """1500 pixels on the default tables (501 x 499 x 181, 501 x 771): inside the pruned set on every pixel (asserted by the
    restatement), and the classes the GPU test needs occur often enough."""
    p, cc, _, r = recipe_run
    assert np.all(r["n_pruned"] >= 1), "a recipe pixel was not searched"
    differ = _flat(r["code"]) != _flat(cc)
    below = p.wspd_dim[_flat(r["code"]) // p.phi_dim.size] < p.wspd_cr[0]
    print(f"joint point != co-pol point: {differ.mean():.3f}; on a speed row below wcr[0]: {below.mean():.3f}; "
          f"pruned set median {np.median(r['n_pruned']):.0f}, mean {r['n_pruned'].mean():.0f}, max {r['n_pruned'].max()} of {p.wspd_dim.size * p.phi_dim.size}")
    assert differ.mean() >= 0.5
    assert below.mean() >= 0.01


def test_infinite_dsig_cr_returns_the_copol_codes(recipe_run):
    """Jsig_cr = 0 on every row: the joint arg-min is the co-pol one, its -phi bit included."""
    p, cc, (inc, s_co, s_cr, dsig, anc), _ = recipe_run
    k = slice(0, 200)
    r = jref.joint(cc[k], inc[k], s_co[k], anc[k], 0.1, s_cr[k], np.inf, p)
    assert np.array_equal(r["code"], cc[k]) and np.all(r["Jsig_cr"] == 0.0) and bits_equal(r["J"], r["Jwind"] + r["Jsig_co"])


def constant_tables(slope_cr=0.0):
    """A constant co-pol table on a 0..180 axis and a cross-pol one that is constant (or rises by slope_cr dB per m/s).  With a
    zero a-priori wind Jwind = (w cos / 2)^2 + (w sin / 2)^2 is w^2 / 4 up to an ulp or two, and Jsig_co -- a constant 2500 with
    tie_scene's sigma0 -- absorbs those ulps: J is a function of the speed row alone, bit for bit, and every direction of the
    best row ties."""
    inc = np.array([20.0, 30.0, 40.0])
    w, phi, wcr = 1.0 + 0.5 * np.arange(20), 15.0 * np.arange(13), 3.0 + 1.0 * np.arange(8)
    lco = olut.Lut(np.full((3, 20, 13), -12.0), inc, w, phi, "dB", "x", "co", "VV")
    lcr = olut.Lut(np.broadcast_to(-30.0 + slope_cr * np.arange(8), (3, 8)).copy(), inc, wcr, None, "dB", "x", "cr", "VH")
    return lco, lcr


def tie_scene(n_phi, s_cr_db, dsig_cr):
    """(code_co, inc, sigma0_co_db, sigma0_cr_db, dsig_cr, anc) of four pixels on constant_tables: any grid code does as input."""
    cc = np.array([5 * n_phi + 7, 0 * n_phi + 12, 19 * n_phi + 0, 0], np.uint32)
    return cc, np.full(4, 30.0), np.full(4, -7.0), np.full(4, s_cr_db), np.full(4, dsig_cr), np.zeros(4, np.complex128)


def test_ties_go_to_the_smallest_flat_index():
    lco, lcr = constant_tables()
    p = oinv.Prepared(lco, lcr)
    n_phi = p.phi_dim.size
    cc, inc, s_co, s_cr, dsig, anc = tie_scene(n_phi, -29.0, 0.5)
    r = jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p, pruned=True)
    assert np.all(r["code"] == 0), "Jwind grows with the speed, everything else is constant: row 0, and its first direction"
    assert np.all(r["n_pruned"] >= n_phi)
    # a cross-pol table that rises with the speed and an observation it meets at 8 m/s: the best row lies inside the axis (row 14),
    # and all its directions tie again
    p2 = oinv.Prepared(*constant_tables(slope_cr=2.0))
    cc, inc, s_co, s_cr, dsig, anc = tie_scene(n_phi, -20.0, 0.25)
    r2 = jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p2, pruned=True)
    assert np.all(r2["code"] == 14 * n_phi), r2["code"]
    assert np.all(r2["n_pruned"] >= n_phi)


def test_gates_one_pixel_each(default_luts):
    lco, lcr = default_luts
    p = oinv.Prepared(lco, lcr)
    n_phi, plane = p.phi_dim.size, p.wspd_dim.size * p.phi_dim.size
    good = 100 * n_phi + 40
    code = np.array([ref.CODE_NAN, ref.CODE_NAN_RE, 0x80000005, plane, good, good, good, good, good, good, good], np.uint32)
    n = code.size
    inc, s_co, s_cr, dsig, anc = np.full(n, 33.0), np.full(n, -14.0), np.full(n, -27.0), np.full(n, 0.5), np.full(n, 9 + 3j)
    inc[4] = np.nan      # NaN incidence next to a grid code
    s_cr[5] = np.nan     # no cross-pol information
    dsig[6] = np.nan     # likewise
    s_co[7] = np.nan     # J_ub NaN
    anc[8] = np.nan      # J_ub NaN
    dsig[9] = 0.0        # J_ub inf (or NaN)
    r = jref.joint(code, inc, s_co, anc, 0.1, s_cr, dsig, p)
    assert list(r["code"][:5]) == [ref.CODE_NAN, ref.CODE_NAN_RE, ref.CODE_NAN_RE, ref.CODE_NAN_RE, ref.CODE_NAN_RE]
    assert all(np.isnan(r[k][:5]).all() for k in jref.FIELDS)
    for k in (5, 6):
        assert r["code"][k] == good and np.isnan(r["Jsig_cr"][k]) and r["J"][k] == r["Jwind"][k] + r["Jsig_co"][k] and np.isfinite(r["J"][k])
    for k in (7, 8, 9):
        assert r["code"][k] == ref.CODE_NAN and all(np.isnan(r[f][k]) for f in jref.FIELDS)
    assert r["code"][10] < 0x80000000 and all(np.isfinite(r[f][10]) for f in jref.FIELDS)


# ------------------------------------------------------------------------------------------------ the Python layer
def _engine_is_the_restatement(monkeypatch, lco, lcr):
    """`_engine.joint_from_codes` replaced by the restatement on the oracle's LUTs; returns the list of calls seen."""
    from xsarsea_amd.windspeed import _engine
    seen = []

    def fake(lut_co, lut_cr, plan, codes, inc, s_co, anc, s_cr, dsig_cr, dsig_co=0.1, details=False, out_dtype=np.float64):
        seen.append(dict(plan=plan, dsig_co=dsig_co, details=details, out_dtype=out_dtype))
        d = s_cr * 0 + dsig_cr if np.isscalar(dsig_cr) else dsig_cr
        r = jref.joint(codes, inc, oinv.to_db(s_co), anc, dsig_co, oinv.to_db(s_cr), d, oinv.Prepared(lco, lcr))
        return [r["code"]] + [r[k].astype(out_dtype) if details else None for k in jref.FIELDS]
    monkeypatch.setattr(_engine, "joint_from_codes", fake)
    monkeypatch.setattr(_engine, "lut_source", lambda m, kw: (m.name, dict(kw)))
    return seen


def test_joint_returns_codes_on_the_same_tables(monkeypatch, no_library):  # noqa: F811
    from xsarsea_amd import windspeed
    d = golden("kernel_small_phi180_f64.npz")
    lco, lcr = small_luts(d)
    seen = _engine_is_the_restatement(monkeypatch, lco, lcr)
    p, tab = oinv.Prepared(lco, lcr), ref.tables(lco, lcr)
    inc, vv, vh, dsig, anc = (np.ascontiguousarray(d[k]) for k in ("inc", "sigma0_vv", "sigma0_vh", "dsig_cr", "anc"))
    codes = _copol_codes(p, tab, inc, oinv.to_db(vv), anc)
    cc = windspeed.CopolCodes(inc, codes, lut_co="the co-pol tables", sigma0_meta=(vv.shape, vv.dtype), ancillary_meta=(anc.shape, anc.dtype), dsig_co=0.1)
    want = jref.joint(codes, inc, oinv.to_db(vv), anc, 0.1, oinv.to_db(vh), dsig, p)
    out = cc.joint(vv, anc, vh, dsig_cr=dsig, model="gmf_s1_v2")
    assert isinstance(out, windspeed.CopolCodes) and out.lut_co == "the co-pol tables" and out.inc is inc and out.dsig_co == 0.1
    assert out.sigma0_meta == cc.sigma0_meta and out.ancillary_meta == cc.ancillary_meta and out.shape == cc.shape
    assert np.array_equal(out.codes, want["code"]) and np.any(out.codes != codes)
    assert seen[-1]["details"] is False and seen[-1]["plan"].shape == inc.shape and seen[-1]["plan"].dtype == np.float64
    det = cc.joint(vv, anc, vh, dsig_cr=dsig, model="gmf_s1_v2", details=True, out_dtype=np.float32)
    assert isinstance(det, windspeed.JointInversion) and isinstance(det.codes, windspeed.CopolCodes) and det["J"] is det.J
    assert np.array_equal(det.codes.codes, want["code"])
    for k in jref.FIELDS:
        assert det[k].dtype == np.float32 and bits_equal(det[k], want[k].astype(np.float32))
    # dsig_co: the stored one, else 0.1, an explicit one wins; a scalar dsig_cr is handed on as it is
    cc.joint(vv, anc, vh, model="gmf_s1_v2", dsig_co=0.5)
    windspeed.CopolCodes(inc, codes, lut_co=None, dsig_co=0.25).joint(vv, anc, vh, model="gmf_s1_v2")
    assert [s["dsig_co"] for s in seen[-2:]] == [0.5, 0.25]


def test_joint_refuses_mismatched_arguments(no_library, xr_env):  # noqa: F811
    """The refusals of `.cost` (the co-pol rasters) and of `.dual` (the cross-pol ones), before any device call."""
    from xsarsea_amd import windspeed
    shape = (6, 10)
    cc = windspeed.CopolCodes(np.full(shape, 33.0, np.float32), np.zeros(shape, np.uint32), lut_co=None, sigma0_meta=(shape, np.dtype(np.float32)),
                              ancillary_meta=(shape, np.dtype(np.complex64)))
    vv, vh, anc = np.full(shape, 1e-2, np.float32), np.full(shape, 1e-3, np.float32), np.full(shape, 5 + 1j, np.complex64)
    kw = dict(model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.joint(vv[:, :9], anc, vh, **kw)
    with pytest.raises(ValueError, match="shape"):
        cc.joint(vv, anc, vh[:, :9], **kw)
    with pytest.raises(ValueError, match="shape"):
        cc.joint(vv, anc, vh, dsig_cr=np.full((6, 3), 0.1, np.float32), **kw)
    with pytest.raises(ValueError, match="dtype"):
        cc.joint(vv.astype(np.float64), anc, vh, **kw)
    with pytest.raises(ValueError, match="dtype"):
        cc.joint(vv, anc, vh.astype(np.float64), **kw)
    with pytest.raises(ValueError, match="needed"):
        cc.joint(vv, None, vh, **kw)
    with pytest.raises(ValueError, match="missing"):
        cc.joint(vv, anc, None, **kw)
    with pytest.raises(ValueError, match="container"):
        cc.joint(_DeviceArray(shape), anc, vh, **kw)
    with pytest.raises(ValueError, match="container"):
        cc.joint(vv, anc, _DeviceArray(shape), **kw)
    with pytest.raises(TypeError, match="xarray"):
        cc.joint(vv, anc, xr_env.xr.DataArray(vh, dims=("line", "sample")), **kw)
    with pytest.raises(ValueError, match="dsig_co"):
        cc.joint(vv, anc, vh, dsig_co=0.0, **kw)
    with pytest.raises(ValueError, match="cross-pol"):
        cc.joint(vv, anc, vh, model="gmf_cmod5n")
    with pytest.raises(ValueError, match="out_dtype"):
        cc.joint(vv, anc, vh, out_dtype=np.int32, resolution="low", **kw)
    with pytest.raises(ValueError, match="model"):
        windspeed.invert_joint(cc.inc, vv, vh, ancillary_wind=anc, model="gmf_cmod5n")


def test_invert_joint_is_the_two_calls(monkeypatch):
    from xsarsea_amd import windspeed
    from xsarsea_amd.windspeed import _engine
    d = golden("kernel_small_phi180_f64.npz")
    lco, lcr = small_luts(d)
    seen = _engine_is_the_restatement(monkeypatch, lco, lcr)
    p, tab = oinv.Prepared(lco, lcr), ref.tables(lco, lcr)
    inc, vv, vh, dsig, anc = (np.ascontiguousarray(d[k]) for k in ("inc", "sigma0_vv", "sigma0_vh", "dsig_cr", "anc"))
    codes = _copol_codes(p, tab, inc, oinv.to_db(vv), anc)
    monkeypatch.setattr(_engine, "invert_numpy", lambda lco_, lcr_, inc_, *a, **k: (codes, None))
    monkeypatch.setattr(_engine, "expand_codes", lambda lco_, lcr_, cco, ccr: (("wind of", cco), None))
    want = jref.joint(codes, inc, oinv.to_db(vv), anc, 0.2, oinv.to_db(vh), dsig, p)["code"]
    kw = dict(ancillary_wind=anc, dsig_co=0.2, dsig_cr=dsig, model=("gmf_cmod5n", "gmf_s1_v2"))
    tag, got = windspeed.invert_joint(inc, vv, vh, **kw)
    assert tag == "wind of" and np.array_equal(got, want) and seen[-1]["dsig_co"] == 0.2
    (tag, got), det = windspeed.invert_joint(inc, vv, vh, details=True, **kw)
    assert tag == "wind of" and np.array_equal(got, want) and isinstance(det, windspeed.JointInversion) and det.J.shape == inc.shape


def test_entry_is_declared_and_bound():
    from xsarsea_amd import _lib, windspeed
    txt = open(os.path.join(REPO, "include", "xsw.h")).read()
    assert "xsw_joint_from_codes" in _lib.EXPORTS and callable(getattr(_lib.Context, "joint_from_codes_raw"))
    assert re.search(r"\bint\s+xsw_joint_from_codes\s*\(\s*xsw_ctx\s*\*", txt) and hasattr(_lib.load(), "xsw_joint_from_codes")
    assert re.search(r"#define\s+XSW_VERSION\s+4\b", txt)
    for name in ("invert_joint", "JointInversion"):
        assert name in windspeed.__all__ and getattr(windspeed, name) is getattr(windspeed.crosspol, name)
    assert callable(windspeed._engine.joint_from_codes) and callable(windspeed.CopolCodes.joint)
