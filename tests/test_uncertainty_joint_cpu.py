"""CPU: the error bars of the joint dual-pol solution -- the numpy restatement
tests/uncertainty_joint_ref.py, the yardstick of tests/test_gpu_uncertainty_joint.py, held to the dense joint cost of
tests/joint_ref.py; the classes that make the GPU comparison meaningful; the (u, v) change of variables; a closed form along the
speed axis; the argument checks of `CopolCodes.uncertainty_joint` (no library call) and the binding of
xsw_uncertainty_joint_from_codes.

Measured on the recipe below (default tables, the first 600 pixels of joint_ref.recipe(default_rng(19), 1500), dsig_co 0.1, joint
codes from the restatement): an estimate on 0.982 of the pixels (0.962 for the co-pol stencil at the same codes); where both give
one, the median wspd_std is 0.49 m/s against 1.05 m/s, the joint one is the smaller on 0.977 of the pixels (below 0.9 of it on
0.894), the median dir_std 3.0 deg against 3.9 deg."""
import os
import re

import numpy as np
import pytest

import crosspol_codes_ref as ref
import joint_ref as jref
import uncertainty_joint_ref as ujref
import uncertainty_ref as uref
from conftest import REPO, golden
from test_crosspol_codes_cpu import _DeviceArray, no_library  # noqa: F401 (fixture)
from test_joint_cpu import _copol_codes, constant_tables
from util import bits_equal, small_luts

from oracle import invert as oinv
from oracle import lut as olut
from xsarsea_amd import _lib
from xsarsea_amd.windspeed import JointUncertainty

EPS = np.finfo(np.float64).eps
GOLDENS = ["phi180_f64", "phi360_f64", "phi90_f64"]


def _dense_J(p, inc, s_co_db, anc, dsig_co, s_cr_db, dsig_cr):
    """The dense joint cost of ONE pixel, in joint_ref.joint's statements."""
    lut_inc = p.co_lut[:, :, np.argmin(np.abs(p.inc_dim - inc))]
    m_antenna, m_azi = np.real(anc), np.imag(anc)
    if p.phi_180:
        m_azi = np.abs(m_azi)
    Jwind_co = ((p.lut_co_antenna - m_antenna) / p.d_antenna) ** 2 + ((p.lut_co_azi - m_azi) / p.d_azi) ** 2
    Jsig_co = ((lut_inc - s_co_db) / dsig_co) ** 2
    rows = jref.jsig_cr_rows(p, np.argmin(np.abs(p.inc_cr_dim - inc)), s_cr_db, dsig_cr)
    return (Jwind_co + Jsig_co) + rows[:, None]


def _assert_stencil_is_the_dense_block(p, code, inc, s_co, anc, s_cr, dsig, joint):
    """On every pixel whose stencil ran with the cross-pol term: the nine J are the 3 x 3 block of the dense J around its arg-min,
    the centre is joint's J and the smallest of the nine.  Returns the number of such pixels."""
    flag, iw, ip, J = ujref.stencil_joint(code, inc, s_co, anc, 0.1, s_cr, dsig, p)
    n_phi = p.phi_dim.size
    ran = np.flatnonzero(flag == 0)
    f = lambda a: np.asarray(a).ravel()
    with np.errstate(all="ignore"):
        for i in ran:
            D = _dense_J(p, f(inc)[i], f(s_co)[i], f(anc)[i], 0.1, f(s_cr)[i], f(dsig)[i])
            assert int(np.argmin(D)) == iw[i] * n_phi + ip[i] == int(f(code)[i]) & 0x3FFFFFFF, f"pixel {i}: the code is not the dense arg-min"
            assert bits_equal(J[i], D[iw[i] - 1:iw[i] + 2, ip[i] - 1:ip[i] + 2]), f"pixel {i}: the stencil is not the dense block"
    assert bits_equal(J[ran, 1, 1], f(joint["J"])[ran]), "the centre is not the joint cost"
    assert np.all(J[ran, 1, 1][:, None, None] <= J[ran]), "the centre of a joint code's stencil is not its smallest"
    return ran.size


def _golden_scene(tag, scale=1.0):
    d = golden(f"kernel_small_{tag}.npz")
    lco, lcr = small_luts(d)
    p, tab = oinv.Prepared(lco, lcr), ref.tables(lco, lcr)
    inc, dsig, anc = d["inc"], d["dsig_cr"], d["anc"] * scale
    s_co, s_cr = oinv.to_db(d["sigma0_vv"]), oinv.to_db(d["sigma0_vh"])
    cc = _copol_codes(p, tab, inc, s_co, anc)
    return p, cc, (inc, s_co, s_cr, dsig, anc), jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p)


@pytest.fixture(scope="module")
def golden_scenes():
    return {tag: _golden_scene(tag) for tag in GOLDENS}


def _near_apriori_codes(p, anc):
    """Some grid code per pixel (the grid point next to the a-priori wind): the joint answer does not depend on its input code."""
    ang = np.degrees(np.angle(anc))
    ang = np.abs(ang) if p.phi_180 else np.mod(ang, 360.0)
    iw = np.argmin(np.abs(p.wspd_dim[None, :] - np.abs(anc)[:, None]), axis=1)
    ip = np.argmin(np.abs(p.phi_dim[None, :] - ang[:, None]), axis=1)
    return (iw * p.phi_dim.size + ip).astype(np.uint32)


@pytest.fixture(scope="module")
def recipe_run(default_luts):
    """The first 600 pixels of the 1500 of tests/test_joint_cpu.py's recipe, their joint codes and the joint error bars."""
    p = oinv.Prepared(*default_luts)
    inc, s_co, s_cr, dsig, anc = (a[:600] for a in jref.recipe(np.random.default_rng(19), 1500, p))
    joint = jref.joint(_near_apriori_codes(p, anc), inc, s_co, anc, 0.1, s_cr, dsig, p)
    assert np.all(joint["code"] < 0x80000000)
    return p, (inc, s_co, s_cr, dsig, anc), joint, ujref.unc_joint(joint["code"], inc, s_co, anc, 0.1, s_cr, dsig, p, terms=True)


# ------------------------------------------------------------------------------------------------ the stencil
@pytest.mark.parametrize("tag", GOLDENS)
def test_stencil_is_the_dense_block_on_small_goldens(golden_scenes, tag):
    p, _, (inc, s_co, s_cr, dsig, anc), joint = golden_scenes[tag]
    n = _assert_stencil_is_the_dense_block(p, joint["code"], inc, s_co, anc, s_cr, dsig, joint)
    print(f"{tag}: {n} of {inc.size} pixels have a joint stencil")
    assert n > 300


def test_stencil_is_the_dense_block_on_the_recipe(recipe_run):
    p, (inc, s_co, s_cr, dsig, anc), joint, _ = recipe_run
    n = _assert_stencil_is_the_dense_block(p, joint["code"], inc, s_co, anc, s_cr, dsig, joint)
    assert n >= 0.9 * inc.size


def test_recipe_has_the_classes_the_gpu_comparison_needs(recipe_run):
    """An estimate on most pixels, and error bars that differ from the co-pol ones where both exist: otherwise a kernel that forgot
    the cross-pol term would pass."""
    p, (inc, s_co, s_cr, dsig, anc), joint, u = recipe_run
    co = uref.unc_co(joint["code"], inc, s_co, anc, 0.1, p)
    est, est_co = u["flag"] == 0, co["flag"] == 0
    both = est & est_co
    ratio = u["wspd_std"][both] / co["wspd_std"][both]
    print(f"estimate: joint {est.mean():.3f}, co-pol stencil at the same codes {est_co.mean():.3f}; flags {dict(zip(*np.unique(u['flag'], return_counts=True)))}; "
          f"median wspd_std {np.median(u['wspd_std'][both]):.2f} against {np.median(co['wspd_std'][both]):.2f} m/s, median ratio {np.median(ratio):.2f}, "
          f"smaller on {np.mean(ratio < 1.0):.3f}, below 0.9 on {np.mean(ratio < 0.9):.3f}; median dir_std {np.median(u['dir_std'][both]):.1f} against "
          f"{np.median(co['dir_std'][both]):.1f} deg")
    assert est.mean() >= 0.75
    assert np.mean(ratio < 1.0) >= 0.5
    assert all(np.array_equal(np.isnan(u[k]), ~est) for k in ujref.FIELDS)


def test_every_flag_occurs_on_the_small_goldens(golden_scenes):
    """Each of the five bits, and an estimate with and without bit 16, on the joint codes of the three scenes."""
    seen = set()
    for tag in GOLDENS:
        p, _, (inc, s_co, s_cr, dsig, anc), joint = golden_scenes[tag]
        u = ujref.unc_joint(joint["code"], inc, s_co, anc, 0.1, s_cr, dsig, p)
        seen |= set(u["flag"].ravel().tolist())
        assert all(np.array_equal(np.isnan(u[k]), (u["flag"] & 15) != 0) for k in ujref.FIELDS)
    print(f"flag values on the small goldens: {sorted(seen)}")
    assert {0, ujref.NO_CROSSPOL} <= seen
    for bit in (ujref.NO_SOLUTION, ujref.WSPD_BORDER, ujref.PHI_BORDER, ujref.NOT_CONVEX, ujref.NO_CROSSPOL):
        assert any(v & bit for v in seen), f"bit {bit} never set"
    assert ujref.NO_CROSSPOL == _lib.UNC_NO_CROSSPOL == JointUncertainty.FLAGS["no_crosspol"]


# ------------------------------------------------------------------------------------------------ no cross-pol term
def _assert_is_unc_co(u, co, bit16):
    for k in uref.FIELDS_CO:
        assert bits_equal(u[k], co[k]), k
    assert np.array_equal(u["flag"], co["flag"] | (ujref.NO_CROSSPOL if bit16 else 0))


@pytest.mark.parametrize("which", ["phi180_f64", "recipe"])
def test_without_crosspol_information_it_is_unc_co(golden_scenes, recipe_run, which):
    """dsig_cr = inf: Jsig_cr = 0 exactly, unc_co bit for bit, bit 16 clear; NaN sigma0_cr or dsig_cr: the same with bit 16 set."""
    if which == "recipe":
        p, (inc, s_co, s_cr, dsig, anc), joint, _ = recipe_run
        k = slice(0, 200)
        inc, s_co, s_cr, dsig, anc, code = inc[k], s_co[k], s_cr[k], dsig[k], anc[k], joint["code"][k]
    else:
        p, code, (inc, s_co, s_cr, dsig, anc), _ = golden_scenes[which]
        s_cr, dsig = np.where(np.isnan(s_cr), -25.0, s_cr), np.where(np.isnan(dsig), 0.3, dsig)
    co = uref.unc_co(code, inc, s_co, anc, 0.1, p)
    assert np.sum(co["flag"] == 0) > 100
    nan, inf = np.full(np.shape(inc), np.nan), np.full(np.shape(inc), np.inf)
    _assert_is_unc_co(ujref.unc_joint(code, inc, s_co, anc, 0.1, s_cr, inf, p), co, False)
    _assert_is_unc_co(ujref.unc_joint(code, inc, s_co, anc, 0.1, nan, dsig, p), co, True)
    _assert_is_unc_co(ujref.unc_joint(code, inc, s_co, anc, 0.1, s_cr, nan, p), co, True)
    with_cr = ujref.unc_joint(code, inc, s_co, anc, 0.1, s_cr, dsig, p)
    assert not bits_equal(with_cr["wspd_std"], co["wspd_std"]) and not np.any(with_cr["flag"] & ujref.NO_CROSSPOL)


def test_a_stencil_that_is_not_finite_is_not_convex(recipe_run):
    p, (inc, s_co, s_cr, dsig, anc), joint, u = recipe_run
    k = np.flatnonzero(u["flag"] == 0)[:6]
    inc, s_co, s_cr, dsig, anc, code = (a[k].copy() for a in (inc, s_co, s_cr, dsig, anc, joint["code"]))
    dsig[0], s_cr[1], s_cr[2], s_co[3], anc[4] = 0.0, np.inf, -np.inf, np.nan, np.nan
    got = ujref.unc_joint(code, inc, s_co, anc, 0.1, s_cr, dsig, p)
    assert list(got["flag"]) == [ujref.NOT_CONVEX] * 5 + [0] and np.isnan(got["u_std"][:5]).all() and np.isfinite(got["u_std"][5])


# ------------------------------------------------------------------------------------------------ (u, v)
def _good_terms(u):
    ok = u["flag"].ravel() & 15 == 0
    return ok, {k: v.ravel()[ok] for k, v in u["terms"].items()}


def test_trace_of_the_uv_covariance(recipe_run):
    """var_u + var_v == Sww + (w r)^2 Spp: the rotation keeps the trace.  Each side is a sum of products with a handful of roundings
    per term, so the two differ by at most a few dozen eps times the absolute sum of the terms."""
    _, _, _, u = recipe_run
    ok, t = _good_terms(u)
    assert ok.sum() > 400
    wr = t["w"] * ujref.DEG
    lhs, rhs = t["var_u"] + t["var_v"], t["Sww"] + (wr * wr) * t["Spp"]
    mag = sum(np.abs(x) for x in ((t["c"] * t["c"]) * t["Sww"], 2.0 * (t["c"] * t["tu"]) * t["Swp"], (t["tu"] * t["tu"]) * t["Spp"],
                                  (t["s"] * t["s"]) * t["Sww"], 2.0 * (t["s"] * t["tv"]) * t["Swp"], (t["tv"] * t["tv"]) * t["Spp"],
                                  t["Sww"], (wr * wr) * t["Spp"]))
    err = np.abs(lhs - rhs) / (EPS * mag)
    print(f"trace identity: largest |lhs - rhs| is {err.max():.2f} eps of the absolute sum of the terms")
    assert np.all(err <= 32.0)


def test_uv_covariance_is_the_jacobian_transform(recipe_run):
    """Against A S A^T written out from the wind itself, u + i v = w exp(+-i phi) with the table's phi and the covariance S of
    (w, phi): for bit 30 the derivatives are those of exp(-i phi).  The same bound as the trace."""
    p, (inc, s_co, s_cr, dsig, anc), joint, _ = recipe_run
    for flip in (0, 1):
        code = joint["code"] ^ np.uint32(flip << 30) if flip else joint["code"]
        u = ujref.unc_joint(code, inc, s_co, anc, 0.1, s_cr, dsig, p, terms=True)
        ok = u["flag"] & 15 == 0
        flat = code.astype(np.int64)[ok] & 0x3FFFFFFF
        w, phi = p.wspd_dim[flat // p.phi_dim.size], np.radians(p.phi_dim[flat % p.phi_dim.size])
        sign = np.where((code[ok] >> 30) & 1, -1.0, 1.0)
        Sww, Spp = u["wspd_std"][ok] ** 2, u["dir_std"][ok] ** 2
        Swp = u["corr"][ok] * u["wspd_std"][ok] * u["dir_std"][ok]  # of (w, the table's phi)
        A = np.array([[np.cos(phi), -w * np.sin(phi) * ujref.DEG], [sign * np.sin(phi), sign * w * np.cos(phi) * ujref.DEG]])
        S = np.array([[Sww, Swp], [Swp, Spp]])
        C = np.einsum("ikn,kln,jln->ijn", A, S, A)
        mag = np.einsum("ikn,kln,jln->ijn", np.abs(A), np.abs(S), np.abs(A))
        su, sv = u["u_std"][ok], u["v_std"][ok]
        for got, want, m in ((su * su, C[0, 0], mag[0, 0]), (sv * sv, C[1, 1], mag[1, 1]), (u["corr_uv"][ok] * su * sv, C[0, 1], mag[0, 1])):
            assert np.all(np.abs(got - want) <= 64.0 * EPS * m), f"bit 30 = {flip}"


def test_bit_30_flips_the_sign_of_corr_uv_alone(recipe_run, golden_scenes):
    p, (inc, s_co, s_cr, dsig, anc), joint, u = recipe_run
    scenes = [(p, joint["code"], inc, s_co, anc, s_cr, dsig, u)]
    for tag in ("phi180_f64", "phi360_f64"):
        gp, _, (g_inc, g_co, g_cr, g_dsig, g_anc), g_joint = golden_scenes[tag]
        scenes.append((gp, g_joint["code"], g_inc, g_co, g_anc, g_cr, g_dsig, ujref.unc_joint(g_joint["code"], g_inc, g_co, g_anc, 0.1, g_cr, g_dsig, gp)))
    for q, code, inc, s_co, anc, s_cr, dsig, a in scenes:
        grid = code < 0x80000000
        b = ujref.unc_joint(np.where(grid, code ^ np.uint32(1 << 30), code), inc, s_co, anc, 0.1, s_cr, dsig, q)
        for k in ("wspd_std", "dir_std", "corr", "u_std", "v_std", "flag"):
            assert bits_equal(a[k], b[k]), k
        assert bits_equal(a["corr_uv"], -b["corr_uv"]) and np.sum(np.abs(a["corr_uv"]) > 0) > 100


def _smooth_luts(w, phi, wcr):
    inc_ax = np.array([20.0, 30.0, 45.0])
    co = -22.0 + 9.0 * np.log10(1.0 + w)[None, :, None] + 2.0 * np.cos(np.deg2rad(2.0 * phi))[None, None, :] - 0.15 * (inc_ax - 20.0)[:, None, None]
    cr = -36.0 + 12.0 * np.log10(1.0 + wcr)[None, :] - 0.05 * (inc_ax - 20.0)[:, None]
    return olut.Lut(co, inc_ax, w, phi, "dB", "x", "co", "VV"), olut.Lut(cr, inc_ax, wcr, None, "dB", "x", "cr", "VH")


def test_at_sin_zero_u_std_is_wspd_std():
    """A direction axis with 0 deg in its interior: there s = 0 exactly, c = 1, u is the speed itself."""
    w, phi, wcr = 1.0 + 0.5 * np.arange(12), np.array([-40.0, -20.0, 0.0, 20.0, 40.0]), 0.5 + 1.0 * np.arange(9)
    lco, lcr = _smooth_luts(w, phi, wcr)
    p = oinv.Prepared(lco, lcr)
    assert not p.phi_180 and ujref.trig(p)[1][2] == 0.0
    iw = np.arange(1, 11)
    code = (iw * 5 + 2).astype(np.uint32)
    inc = np.full(iw.size, 31.0)
    s_co, s_cr = lco.values[1, iw, 2] + 0.02, np.interp(w[iw], wcr, lcr.values[1]) - 0.1
    anc = (w[iw] * 1.05).astype(np.complex128)
    for c in (code, code | np.uint32(1 << 30)):
        u = ujref.unc_joint(c, inc, s_co, anc, 0.1, s_cr, np.full(iw.size, 0.5), p)
        assert np.sum(u["flag"] == 0) >= 5, u["flag"]
        assert bits_equal(u["u_std"], u["wspd_std"])


# ------------------------------------------------------------------------------------------------ a closed form along the speed
def test_closed_form_in_speed():
    """A co-pol table constant in both axes and a cross-pol table linear in the speed with slope c1: along the speed J is a
    parabola, Jwind = ((w c - a) / 2)^2 + ((w s - b) / 2)^2 with curvature (c^2 + s^2) / 2 and Jsig_cr with 2 c1^2 / dsig_cr^2, so
    Jww = 2 c1^2 / dsig_cr^2 + 1/2 at any step.  Axis values, table entries, sigma0 and dsig_cr are binary fractions, so the lerp,
    Jsig_cr and Jsig_co are exact and a J carries the roundings of Jwind (two products with a rounded cos / sin, two differences,
    two squares, a sum) and of the two additions: at most 12 eps max|J|.  The second difference adds four such errors over h^2
    and rounds five times more; c^2 + s^2 is 1 to within 2 eps: |d Jww| <= 4 * 12 eps max|J| / h^2 + 8 eps Jww.  On the rows below
    wcr[0] the cross-pol table is held constant and adds no curvature: Jww = 1/2."""
    c1, dsig_cr, h = 2.0, 0.25, 0.5
    lco, lcr = constant_tables(slope_cr=c1)  # w = 1, 1.5 .. 10.5; wcr = 3, 4 .. 10; cr = -30 + 2 (wcr - 3)
    p = oinv.Prepared(lco, lcr)
    n_w, n_phi = p.wspd_dim.size, p.phi_dim.size
    iw, ip = np.meshgrid(np.arange(n_w), np.arange(1, n_phi - 1), indexing="ij")
    code = (iw * n_phi + ip).astype(np.uint32)
    shape = code.shape
    inc, s_co, s_cr, anc = np.full(shape, 30.0), np.full(shape, -12.5), np.full(shape, -20.0), np.full(shape, 5.0 + 2.0j)
    u = ujref.unc_joint(code, inc, s_co, anc, 0.1, s_cr, np.full(shape, dsig_cr), p, terms=True)
    assert np.all(u["flag"][[0, -1]] == ujref.WSPD_BORDER) and not np.any(u["flag"][1:-1] & 7)
    maxJ = np.nanmax(u["J"])
    inside = (p.wspd_dim - h >= p.wspd_cr[0]) & (p.wspd_dim + h <= p.wspd_cr[-1])
    below = p.wspd_dim + h <= p.wspd_cr[0]
    below[0] = False
    assert inside.sum() == 13 and below.sum() == 3
    for rows, want in ((inside, 2.0 * c1 ** 2 / dsig_cr ** 2 + 0.5), (below, 0.5)):
        tol = 4 * 12 * EPS * maxJ / h ** 2 + 8 * EPS * want
        err = np.max(np.abs(u["Jww"][rows] - want))
        print(f"closed form: Jww {want} with largest error {err:.3e}, bound {tol:.3e} (max J {maxJ:.3e})")
        assert err <= tol
    co = uref.unc_co(code, inc, s_co, anc, 0.1, p)
    good = (u["flag"] == 0) & (co["flag"] == 0) & inside[:, None]
    assert good.sum() > 10 and np.all(u["wspd_std"][good] < 0.2 * co["wspd_std"][good])


# ------------------------------------------------------------------------------------------------ the Python layer
def _engine_is_the_restatement(monkeypatch, lco, lcr):
    """`_engine.uncertainty_joint_from_codes` replaced by the restatement on the oracle's LUTs; returns the list of calls seen."""
    from xsarsea_amd.windspeed import _engine
    seen = []

    def fake(lut_co, lut_cr, plan, codes, inc, s_co, anc, s_cr, dsig_cr, dsig_co=0.1, out_dtype=np.float64):
        seen.append(dict(plan=plan, dsig_co=dsig_co, out_dtype=out_dtype, lut_co=lut_co, lut_cr=lut_cr))
        d = s_cr * 0 + dsig_cr if np.isscalar(dsig_cr) else dsig_cr
        r = ujref.unc_joint(codes, inc, oinv.to_db(s_co), anc, dsig_co, oinv.to_db(s_cr), d, oinv.Prepared(lco, lcr))
        return [r[k].astype(out_dtype) for k in ujref.FIELDS] + [r["flag"]]
    monkeypatch.setattr(_engine, "uncertainty_joint_from_codes", fake)
    monkeypatch.setattr(_engine, "lut_source", lambda m, kw: (m.name, dict(kw)))
    return seen


def test_uncertainty_joint_returns_the_seven_rasters(monkeypatch, no_library):  # noqa: F811
    from xsarsea_amd import windspeed
    d = golden("kernel_small_phi180_f64.npz")
    lco, lcr = small_luts(d)
    seen = _engine_is_the_restatement(monkeypatch, lco, lcr)
    p, tab = oinv.Prepared(lco, lcr), ref.tables(lco, lcr)
    inc, vv, vh, dsig, anc = (np.ascontiguousarray(d[k]) for k in ("inc", "sigma0_vv", "sigma0_vh", "dsig_cr", "anc"))
    codes = jref.joint(_copol_codes(p, tab, inc, oinv.to_db(vv), anc), inc, oinv.to_db(vv), anc, 0.1, oinv.to_db(vh), dsig, p)["code"]
    cc = windspeed.CopolCodes(inc, codes, lut_co="the co-pol tables", sigma0_meta=(vv.shape, vv.dtype), ancillary_meta=(anc.shape, anc.dtype), dsig_co=0.1)
    want = ujref.unc_joint(codes, inc, oinv.to_db(vv), anc, 0.1, oinv.to_db(vh), dsig, p)
    out = cc.uncertainty_joint(vv, anc, vh, dsig_cr=dsig, model="gmf_s1_v2", resolution="low")
    assert isinstance(out, windspeed.JointUncertainty) and out["u_std"] is out.u_std and not isinstance(out, windspeed.InversionUncertainty)
    for k in ujref.FIELDS:
        assert out[k].dtype == np.float64 and bits_equal(out[k], want[k])
    assert out.flag.dtype == np.uint8 and np.array_equal(out.flag, want["flag"]) and np.any(out.flag == 0)
    s = seen[-1]
    assert s["plan"].shape == inc.shape and s["plan"].dtype == np.float64 and s["out_dtype"] == np.float64
    assert s["lut_co"] == "the co-pol tables" and s["lut_cr"] == ("gmf_s1_v2", dict(resolution="low"))
    out32 = cc.uncertainty_joint(vv, anc, vh, dsig_cr=dsig, model="gmf_s1_v2", out_dtype=np.float32)
    for k in ujref.FIELDS:
        assert out32[k].dtype == np.float32 and bits_equal(out32[k], want[k].astype(np.float32))
    # dsig_co: the stored one, else 0.1, an explicit one wins; a scalar dsig_cr is handed on as it is
    cc.uncertainty_joint(vv, anc, vh, model="gmf_s1_v2", dsig_co=0.5)
    windspeed.CopolCodes(inc, codes, lut_co=None, dsig_co=0.25).uncertainty_joint(vv, anc, vh, model="gmf_s1_v2")
    windspeed.CopolCodes(inc, codes, lut_co=None).uncertainty_joint(vv, anc, vh, model="gmf_s1_v2")
    assert [s["dsig_co"] for s in seen[-3:]] == [0.5, 0.25, 0.1]


def test_uncertainty_joint_refuses_mismatched_arguments(no_library, xr_env):  # noqa: F811
    """The refusals of `.joint` (`_co_step` for the co-pol rasters, `_cross_step` for the cross-pol ones), before any device call."""
    from xsarsea_amd import windspeed
    shape = (6, 10)
    cc = windspeed.CopolCodes(np.full(shape, 33.0, np.float32), np.zeros(shape, np.uint32), lut_co=None, sigma0_meta=(shape, np.dtype(np.float32)),
                              ancillary_meta=(shape, np.dtype(np.complex64)))
    vv, vh, anc = np.full(shape, 1e-2, np.float32), np.full(shape, 1e-3, np.float32), np.full(shape, 5 + 1j, np.complex64)
    kw = dict(model="gmf_s1_v2")
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty_joint(vv[:, :9], anc, vh, **kw)
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty_joint(vv, anc, vh[:, :9], **kw)
    with pytest.raises(ValueError, match="shape"):
        cc.uncertainty_joint(vv, anc, vh, dsig_cr=np.full((6, 3), 0.1, np.float32), **kw)
    with pytest.raises(ValueError, match="dtype"):
        cc.uncertainty_joint(vv.astype(np.float64), anc, vh, **kw)
    with pytest.raises(ValueError, match="dtype"):
        cc.uncertainty_joint(vv, anc, vh.astype(np.float64), **kw)
    with pytest.raises(ValueError, match="needed"):
        cc.uncertainty_joint(vv, None, vh, **kw)
    with pytest.raises(ValueError, match="missing"):
        cc.uncertainty_joint(vv, anc, None, **kw)
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty_joint(_DeviceArray(shape), anc, vh, **kw)
    with pytest.raises(ValueError, match="container"):
        cc.uncertainty_joint(vv, anc, _DeviceArray(shape), **kw)
    with pytest.raises(TypeError, match="xarray"):
        cc.uncertainty_joint(vv, anc, xr_env.xr.DataArray(vh, dims=("line", "sample")), **kw)
    with pytest.raises(ValueError, match="dsig_co"):
        cc.uncertainty_joint(vv, anc, vh, dsig_co=0.0, **kw)
    with pytest.raises(ValueError, match="dsig_co"):
        cc.uncertainty_joint(vv, anc, vh, dsig_co=float("nan"), **kw)
    with pytest.raises(ValueError, match="cross-pol"):
        cc.uncertainty_joint(vv, anc, vh, model="gmf_cmod5n")
    with pytest.raises(ValueError, match="out_dtype"):
        cc.uncertainty_joint(vv, anc, vh, out_dtype=np.int32, resolution="low", **kw)


def test_entry_is_declared_and_bound():
    from xsarsea_amd import windspeed
    txt = open(os.path.join(REPO, "include", "xsw.h")).read()
    assert "xsw_uncertainty_joint_from_codes" in _lib.EXPORTS and callable(getattr(_lib.Context, "uncertainty_joint_from_codes_raw"))
    assert re.search(r"\bint\s+xsw_uncertainty_joint_from_codes\s*\(\s*xsw_ctx\s*\*", txt) and hasattr(_lib.load(), "xsw_uncertainty_joint_from_codes")
    assert re.search(r"#define\s+XSW_VERSION\s+4\b", txt) and re.search(r"#define\s+XSW_UNC_NO_CROSSPOL\s+16u?\b", txt)
    assert "JointUncertainty" in windspeed.__all__ and windspeed.JointUncertainty is windspeed.crosspol.JointUncertainty
    assert callable(windspeed._engine.uncertainty_joint_from_codes) and callable(windspeed.CopolCodes.uncertainty_joint)
    assert "uncertainty_joint" in windspeed.CopolCodes.uncertainty.__doc__
