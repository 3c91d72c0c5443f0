"""k_invert_band with the cos / sin table of the directions in LDS (xsw_band.hpp: kBandCsCap, ChainPlan::cs_lds) and with results
and lane -> slot words inside the slots.  Every candidate is still scored with the same doubles, so the fast path must equal the
exhaustive sweep bit for bit: on either side of the table-size threshold between the LDS route and the one that reads global
memory, in every window class, in the statistics instantiation, and -- what pins sigma0 -> dB (xsw_device.hpp: to_db(float)) for
NaN / 0 / inf / negative sigma0, whichever way it treats them -- in waves that hold one, only, or no special sigma0."""
import numpy as np
import pytest

import prune_model as pm
from test_gpu_band_pool import _classes_scene, _mono_equal
from util import bits_equal, lut_dicts

pytestmark = pytest.mark.gpu

CS_CAP = 192  # kBandCsCap (xsw_band.hpp): directions the LDS copy of the table holds
DSIG_CO = 0.1  # invert_host's default


def _cmod_lut(n_phi, phi_last, n_w=101, n_inc=5):
    """CMOD5.N in dB on np.linspace axes: incidence 30..46 degrees (what synthetic_scene spans), n_phi directions over 0..phi_last."""
    from oracle import gmf, lut as olut
    inc_ax, w_ax, phi_ax = np.linspace(30.0, 46.0, n_inc), np.linspace(0.2, 50.0, n_w), np.linspace(0.0, phi_last, n_phi)
    co = 10 * np.log10(gmf.gmf_cmod5n(inc_ax[:, None, None], w_ax[None, :, None], phi_ax[None, None, :]) + 1e-15)
    return olut.Lut(np.ascontiguousarray(co), inc_ax, w_ax, phi_ax, "dB", "x", "co", "VV")


def _install(ctx, lco):
    co, _ = lut_dicts(lco, None)
    ctx.upload_luts(co=co)


@pytest.fixture(scope="module")
def restore_default(gpu_ctx, default_luts):
    """The tests here install tables of their own on the session's context: the default ones are put back afterwards."""
    yield
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)


def _window_class(nv):
    """band_wave's class of a window of nv directions: the smallest of S x K = 4, 6, 8, 12, ..., 96, 128 that holds it (10: wider)."""
    if nv <= 4:
        return 0
    p2 = int(np.floor(np.log2(max(nv, 2) - 1)))
    return min(2 * p2 - 3 + (1 if nv > (3 << (p2 - 1)) else 0), 10)


def _windows(lco, inc, s_vv, anc):
    """(first direction, directions) of every pixel's search window by tests/prune_model.py (the bound of the whole ray along the
    a-priori direction, then search_window); 0 directions where the pixel has no finite co-pol problem."""
    from oracle import invert as oinv
    wspd, phi = np.asarray(lco.wspd), np.asarray(lco.phi)
    n_w, n_phi = len(wspd), len(phi)
    phi_180 = (180.0 - (phi[-1] - phi[0])) < 2.0
    cphi, sphi = np.cos(np.radians(phi)), np.sin(np.radians(phi))
    w0, inv_wstep = wspd[0], (n_w - 1) / (wspd[-1] - wspd[0])
    phi0, inv_dphi = phi[0], (n_phi - 1) / (phi[-1] - phi[0])
    wh, inv = 0.5 * wspd, 1.0 / DSIG_CO
    with np.errstate(all="ignore"):
        sco = oinv.to_db(s_vv)
    ip_lo_all, ncols = np.zeros(inc.shape, dtype=np.int64), np.zeros(inc.shape, dtype=np.int64)
    for i in np.ndindex(inc.shape):
        s, a, b = float(sco[i]), float(anc[i].real), float(anc[i].imag)
        if phi_180:
            b = abs(b)
        if not (np.isfinite(inc[i]) and np.isfinite(s) and np.isfinite(a) and np.isfinite(b)):
            continue
        col_all = lco.values[int(np.argmin(np.abs(lco.incidence - float(inc[i]))))]
        ah, bh = 0.5 * a, 0.5 * b
        theta = np.degrees(np.arctan2(b, a))
        if theta < phi0:
            theta += 360.0
        ipr = int(np.clip(np.rint((theta - phi0) * inv_dphi), 0, n_phi - 1))
        ur = 2.0 * (ah * cphi[ipr] + bh * sphi[ipr])
        j_ub = np.min(wh * (wh - ur) + (col_all[:, ipr] * inv - s * inv) ** 2) + ah * ah + bh * bh
        _, _, ip_lo, ip_hi = pm.search_window(np.hypot(a, b), theta, j_ub, w0, inv_wstep, n_w, phi0, phi[-1], inv_dphi, n_phi)
        ip_lo_all[i], ncols[i] = ip_lo, max(ip_hi - ip_lo + 1, 0)
    return ip_lo_all, ncols


# cap - 1, cap, cap + 1 directions over the half circle: the LDS route, the LDS route with its last entry in use, the route that
# reads global memory; and a whole circle (folded a-priori azimuth, candidates past 180 degrees) that fills the LDS table
TABLES = {"cap_minus_1": (CS_CAP - 1, 180.0), "cap": (CS_CAP, 180.0), "cap_plus_1": (CS_CAP + 1, 180.0), "full_circle_cap": (CS_CAP, 360.0)}


@pytest.mark.parametrize("table", sorted(TABLES))
def test_table_size_routes(gpu_ctx, restore_default, table):
    """Rasters of 7 x 130 and 9 x 333 pixels (heights no multiple of 4, widths no multiple of 64) on tables just below, at and
    just above the capacity of the LDS copy."""
    n_phi, phi_last = TABLES[table]
    _install(gpu_ctx, _cmod_lut(n_phi, phi_last))
    for lines, samples, seed in ((7, 130, 31), (9, 333, 32)):
        inc, s_vv, anc = _classes_scene(lines, samples, seed)
        _mono_equal(gpu_ctx, inc, s_vv, anc, (table, lines, samples))


def test_every_window_class(gpu_ctx, restore_default, default_luts):
    """The default table (181 directions: the LDS route).  Conditions the scene is chosen to meet, shown on the CPU: every
    window class occurs, and the winning directions include the table's first and last entry."""
    lco, _ = default_luts
    _install(gpu_ctx, lco)
    lines, samples = 16, 333
    inc, s_vv, anc = _classes_scene(lines, samples, 11)
    _, ncols = _windows(lco, inc, s_vv, anc)
    classes = {_window_class(int(n)) for n in ncols.ravel() if n > 0}
    assert classes == set(range(11)), sorted(classes)
    got = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
    ex = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    assert bits_equal(got[0], ex[0])
    assert np.array_equal(got[2], ex[2])
    won = set(ex[2][..., 1][ncols > 0].tolist())
    assert 0 in won and len(lco.phi) - 1 in won, (min(won), max(won))


def test_second_chunk_of_the_widest_class(gpu_ctx, restore_default):
    """A window of more than 192 directions is swept in chunks of 64 x 3, and a table with that many directions is beyond the LDS
    copy: the route that reads global memory, on 361 directions over the half circle.  Condition shown on the CPU: some pixel's
    window is wider than a chunk and its winning direction lies in the second one."""
    lco = _cmod_lut(361, 180.0)
    _install(gpu_ctx, lco)
    inc, s_vv, anc = _classes_scene(12, 200, 13)
    ip_lo, ncols = _windows(lco, inc, s_vv, anc)
    got = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
    ex = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    assert bits_equal(got[0], ex[0])
    assert np.array_equal(got[2], ex[2])
    assert np.any((ncols > 3 * 64) & (ex[2][..., 1] - ip_lo >= 3 * 64))


def test_statistics_instantiation_same_winds(gpu_ctx, restore_default, default_luts):
    """The statistics instantiation of k_invert_band (every window swept there, candidates counted) reads the LDS table as well."""
    lco, _ = default_luts
    _install(gpu_ctx, lco)
    inc, s_vv, anc = _classes_scene(7, 333, 5)
    ex = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    gpu_ctx.stats_enable(True)
    try:
        got = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
        counted = gpu_ctx.stats()
    finally:
        gpu_ctx.stats_enable(False)
    assert counted["cand_co"] > 0
    assert bits_equal(got[0], ex[0])
    assert np.array_equal(got[2], ex[2])


def test_sigma0_specials(gpu_ctx, restore_default, default_luts):
    """float32 rasters of linear sigma0, 8 x 192: of the 24 waves (strips of 64 samples) a third hold no special sigma0, a third
    exactly one, a third nothing else -- NaN, +inf, 0, -1e-15f (the dB offset cancels it: log10(0)), -1, the smallest denormal,
    FLT_MAX.  The NaN mask is the reference's (NaN where the incidence or sigma0 in dB is), and everything equals the exhaustive
    route's."""
    from oracle import invert as oinv
    from test_gpu_kernel import synthetic_scene
    lco, _ = default_luts
    _install(gpu_ctx, lco)
    lines, samples = 8, 192
    inc, s_vv, _, _, anc = synthetic_scene(lines, samples, np.float32, 41)
    s_vv = np.where(np.isnan(s_vv), np.float32(0.01), s_vv)  # (the generator's own NaN pixels: the waves' contents are set below)
    specials = np.array([np.nan, np.inf, 0.0, -1e-15, -1.0, 1e-45, np.finfo(np.float32).max], dtype=np.float32)
    assert specials[5] > 0 and specials[5] < np.finfo(np.float32).tiny
    for ln in range(lines):
        for st in range(samples // 64):
            w = ln * (samples // 64) + st
            sl = slice(64 * st, 64 * st + 64)
            if w % 3 == 1:
                s_vv[ln, 64 * st + (7 * w + 3) % 64] = specials[(w // 3) % len(specials)]
            elif w % 3 == 2:
                s_vv[ln, sl] = specials[(np.arange(64) + w) % len(specials)]
    got = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
    ex = gpu_ctx.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    with np.errstate(all="ignore"):
        sdb = oinv.to_db(s_vv)
    assert sdb.dtype == np.float32
    want_nan = np.isnan(inc) | np.isnan(sdb)
    assert np.isnan(sdb).sum() >= 3 * 8 and np.isinf(sdb).sum() >= 3 * 8  # (NaN, -1 -> NaN; +inf -> +inf, -1e-15f -> -inf)
    assert np.array_equal(np.isnan(got[0].real), want_nan)
    assert bits_equal(got[0], ex[0])
    assert np.array_equal(got[2], ex[2])
