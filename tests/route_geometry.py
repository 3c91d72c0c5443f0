"""Seven LUT geometries and one scene per geometry for the forced-route tests (tests/test_gpu_route_geometry.py on the GPU,
tests/test_route_geometry_cpu.py without one).  Everything here is numpy on the host and deterministic: the parent pytest
process builds tables, scenes and the CPU oracle's answer once, the child processes of the routes only load them.

Each geometry is there for a hazard of the inversion chain that the default 501 x 499 x 181 table cannot show:

  pad4_half     phi_pad 76 (76 % 8 == 4): the rows of the inverse-row table are 152 bytes apart, so every odd row's 16-byte read
                of eight directions (window_arc, live_arc) is misaligned and its groups straddle two rows
  pad4_full     directions 0..360, phi_pad 148 (% 8 == 4), w_pad != n_w, a cross-pol speed axis that is no multiple of 4.  By the
                reference's rule (180 - span < 2) such a table has phi_180 == 1 like a half circle: the a-priori azimuth is
                folded, and the directions past 180 degrees are candidates that only ever lose or tie
  open_half     directions 0..175: the only kind of axis with phi_180 == 0 (a span below 178 degrees) -- signed a-priori azimuth,
                360 added to directions below phi[0], windows that leave the axis at either end, no +-phi choice in the store --
                on a phi_pad % 8 == 4 table
  narrow        12 directions: fewer than two groups of 8, one block column; the groups of the table's last row read into the slack
  coarse_full   15 degree steps over 0..360: a block (16 directions) spans more than 170 degrees, so k_invert_blocks is off and list
                C's pixels must come out of k_invert_list
  tail          incidence 17..23 degrees: columns that fall again at high wind (rows past the monotone part: tail_min, tail sweep)
                on a phi_pad % 8 == 4 table
  default_like  the control: 181 directions, phi_pad 184
"""
import numpy as np

LINES, SAMPLES = 13, 333  # three whole workgroups of four lines + one of a single line; five whole strips of 64 samples + one of 13
DSIG_CO = 0.1
# line % 4 -> a-priori wind as a multiple of the truth, and the noise on it (m/s per component): the four waves of a workgroup hold
# narrow, wider, wider and whole-circle windows (as _classes_scene of test_gpu_band_pool.py, further apart)
SCALE = (1.0, 1.6, 0.6, 0.3)
NOISE = (0.2, 1.0, 1.5, 2.0)
PINNED_LINE = 6  # its a-priori directions sit within 2 degrees of phi[0] and phi[-1]: the seam, and the last group of 8

# (seed: of the scene.  The wide-window property of tests/test_route_geometry_cpu.py is statistical -- 58 of a strip's 64 pixels have a
# finite co-pol problem, some 6 of those a narrow window all the same -- and the seeds are the ones of 1..12 that leave it the most
# room: 50 or more of 64 in the worst strip.  w_true_max: `tail` keeps the true wind below 18 m/s -- at 17..23 degrees sigma0 saturates
# beyond, the a-priori speed itself then explains it and the window shrinks to a few directions -- which still sends the windows of the
# lines at 1.6 of the truth past the monotone rows (24 m/s and up))
GEOMETRIES = {
    "pad4_half": dict(seed=8, n_inc=3, n_w=120, n_phi=73, phi_last=180.0, n_wcr=115, inc=(30.0, 42.0)),
    "pad4_full": dict(seed=2, n_inc=3, n_w=97, n_phi=145, phi_last=360.0, n_wcr=33, inc=(30.0, 42.0)),
    "open_half": dict(seed=12, n_inc=3, n_w=97, n_phi=73, phi_last=175.0, n_wcr=33, inc=(30.0, 42.0)),
    "narrow": dict(seed=5, n_inc=2, n_w=40, n_phi=12, phi_last=180.0, n_wcr=115, inc=(30.0, 42.0)),
    "coarse_full": dict(seed=9, n_inc=3, n_w=90, n_phi=25, phi_last=360.0, n_wcr=60, inc=(30.0, 42.0)),
    "tail": dict(seed=9, w_true_max=18.0, n_inc=4, n_w=160, n_phi=73, phi_last=180.0, n_wcr=115, inc=(17.0, 23.0)),
    "default_like": dict(seed=2, n_inc=3, n_w=101, n_phi=181, phi_last=180.0, n_wcr=115, inc=(30.0, 42.0)),
}
W_RANGE = (0.2, 50.0)    # CMOD5.N's own speed range
WCR_RANGE = (3.0, 60.0)  # as test_random_configurations


def build_luts(name):
    """(co-pol, cross-pol) dB tables of one geometry: CMOD5.N and the S1 v2 cross-pol GMF on np.linspace axes."""
    from oracle import gmf, lut as olut
    g = GEOMETRIES[name]
    inc_ax = np.linspace(g["inc"][0], g["inc"][1], g["n_inc"])
    w_ax = np.linspace(W_RANGE[0], W_RANGE[1], g["n_w"])
    phi_ax = np.linspace(0.0, g["phi_last"], g["n_phi"])
    co = 10 * np.log10(gmf.gmf_cmod5n(inc_ax[:, None, None], w_ax[None, :, None], phi_ax[None, None, :]) + 1e-15)
    wcr_ax = np.linspace(WCR_RANGE[0], WCR_RANGE[1], g["n_wcr"])
    cr = 10 * np.log10(gmf.GMFS["gmf_s1_v2"][0](inc_ax[:, None], wcr_ax[None, :]) + 1e-15)
    return (olut.Lut(np.ascontiguousarray(co), inc_ax, w_ax, phi_ax, "dB", "x", "co", "VV"),
            olut.Lut(np.ascontiguousarray(cr), inc_ax, wcr_ax, None, "dB", "x", "cr", "VH"))


def build_scene(name, dtype):
    """One 13 x 333 raster of geometry `name` in `dtype` (float32 / float64): dict(inc, sco, scr, dsig, anc) with sigma0 in dB
    (host-computed in `dtype`, as test_random_configurations hands it over).  Incidences from 3 degrees below the axis to 3 above
    it, true directions over the table's whole range, the a-priori wind at SCALE[line % 4] of the truth with NOISE[line % 4] on
    it, PINNED_LINE's a-priori directions at the ends of the direction axis, about 3 % of every input raster NaN / 0 / inf."""
    from oracle import gmf
    from oracle import invert as oinv
    g = GEOMETRIES[name]
    rng = np.random.default_rng(g["seed"])
    shape, n = (LINES, SAMPLES), LINES * SAMPLES
    ln = np.arange(LINES)[:, None]
    # (the ramp's samples in a scrambled order: every strip of 64 then holds the whole range, slices that differ from lane to lane,
    # and its share of the pixels beyond the axis ends, whose sigma0 no speed near the truth explains)
    inc = np.linspace(g["inc"][0] - 3.0, g["inc"][1] + 3.0, SAMPLES)[(np.arange(SAMPLES) * 109) % SAMPLES][None, :] + 0.01 * ln
    wt = rng.uniform(3.0, g.get("w_true_max", 25.0), shape)
    folded = (180.0 - g["phi_last"]) < 2.0  # phi_180: the sign of the azimuth is the store's choice, so the truth takes both
    pt = rng.uniform(-180.0, 180.0, shape) if folded else rng.uniform(0.0, g["phi_last"], shape)
    pin = np.where(rng.random(SAMPLES) < 0.5, 0.0, g["phi_last"]) + rng.uniform(-2.0, 2.0, SAMPLES)
    pt[PINNED_LINE] = pin
    s_vv = gmf.gmf_cmod5n(np.clip(inc, 17.0, 65.0), wt, pt) * rng.gamma(100, 1 / 100, shape)
    s_vh = gmf.GMFS["gmf_s1_v2"][0](np.clip(inc, 17.0, 65.0), np.maximum(wt, 3.0)) * rng.gamma(100, 1 / 100, shape)
    scale, noise = np.array(SCALE)[ln % 4], np.array(NOISE)[ln % 4]
    anc = wt * scale * np.exp(1j * np.deg2rad(pt)) + noise * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    anc[PINNED_LINE] = (wt * scale)[PINNED_LINE] * np.exp(1j * np.deg2rad(pin))  # no noise: the direction stays within 2 degrees
    dsig = 10 ** rng.uniform(-3, 1, shape)
    k = max(1, n // 33)  # ~3 % of each raster
    # (sigma0_co: mostly inf -- a pixel with a non-finite co-pol problem is k_invert_list's whatever the route, and the 64 entries of
    # list G under XSW_LIST_CAP_TEST=64 must not hold them: some 85 per raster)
    for arr, vals, p in ((inc, [np.nan], None), (s_vv, [np.nan, 0.0, np.inf, -1.0], [0.1, 0.1, 0.7, 0.1]), (s_vh, [np.nan, 0.0], None),
                         (dsig, [np.nan, 0.0, np.inf], None)):
        arr.ravel()[rng.integers(0, n, k)] = rng.choice(vals, k, p=p)
    anc.ravel()[rng.integers(0, n, k // 2)] = complex(np.nan, 0)
    anc.ravel()[rng.integers(0, n, k // 2)] = 0j
    dt = np.dtype(dtype)
    cdt = np.complex64 if dt == np.float32 else np.complex128
    inc, s_vv, s_vh, dsig = (np.ascontiguousarray(a, dtype=dt) for a in (inc, s_vv, s_vh, dsig))
    with np.errstate(all="ignore"):
        sco, scr = oinv.to_db(s_vv), oinv.to_db(s_vh)
    return dict(inc=inc, sco=sco, scr=scr, dsig=dsig, anc=np.ascontiguousarray(anc, dtype=cdt))


def oracle_answer(lco, lcr, sc):
    """The CPU oracle on one scene: (co, cr, idx) of the dual-pol call.  The co-pol part of it is the mono call's answer as well
    (the reference's co-pol search never reads the cross-pol inputs).  The C restatement on an incidence-major copy where it is
    built (identical arithmetic, what test_random_configurations_large_axes trusts), the numpy restatement otherwise."""
    from oracle import invert as oinv
    p = oinv.Prepared(lco, lcr, DSIG_CO)
    try:
        from oracle import cport
        cport.lib()
    except Exception:
        return oinv.invert_numpy(p, sc["inc"], sc["sco"], sc["scr"], sc["dsig"], sc["anc"], return_idx=True)
    return cport.invert_numpy(p, sc["inc"], sc["sco"], sc["scr"], sc["dsig"], sc["anc"], return_idx=True, reference_layout=False)


def window_columns(lco, sc):
    """Directions of every pixel's search window (tests/prune_model.py: the ray bound of pruned_argmin, then search_window), 0
    where the pixel has no finite co-pol problem: int array of the raster's shape."""
    import prune_model as pm
    wspd, phi = np.asarray(lco.wspd), np.asarray(lco.phi)
    n_w, n_phi = len(wspd), len(phi)
    phi_180 = (180.0 - (phi[-1] - phi[0])) < 2.0
    cphi, sphi = np.cos(np.radians(phi)), np.sin(np.radians(phi))
    w0, inv_wstep = wspd[0], (n_w - 1) / (wspd[-1] - wspd[0])
    phi0, inv_dphi = phi[0], (n_phi - 1) / (phi[-1] - phi[0])
    wh = 0.5 * wspd
    inc, sco, anc = (np.asarray(sc[k]) for k in ("inc", "sco", "anc"))
    out = np.zeros(inc.shape, dtype=np.int64)
    inv = 1.0 / DSIG_CO
    for i in np.ndindex(inc.shape):
        s, a, b = float(sco[i]), float(anc[i].real), float(anc[i].imag)
        if phi_180:
            b = abs(b)
        if not (np.isfinite(inc[i]) and np.isfinite(s) and np.isfinite(a) and np.isfinite(b)):
            continue
        col_all = lco.values[int(np.argmin(np.abs(lco.incidence - float(inc[i]))))]
        ah, bh = 0.5 * a, 0.5 * b
        m2 = ah * ah + bh * bh
        theta = np.degrees(np.arctan2(b, a))
        if theta < phi0:
            theta += 360.0
        ipr = int(np.clip(np.rint((theta - phi0) * inv_dphi), 0, n_phi - 1))
        ur = 2.0 * (ah * cphi[ipr] + bh * sphi[ipr])
        j_ub = np.min(wh * (wh - ur) + (col_all[:, ipr] * inv - s * inv) ** 2) + m2  # (the whole ray: at most the bisection's bound)
        _, _, ip_lo, ip_hi = pm.search_window(np.hypot(a, b), theta, j_ub, w0, inv_wstep, n_w, phi0, phi[-1], inv_dphi, n_phi)
        out[i] = max(ip_hi - ip_lo + 1, 0)
    return out
