"""Tables, scenes and a CPU model of stage 1 for tests/test_gpu_band_slot.py: rasters built pixel by pixel so that k_invert_band
ITSELF (not the kernels it hands pixels to) meets every way its passes address the tables from the slot's packed offsets
(csrc/xsw_bandslot.hpp).  Everything here is numpy on the host and deterministic.

A pixel is made from a recipe: an incidence ON a node of the table's axis (the slice is then known), a true wind ON a node of
the speed and direction axes, sigma0 of that wind without speckle, and an a-priori wind along the true direction at a fraction
f < 1 of the true speed.  The upper bound along the a-priori direction is then the wind term of the truth, (1 - f)^2 w^2 / 4, the
search disc has radius (1 - f) w around f w, and the window spans asin((1 - f) / f) to either side: f sets the window class.  Low true speeds keep the band a row or two long
(sigma0 moves by 0.3 dB per 0.1 m/s at 3 m/s, the band's half width is 0.1 sqrt(J_ub) dB), so the pixel is not handed to
k_invert_band2 for its run length (XSW_LONG_RUN_DEFAULT = 5 rows, csrc/xsw_plan.hpp).

`stage1` restates what stage 1 of k_invert_band parks for a pixel (tests/prune_model.py: three rays, window, band radius, tail
cut, table bins; then the run length along the a-priori direction from the inverse-row table) and says whether the pixel stays
with k_invert_band under the default route knobs.  The tests use it to SHOW that the conditions they are after occur among such
pixels; the share of pixels k_invert_band decides is asserted from the device's own hand-over counters."""
import numpy as np

import lut_tables_ref as ltr
import prune_model as pm
import route_geometry as rg

DSIG_CO = 0.1
LONG_RUN, B2_AREA, ARC_MIN, ARC_CROWD = 5, 2048, 32, 48  # XSW_LONG_RUN_DEFAULT, XSW_B2_AREA, XSW_ARC_MIN, XSW_ARC_CROWD (csrc/xsw_plan.hpp)
CLASS_CAP = (4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)    # directions a window class holds (band_wave); wider: chunks of 192
CHUNK = 192


def luts(name):
    """(co-pol, cross-pol) tables: "default" 501 x 499 x 181 (phi_pad 184, the LDS direction table); "pad4" 3 x 120 x 73
    (phi_pad 76, 76 % 8 == 4: route_geometry's pad4_half); "wide" 5 x 101 x 361 over the half circle (more than 192 directions:
    the instantiation that reads the direction table from global memory, and windows of two chunks)."""
    from oracle import gmf, lut as olut
    if name == "default":
        return olut.to_lut("gmf_cmod5n"), olut.to_lut("gmf_s1_v2")
    if name == "pad4":
        return rg.build_luts("pad4_half")
    assert name == "wide"
    inc_ax, w_ax, phi_ax = np.linspace(30.0, 46.0, 5), np.linspace(0.2, 50.0, 101), np.linspace(0.0, 180.0, 361)
    co = 10 * np.log10(gmf.gmf_cmod5n(inc_ax[:, None, None], w_ax[None, :, None], phi_ax[None, None, :]) + 1e-15)
    return olut.Lut(np.ascontiguousarray(co), inc_ax, w_ax, phi_ax, "dB", "x", "co", "VV"), rg.build_luts("default_like")[1]


def window_class(nv):
    """band_wave's class of a window of nv directions: the smallest of CLASS_CAP that holds it (10: wider as well)."""
    return next((c for c, cap in enumerate(CLASS_CAP) if nv <= cap), 10)


class Tables:
    """Per-slice tables of a co-pol LUT that stage 1 reads, restated by tests/lut_tables_ref.py."""

    def __init__(self, lco):
        self.lco = lco
        dense = np.asarray(lco.values)
        self.mono = ltr.mono_rows(dense)
        self.grid = ltr.inv_grid(dense, self.mono)

    def inv_row(self, i_inc, ip, b):
        """inv_rows[i_inc][b][ip]: the first monotone row of the column at or above threshold b (bin 0: row 0)."""
        if b == 0:
            return 0
        t0, width, _ = self.grid[i_inc]
        m = int(self.mono[i_inc])
        return int(np.searchsorted(np.asarray(self.lco.values)[i_inc, :m, ip], ltr.fma(float(b), float(width), float(t0)), side="left"))


def stage1(tab, inc, s_lin, a):
    """What stage 1 of k_invert_band finds for one float32 pixel, or None where the pixel has no finite co-pol problem: dict of
    elig (the band rule applies), i_inc, w_lo, w_hi, ip_lo, ncols, b_lo, b_hi (-1: no threshold above s + d), below (s - d lies
    below the threshold grid), run (rows of the band along the a-priori direction) and kept (k_invert_band sweeps the pixel
    itself under the default knobs: eligible, no tail, run below XSW_LONG_RUN_DEFAULT, run x directions within XSW_B2_AREA)."""
    from oracle import invert as oinv
    lco = tab.lco
    wspd, phi = np.asarray(lco.wspd), np.asarray(lco.phi)
    n_w, n_phi = len(wspd), len(phi)
    phi_180 = (180.0 - (phi[-1] - phi[0])) < 2.0
    with np.errstate(all="ignore"):
        s = float(oinv.to_db(s_lin))  # (float32 in, float32 out: the device's own conversion, tests/test_gpu_db_f32.py)
    ar, b = float(a.real), float(a.imag)
    if phi_180:
        b = abs(b)
    if not (np.isfinite(inc) and np.isfinite(s) and np.isfinite(ar) and np.isfinite(b)):
        return None
    i_inc = int(np.argmin(np.abs(np.asarray(lco.incidence) - float(inc))))
    sl = np.asarray(lco.values)[i_inc]
    cphi, sphi = np.cos(np.radians(phi)), np.sin(np.radians(phi))
    w0, inv_wstep = wspd[0], (n_w - 1) / (wspd[-1] - wspd[0])
    phi0, inv_dphi = phi[0], (n_phi - 1) / (phi[-1] - phi[0])
    inv, wh = 1.0 / DSIG_CO, 0.5 * wspd
    sn, ah, bh = -s * inv, 0.5 * ar, 0.5 * b
    m2 = ah * ah + bh * bh
    theta = np.degrees(np.arctan2(b, ar))
    if theta < phi0:
        theta += 360.0
    ipr = int(np.clip(np.rint((theta - phi0) * inv_dphi), 0, n_phi - 1))
    npairs, rbest, seed = (n_w + 1) >> 1, np.inf, 0
    for q, ipq in enumerate((ipr, max(ipr - 2, 0), min(ipr + 2, n_phi - 1))):
        ur = 2.0 * (ah * cphi[ipq] + bh * sphi[ipq])
        lo, hi = (0, npairs) if q == 0 else (max(seed - 4, 0), min(seed + 4, npairs))
        col = sl[:, ipq]
        for _ in range(int(npairs).bit_length() if q == 0 else 3):
            mid = min((lo + hi) >> 1, npairs - 1)
            ja = wh[2 * mid] * (wh[2 * mid] - ur) + (col[2 * mid] * inv + sn) ** 2
            jb = wh[2 * mid + 1] * (wh[2 * mid + 1] - ur) + (col[2 * mid + 1] * inv + sn) ** 2 if 2 * mid + 1 < n_w else np.inf
            rbest = min(rbest, ja, jb)
            if lo < hi:
                lo, hi = (mid + 1, hi) if jb < ja else (lo, mid)
        if q == 0:
            seed = lo
    j_ub = (rbest + m2) * (1.0 + 1e-9) + 1e-9
    w_lo, w_hi, ip_lo, ip_hi = pm.search_window(np.sqrt(ar * ar + b * b), theta, rbest + m2, w0, inv_wstep, n_w, phi0, phi[-1], inv_dphi, n_phi)
    d = pm.band_radius(j_ub, DSIG_CO)
    mono = int(tab.mono[i_inc])
    tail = False
    if w_hi >= mono and ip_hi >= ip_lo:
        if s + d < pm.tail_min(sl, mono, ip_lo, ip_hi):
            w_hi = mono - 1
        else:
            tail = True
    ncols = max(ip_hi - ip_lo + 1, 0)
    elig = not tail and w_hi < mono and w_hi >= w_lo and ncols >= 1
    t0, width, inv_width = (float(v) for v in tab.grid[i_inc])
    b_lo, b_hi = pm.table_bins(t0, width, inv_width, ltr.INV_BINS, s - d, s + d)
    run = 0
    if elig:
        first, last = pm.band_rows_from_table({b_lo: tab.inv_row(i_inc, ipr, b_lo), b_hi: tab.inv_row(i_inc, ipr, b_hi) if b_hi >= 0 else 0},
                                              b_lo, b_hi, w_lo, w_hi)
        run = last - first + 1
    kept = bool(elig and run < LONG_RUN and run * ncols <= B2_AREA)
    return dict(elig=bool(elig), i_inc=i_inc, w_lo=w_lo, w_hi=w_hi, ip_lo=ip_lo, ncols=ncols, b_lo=b_lo, b_hi=b_hi, below=(s - d) < t0, run=run,
                kept=kept, ipr=ipr)


# directions a recipe's window is meant to span: one per window class, one of more than 128 and one of more than a chunk
TARGETS = (3, 5, 7, 10, 14, 20, 28, 40, 56, 80, 112, 150, 260)


def scene(lco, lcr, lines, samples, seed):
    """float32 rasters (inc, s_vv, s_vh, dsig, anc as complex64) of lines x samples pixels, one recipe per pixel (module
    docstring), the recipes dealt so that every strip of 64 samples holds all of them:

      * window recipes, one per entry of TARGETS that the table's directions can hold, on random slices, on the first and on the
        last one, and with the true direction on the first / the last node of the direction axis;
      * "below": sigma0 a little below the smallest value of the slice (first and last slice): s - d lies below the threshold grid;
      * "above": sigma0 a little above the largest value of the last slice, the a-priori speed just below the top of the speed axis:
        no threshold above s + d, windows that end at the table's last row;
      * NaN holes: sigma0 (3 %), incidence and a-priori wind (1 % each); and infinite sigma0 (every 97th pixel): searchable pixels that are
        k_invert_list's whatever the route -- the hand-over counters the tests read must show them."""
    from oracle import gmf
    rng = np.random.default_rng(seed)
    inc_ax, wspd, phi = np.asarray(lco.incidence), np.asarray(lco.wspd), np.asarray(lco.phi)
    vals = np.asarray(lco.values)
    n_inc, n_phi = len(inc_ax), len(phi)
    dphi = (phi[-1] - phi[0]) / (n_phi - 1)
    targets = [t for t in TARGETS if t <= n_phi]
    recipes = [("window", t, where) for t in targets for where in ("any", "any")]
    recipes += [("window", t, where) for t in targets[:6] for where in ("first_slice", "last_slice", "first_dir", "last_dir")]
    recipes += [("below", 0, "first_slice"), ("below", 0, "last_slice"), ("above", 0, "last_slice"), ("above", 0, "last_slice")]
    n = lines * samples
    order = np.concatenate([rng.permutation(len(recipes)) for _ in range(n // len(recipes) + 1)])[:n]
    inc, s_vv, wt, anc = np.empty(n), np.empty(n), np.empty(n), np.empty(n, dtype=complex)
    for k in range(n):
        kind, t, where = recipes[order[k]]
        i = {"first_slice": 0, "last_slice": n_inc - 1}.get(where, int(rng.integers(0, n_inc)))
        p = {"first_dir": phi[0], "last_dir": phi[-1]}.get(where, phi[int(rng.integers(0, n_phi))])
        if kind == "window":
            # (the truth ON a node of the speed and of the direction axis: the bound along the a-priori direction is then the
            # wind term alone -- off the nodes the sigma0 term of the nearest row dominates it and every window comes out wide)
            w = wspd[np.argmin(np.abs(wspd - (rng.uniform(2.5, 4.0) if t >= 20 else rng.uniform(4.0, 8.0))))]
            half = np.radians(0.5 * (t - 1) * dphi)
            f = 1.0 / (1.0 + np.sin(half)) if half < 0.5 * np.pi else 0.45
            s, a = gmf.gmf_cmod5n(inc_ax[i], w, p), f * w * np.exp(1j * np.radians(p))
        elif kind == "below":
            ip = int(np.argmin(vals[i, 0]))
            w = wspd[0]
            s, a = 10.0 ** (vals[i, 0, ip] / 10.0) * (1.0 - 1e-3), 0.9 * w * np.exp(1j * np.radians(phi[ip]))
        else:
            ip = int(np.argmax(vals[i, -1]))
            w = wspd[-1]
            s, a = 10.0 ** (vals[i, -1, ip] / 10.0) * 1.01, 0.998 * w * np.exp(1j * np.radians(phi[ip]))
        inc[k], s_vv[k], wt[k], anc[k] = inc_ax[i], s, w, a
    shape = (lines, samples)
    inc, s_vv, wt, anc = inc.reshape(shape), s_vv.reshape(shape), wt.reshape(shape), anc.reshape(shape)
    s_vh = gmf.GMFS["gmf_s1_v2"][0](np.clip(inc, np.asarray(lcr.incidence)[0], np.asarray(lcr.incidence)[-1]), np.maximum(wt, 3.0)) + 10 ** -3.5
    dsig = (1.25 / (s_vh / 10 ** -3.5)) ** 4.0
    is_inf = (np.arange(n) % 97 == 50).reshape(shape)  # (three of 5 x 70, eighteen of 9 x 200)
    s_vv[rng.random(shape) < 0.03] = np.nan
    inc[(rng.random(shape) < 0.01) & ~is_inf] = np.nan
    anc[(rng.random(shape) < 0.01) & ~is_inf] = complex(np.nan, 0.0)
    s_vv[is_inf] = np.inf
    return inc.astype(np.float32), s_vv.astype(np.float32), s_vh.astype(np.float32), dsig.astype(np.float32), anc.astype(np.complex64)


def searchable(inc, s_vv, anc):
    """Pixels with a co-pol search: incidence and sigma0 not NaN (inf counts), |a-priori wind| not NaN."""
    with np.errstate(all="ignore"):
        return int(np.sum(~np.isnan(inc) & ~np.isnan(s_vv) & ~np.isnan(np.abs(anc))))


def survey(tab, inc, s_vv, anc):
    """The model over a raster: (list of stage1 dicts of the pixels k_invert_band keeps, with their raster index as "at"; the
    largest number of pixels with ARC_MIN directions or more in one wave = one strip of 64 samples of one line)."""
    kept, crowd = [], 0
    lines, samples = inc.shape
    for ln in range(lines):
        for st in range(0, samples, 64):
            wide = 0
            for sm in range(st, min(st + 64, samples)):
                m = stage1(tab, inc[ln, sm], s_vv[ln, sm], anc[ln, sm])
                if m is None:
                    continue
                wide += m["elig"] and m["ncols"] >= ARC_MIN
                if m["kept"]:
                    m["at"] = (ln, sm)
                    kept.append(m)
            crowd = max(crowd, wide)
    return kept, crowd
