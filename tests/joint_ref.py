"""CPU restatement of the joint dual-pol inversion from stored co-pol grid codes (test infrastructure; the executable specification
of k_joint_from_codes / xsw_joint_from_codes).

Per pixel the DENSE cost over the whole co-pol grid is formed in numpy,

    J = (Jwind_co + Jsig_co) + Jsig_cr[:, None]

Jwind_co / Jsig_co by the expressions of `cost_codes_ref.cost_co` (the reference's own, windspeed/windspeed.py:216-225) on the
tables `oracle.invert.Prepared` builds, Jsig_cr per co-pol speed row from the cross-pol table at that speed (`jsig_cr_rows`:
the table is held constant beyond its speed axis, interpolated linearly inside it with tests/forward_ref.py's statements), and
the answer is `np.argmin(J)`: the first minimum in flat order iw * n_phi + ip.  float64, IEEE + - * / only (numpy fuses nothing).

Gates, in this order: XSW_CODE_NAN / XSW_CODE_NAN_RE keep their code; a code of no LUT or a NaN incidence gives XSW_CODE_NAN_RE
(costs NaN in all of these); a grid code next to a NaN sigma0_cr / dsig_cr keeps its code with J = J_co at its point and Jsig_cr
NaN; otherwise J_ub = J at the input code's point must be finite, else XSW_CODE_NAN with NaN costs.  The -phi bit of a 0..180
table is the inversion's own rule (:234-242) applied to the joint grid point.

`joint(..., pruned=True)` also proves, pixel by pixel, the claim the kernel relies on: the arg-min lies in the set
{Jwind_co <= J_ub} intersected with the rows {Jsig_cr <= J_ub}; it returns that set's size."""
import numpy as np

from crosspol_codes_ref import CODE_NAN, CODE_NAN_RE

FIELDS = ("J", "Jwind", "Jsig_co", "Jsig_cr")


def jsig_cr_rows(p, i_inc_cr, s_cr_db, dsig_cr):
    """Jsig_cr of every co-pol speed row (rule 3)."""
    w, wcr, cr = p.wspd_dim, p.wspd_cr, p.cr_lut[:, i_inc_cr]
    if wcr.size >= 2:
        x = np.minimum(np.maximum(w, wcr[0]), wcr[-1])
        k = np.clip(np.searchsorted(wcr, x), 1, wcr.size - 1)
        slope = (cr[k] - cr[k - 1]) / (wcr[k] - wcr[k - 1])
        crw = slope * (x - wcr[k - 1]) + cr[k - 1]
    else:
        crw = np.full(w.shape, cr[0])
    d = (crw - s_cr_db) / dsig_cr
    return d * d


def _sign(p, iw, ip, one_ancillary_wind):
    """windspeed.py:234-242 at grid point (iw, ip): 1 when the -phi solution is stored."""
    if not p.phi_180:
        return 0
    wspd_co, wphi_co = p.wspd_lut[iw, ip], p.phi_lut[iw, ip]
    sol = wspd_co * np.exp(1j * np.deg2rad(wphi_co))
    sol_2 = wspd_co * np.exp(1j * (np.deg2rad(-wphi_co)))
    diff_angle = np.angle(one_ancillary_wind / sol)
    diff_angle_2 = np.angle(one_ancillary_wind / sol_2)
    return 0 if np.abs(diff_angle) <= np.abs(diff_angle_2) else 1


def joint(code_co, inc, s_co_db, anc, dsig_co, s_cr_db, dsig_cr, p, pruned=False):
    """dict(code uint32, J, Jwind, Jsig_co, Jsig_cr float64) of every pixel; sigma0 already in dB, dsig_cr a raster (a scalar
    already broadcast), p = oracle.invert.Prepared(lut_co, lut_cr).  pruned=True adds `n_pruned` (int64, -1 where no search ran)
    after asserting that the arg-min lies in the pruned set."""
    shape = np.shape(inc)
    flat64 = lambda a, t=np.float64: np.ascontiguousarray(np.broadcast_to(np.asarray(a), shape)).astype(t).ravel()
    code_in = np.ascontiguousarray(np.broadcast_to(np.asarray(code_co, dtype=np.uint32), shape)).ravel()
    inc_1d, s_co_1d, s_cr_1d, dsig_1d, anc_1d = flat64(inc), flat64(s_co_db), flat64(s_cr_db), flat64(dsig_cr), flat64(anc, np.complex128)
    n, n_phi, plane = inc_1d.size, p.phi_dim.size, p.wspd_dim.size * p.phi_dim.size
    out = {k: np.full(n, np.nan) for k in FIELDS}
    code = code_in.copy()
    n_pruned = np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for i in range(n):
            c = int(code_in[i])
            if c in (CODE_NAN, CODE_NAN_RE):
                continue
            flat0 = c & 0x3FFFFFFF
            if (c & 0x80000000) or flat0 >= plane or np.isnan(inc_1d[i]):
                code[i] = CODE_NAN_RE
                continue
            one_inc, one_sigma0_co_db, one_ancillary_wind = inc_1d[i], s_co_1d[i], anc_1d[i]
            lut_inc = p.co_lut[:, :, np.argmin(np.abs(p.inc_dim - one_inc))]
            m_antenna, m_azi = np.real(one_ancillary_wind), np.imag(one_ancillary_wind)
            if p.phi_180:
                m_azi = np.abs(m_azi)
            Jwind_co = ((p.lut_co_antenna - m_antenna) / p.d_antenna) ** 2 + ((p.lut_co_azi - m_azi) / p.d_azi) ** 2
            Jsig_co = ((lut_inc - one_sigma0_co_db) / dsig_co) ** 2
            J_co = Jwind_co + Jsig_co
            at = (flat0 // n_phi, flat0 % n_phi)
            if np.isnan(s_cr_1d[i]) or np.isnan(dsig_1d[i]):  # no cross-pol information: the co-pol answer and its cost
                out["J"][i], out["Jwind"][i], out["Jsig_co"][i] = J_co[at], Jwind_co[at], Jsig_co[at]
                continue
            rows = jsig_cr_rows(p, np.argmin(np.abs(p.inc_cr_dim - one_inc)), s_cr_1d[i], dsig_1d[i])
            J_ub = J_co[at] + rows[at[0]]
            if not np.isfinite(J_ub):
                code[i] = CODE_NAN
                continue
            J = J_co + rows[:, None]
            best = int(np.argmin(J))
            at = (best // n_phi, best % n_phi)
            if pruned:
                keep = (Jwind_co <= J_ub) & (rows <= J_ub)[:, None]
                assert keep[at], f"pixel {i}: the dense arg-min {at} lies outside the pruned set (J_ub {J_ub})"
                n_pruned[i] = int(keep.sum())
            code[i] = best | (_sign(p, at[0], at[1], one_ancillary_wind) << 30)
            out["J"][i], out["Jwind"][i], out["Jsig_co"][i], out["Jsig_cr"][i] = J[at], Jwind_co[at], Jsig_co[at], rows[at[0]]
    res = {k: v.reshape(shape) for k, v in out.items()}
    res["code"] = code.reshape(shape)
    if pruned:
        res["n_pruned"] = n_pruned.reshape(shape)
    return res


def recipe(rng, n, p, dtype=np.float64):
    """n pixels of the experiment behind DESIGN.md section 19, as (inc, sigma0_co_db, sigma0_cr_db, dsig_cr, anc) of `dtype`
    (complex for anc): incidence 18..46 deg, true speed 1.5..45 m/s, true direction 0..180 deg, sigma0 from the tables' nearest
    grid point, VV noise 0.3 dB, dsig_cr = 2.0 / 0.5 / 0.15 dB below 8 / below 15 / from 15 m/s times U(0.7, 1.4), VH noise
    N(0, 1) dsig_cr, a-priori = truth times U(0.6, 1.5) in speed, plus N(0, 25 deg) in direction."""
    inc = rng.uniform(18.0, 46.0, n)
    wspd, phi = rng.uniform(1.5, 45.0, n), rng.uniform(0.0, 180.0, n)
    near = lambda ax, x: np.argmin(np.abs(ax[None, :] - x[:, None]), axis=1)
    s_co = p.co_lut[near(p.wspd_dim, wspd), near(p.phi_dim, phi), near(p.inc_dim, inc)] + 0.3 * rng.standard_normal(n)
    dsig = np.where(wspd < 8.0, 2.0, np.where(wspd < 15.0, 0.5, 0.15)) * rng.uniform(0.7, 1.4, n)
    s_cr = p.cr_lut[near(p.wspd_cr, wspd), near(p.inc_cr_dim, inc)] + rng.standard_normal(n) * dsig
    anc = wspd * rng.uniform(0.6, 1.5, n) * np.exp(1j * np.deg2rad(phi + 25.0 * rng.standard_normal(n)))
    cdt = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    return inc.astype(dtype), s_co.astype(dtype), s_cr.astype(dtype), dsig.astype(dtype), anc.astype(cdt)
