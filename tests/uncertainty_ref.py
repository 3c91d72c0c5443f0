"""CPU restatement of the wind uncertainty from stored grid codes (test infrastructure; the executable specification of
k_unc_co / k_unc_cr, include/xsw.h: xsw_uncertainty_from_codes, xsw_uncertainty_cr_from_codes).

The cost the inversion minimises is Bayesian, the posterior is ~ exp(-J / 2), so near the minimum the covariance of the
retrieved (wind speed, direction) is 2 H^-1 with H the Hessian of J.  H is taken by second differences over the grid points
around the one a pixel's code names; every J of the stencil is `cost_codes_ref.cost_co` / `cost_cr` on the SHIFTED code, i.e.
the reference's own expression at that grid point (tests/test_uncertainty_cpu.py pins the stencil to the 3 x 3 / 3 block of
the reference's dense J_co / J_cr around its arg-min, bit for bit).  Everything after that is float64 + - * / sqrt in the
order written here.

    flag 1  no solution: no grid code of this LUT / no cross-pol search, or NaN incidence (cost_codes_ref's rules)
    flag 2  the wind-speed index is the first or last of its axis        flag 4  the same for the direction index (co-pol)
    flag 8  interior, but not (Jww > 0 and Jpp > 0 and det > 0)  [cross-pol: not Jww > 0]
    any flag: NaN in the real fields.  No wrap of a 0..360 axis, no mirror of a 0..180 one.
"""
import numpy as np

import cost_codes_ref as cref
from cost_codes_ref import CODE_NAN, CODE_NAN_RE, CODE_NO_INDEX

NO_SOLUTION, WSPD_BORDER, PHI_BORDER, NOT_CONVEX = 1, 2, 4, 8
FIELDS_CO = ("wspd_std", "dir_std", "corr")


def _d2(Jm, J0, Jp, hm, hp):
    """The second difference at spacings hm (below) and hp (above)."""
    return 2.0 * ((Jp - J0) / hp + (Jm - J0) / hm) / (hp + hm)


def _steps(axis, i):
    """(h-, h+) of the axis at the interior indices i (any values where i is not interior: clipped)."""
    n = axis.size
    lo, mid, hi = np.clip(i - 1, 0, n - 1), np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1)
    return axis[mid] - axis[lo], axis[hi] - axis[mid]


def stencil_co(code_co, inc, s_co_db, anc, dsig_co, p):
    """(flag without bit 8, iw, ip, J[n, 3, 3]) of the flattened raster: J[:, k + 1, l + 1] = J_co at (iw + k, ip + l) for the
    pixels whose flag is 0 so far, NaN elsewhere."""
    shape = np.shape(inc)
    code = np.ascontiguousarray(np.broadcast_to(np.asarray(code_co, dtype=np.uint32), shape)).ravel()
    n_w, n_phi = p.wspd_dim.size, p.phi_dim.size
    grid, flat = cref._co_grid(code, p)
    ok = grid & ~np.isnan(np.asarray(inc, dtype=np.float64).ravel())
    iw, ip = flat // max(n_phi, 1), flat % max(n_phi, 1)
    flag = np.where(ok, np.where((iw == 0) | (iw == n_w - 1), WSPD_BORDER, 0) | np.where((ip == 0) | (ip == n_phi - 1), PHI_BORDER, 0), NO_SOLUTION)
    inner = flag == 0
    J = np.full((code.size, 3, 3), np.nan)
    for k in (-1, 0, 1):
        for l in (-1, 0, 1):
            shifted = np.where(inner, (iw + k) * n_phi + (ip + l), CODE_NAN).astype(np.uint32).reshape(shape)
            J[:, k + 1, l + 1] = cref.cost_co(shifted, inc, s_co_db, anc, dsig_co, p)["J"].ravel()
    return flag.astype(np.uint8), iw, ip, J


def unc_co(code_co, inc, s_co_db, anc, dsig_co, p):
    """{wspd_std, dir_std, corr} float64 and flag uint8 of every pixel; sigma0 already in dB; p = cost_codes_ref.tables(...).
    Bit 30 of a code (the -phi choice) does not enter."""
    shape = np.shape(inc)
    flag, iw, ip, J = stencil_co(code_co, inc, s_co_db, anc, dsig_co, p)
    hwm, hwp = _steps(p.wspd_dim, iw)
    hpm, hpp = _steps(p.phi_dim, ip)
    with np.errstate(all="ignore"):
        Jww = _d2(J[:, 0, 1], J[:, 1, 1], J[:, 2, 1], hwm, hwp)
        Jpp = _d2(J[:, 1, 0], J[:, 1, 1], J[:, 1, 2], hpm, hpp)
        Jwp = ((J[:, 2, 2] - J[:, 2, 0]) - (J[:, 0, 2] - J[:, 0, 0])) / ((hwp + hwm) * (hpp + hpm))
        det = Jww * Jpp - Jwp * Jwp
        good = (flag == 0) & (Jww > 0) & (Jpp > 0) & (det > 0)
        flag = np.where((flag == 0) & ~good, NOT_CONVEX, flag).astype(np.uint8)
        out = dict(wspd_std=np.sqrt(2.0 * Jpp / det), dir_std=np.sqrt(2.0 * Jww / det), corr=-Jwp / np.sqrt(Jww * Jpp))
    out = {k: np.where(good, v, np.nan).reshape(shape) for k, v in out.items()}
    out["flag"] = flag.reshape(shape)
    return out


def stencil_cr(code_co, code_cr, inc, s_cr_db, dsig_cr, p):
    """(flag without bit 8, icr, J[n, 3]): J[:, k + 1] = J_cr at icr + k for the pixels whose flag is 0 so far, NaN elsewhere."""
    shape = np.shape(inc)
    ccr = np.ascontiguousarray(np.broadcast_to(np.asarray(code_cr, dtype=np.uint32), shape)).ravel().astype(np.int64)
    n = p.wspd_cr.size
    icr = ccr & CODE_NO_INDEX
    ok = (ccr != CODE_NAN_RE) & (icr != CODE_NO_INDEX) & (icr < n) & ~np.isnan(np.asarray(inc, dtype=np.float64).ravel())
    icr = np.where(ok, icr, 0)
    flag = np.where(ok, np.where((icr == 0) | (icr == n - 1), WSPD_BORDER, 0), NO_SOLUTION)
    inner = flag == 0
    J = np.full((ccr.size, 3), np.nan)
    for k in (-1, 0, 1):
        shifted = np.where(inner, icr + k, CODE_NAN_RE).astype(np.uint32).reshape(shape)
        J[:, k + 1] = cref.cost_cr(code_co, shifted, inc, s_cr_db, dsig_cr, p)["J"].ravel()
    return flag.astype(np.uint8), icr, J


def unc_cr(code_co, code_cr, inc, s_cr_db, dsig_cr, p):
    """{wspd_std float64, flag uint8}; code_co None: every pixel XSW_CODE_NAN; dsig_cr a raster (a scalar already broadcast);
    XSW_CODE_PICK_CO does not enter."""
    shape = np.shape(inc)
    flag, icr, J = stencil_cr(code_co, code_cr, inc, s_cr_db, dsig_cr, p)
    hm, hp = _steps(p.wspd_cr, icr)
    with np.errstate(all="ignore"):
        Jww = _d2(J[:, 0], J[:, 1], J[:, 2], hm, hp)
        good = (flag == 0) & (Jww > 0)
        flag = np.where((flag == 0) & ~good, NOT_CONVEX, flag).astype(np.uint8)
        std = np.sqrt(2.0 / Jww)
    return dict(wspd_std=np.where(good, std, np.nan).reshape(shape), flag=flag.reshape(shape))
