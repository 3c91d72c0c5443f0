"""CPU restatement of the inversion cost at the stored grid point (test infrastructure; the executable specification of
k_cost_co / k_cost_cr, include/xsw.h: xsw_cost_from_codes, xsw_cost_cr_from_codes).

The reference forms the dense cost arrays J_co (windspeed/windspeed.py:216-225) and J_cr (:257-264), takes their arg-min and
drops the value.  Here the reference's own expressions are evaluated at the ONE grid point a pixel's code names -- with
numpy array operations, as the reference does (`** 2` of an array is a multiplication; of a numpy scalar it is libm's pow),
on the tables `oracle.invert.Prepared` builds (:144-176) -- so the result is the element the arg-min picked, i.e. J.min().

    co-pol    a grid code: bit 31 clear and flat = code & 0x3FFFFFFF < n_wspd * n_phi -> (i_wspd, i_phi) = divmod(flat, n_phi);
              anything else (XSW_CODE_NAN, XSW_CODE_NAN_RE, a code of another LUT) and a NaN incidence: NaN in every field
    cross-pol searched: code_cr != XSW_CODE_NAN_RE, index = code_cr & 0x3FFFFFFF != XSW_CODE_NO_INDEX and < n_wspd_cr, incidence
              not NaN (XSW_CODE_PICK_CO is ignored); with a co-pol grid code J = Jsig + Jwind (:261), else J = Jsig, Jwind NaN
"""
import numpy as np

from crosspol_codes_ref import CODE_NAN, CODE_NAN_RE, CODE_NO_INDEX  # noqa: F401 (re-exported for the tests)
from oracle import invert as oinv

FIELDS = ("J", "Jsig", "Jwind", "residual")


def tables(lut_co, lut_cr):
    """`oracle.invert.Prepared` of the two dB LUTs (either may be None): the reference's closure state :139-181."""
    return oinv.Prepared(lut_co, lut_cr)


def _flat64(a, shape, dtype=np.float64):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a), shape)).astype(dtype).ravel()


def _nearest(dim, x):
    """np.argmin(np.abs(dim - x)) per pixel (:212, :254); the row of a NaN x is never used."""
    with np.errstate(all="ignore"):
        return np.argmin(np.abs(dim[None, :] - x[:, None]), axis=1)


def _co_grid(code, p):
    """(is a grid code of this LUT, flat index or 0) of uint32 co-pol codes."""
    code = code.astype(np.int64)
    flat = code & 0x3FFFFFFF
    ok = ((code & 0x80000000) == 0) & (flat < p.wspd_dim.size * p.phi_dim.size)
    return ok, np.where(ok, flat, 0)


def cost_co(code_co, inc, s_co_db, anc, dsig_co, p):
    """{J, Jsig, Jwind, residual} float64 of every pixel; sigma0 already in dB; p = tables(lut_co, ...)."""
    shape = np.shape(inc)
    code = np.ascontiguousarray(np.broadcast_to(np.asarray(code_co, dtype=np.uint32), shape)).ravel()
    one_inc, one_sigma0_co_db, one_ancillary_wind = _flat64(inc, shape), _flat64(s_co_db, shape), _flat64(anc, shape, np.complex128)
    grid, flat = _co_grid(code, p)
    ok = grid & ~np.isnan(one_inc)
    lut_idx = (flat // p.phi_dim.size, flat % p.phi_dim.size)
    with np.errstate(all="ignore"):
        i_inc = _nearest(p.inc_dim, one_inc)
        lut_inc = p.co_lut[lut_idx[0], lut_idx[1], i_inc]
        m_antenna, m_azi = np.real(one_ancillary_wind), np.imag(one_ancillary_wind)
        if p.phi_180:
            m_azi = np.abs(m_azi)
        Jwind_co = ((p.lut_co_antenna[lut_idx] - m_antenna) / p.d_antenna) ** 2 + ((p.lut_co_azi[lut_idx] - m_azi) / p.d_azi) ** 2
        Jsig_co = ((lut_inc - one_sigma0_co_db) / dsig_co) ** 2
        J_co = Jwind_co + Jsig_co
        res = lut_inc - one_sigma0_co_db
    return {k: np.where(ok, v, np.nan).reshape(shape) for k, v in zip(FIELDS, (J_co, Jsig_co, Jwind_co, res))}


def cost_cr(code_co, code_cr, inc, s_cr_db, dsig_cr, p):
    """The same for the cross-pol codes; code_co None: every pixel XSW_CODE_NAN; dsig_cr a raster (a scalar already broadcast)."""
    shape = np.shape(inc)
    ccr = np.ascontiguousarray(np.broadcast_to(np.asarray(code_cr, dtype=np.uint32), shape)).ravel().astype(np.int64)
    cco = np.full(ccr.shape, CODE_NAN, np.uint32) if code_co is None else np.ascontiguousarray(np.broadcast_to(np.asarray(code_co, dtype=np.uint32), shape)).ravel()
    one_inc, one_sigma0_cr_db, one_dsig_cr = _flat64(inc, shape), _flat64(s_cr_db, shape), _flat64(dsig_cr, shape)
    icr = ccr & CODE_NO_INDEX
    ok = (ccr != CODE_NAN_RE) & (icr != CODE_NO_INDEX) & (icr < p.wspd_cr.size) & ~np.isnan(one_inc)
    icr = np.where(ok, icr, 0)
    if code_co is None or p.wspd_dim.size == 0:
        have_co, abs_wind_co = np.zeros(ccr.shape, bool), np.full(ccr.shape, np.nan)
    else:
        have_co, flat = _co_grid(cco, p)
        iw, ip = flat // p.phi_dim.size, flat % p.phi_dim.size
        sign = np.where((cco.astype(np.int64) >> 30) & 1, -1.0, 1.0)
        wind_co = p.wspd_dim[iw] * np.exp(1j * np.deg2rad(sign * p.phi_dim[ip]))  # :236-237, the stored solution
        abs_wind_co = np.where(have_co, np.abs(wind_co), np.nan)
    with np.errstate(all="ignore"):
        i_inc = _nearest(p.inc_cr_dim, one_inc)
        lut_cr_inc = p.cr_lut[icr, i_inc]
        Jwind_cr = ((p.wspd_cr[icr] - abs_wind_co) / p.dwspd_fg) ** 2.0
        Jsig_cr = ((lut_cr_inc - one_sigma0_cr_db) / one_dsig_cr) ** 2.0
        J_cr = np.where(have_co, Jsig_cr + Jwind_cr, Jsig_cr)  # :259-264
        res = lut_cr_inc - one_sigma0_cr_db
    return {k: np.where(ok, v, np.nan).reshape(shape) for k, v in zip(FIELDS, (J_cr, Jsig_cr, Jwind_cr, res))}
