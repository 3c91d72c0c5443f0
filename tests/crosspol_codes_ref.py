"""CPU restatement of the cross-pol step of a dual-pol inversion run from STORED co-pol grid codes (test infrastructure;
the executable specification of k_cross_from_codes / xsw_cross_from_codes).

Restates the reference's windspeed/windspeed.py :252-278 (cross-pol cost, argmin, wind_dual) and :426-428 (the dual-pol
select) literally, per pixel, in numpy; the only thing that differs from `oracle.invert.invert_1d` is where `wind_co` comes
from: not from a co-pol search but from the pixel's co-pol code (include/xsw.h, out_code_co):

    XSW_CODE_NAN_RE   the pixel left at :198-201 / :204-207            -> out_cr = np.nan  (nan + 0j)
    XSW_CODE_NAN      no co-pol search ran (:250)                      -> wind_co = np.nan * 1j
    a grid code       flat = i_wspd * n_phi + i_phi in bits 0..29, bit 30 = the -phi solution (:234-242)
                      -> wind_co = wspd * exp(1j * deg2rad(+-phi)), the value :236-237 / :247 computed
    anything else     (bit 31 set, or flat >= n_wspd * n_phi: a code of another LUT) is handled as XSW_CODE_NAN_RE
"""
import numpy as np

CODE_NAN_RE, CODE_NAN, CODE_PICK_CO, CODE_NO_INDEX = 0xFFFFFFFF, 0xFFFFFFFE, 0x40000000, 0x3FFFFFFF


def tables(lut_co, lut_cr):
    """What the restatement reads of the two dB LUTs (`oracle.lut.Lut`; lut_co may be None for cross-pol-only codes)."""
    t = dict(wspd_cr=np.asarray(lut_cr.wspd, dtype=np.float64), inc_cr_dim=np.asarray(lut_cr.incidence, dtype=np.float64),
             cr_lut=np.ascontiguousarray(np.transpose(lut_cr.values, (1, 0))), n_wspd=0, n_phi=0, sol=None)  # (wspd, incidence) :171-173
    if lut_co is not None:
        wspd, phi = np.asarray(lut_co.wspd, dtype=np.float64), np.asarray(lut_co.phi, dtype=np.float64)
        e = np.stack([np.exp(1j * np.deg2rad(phi)), np.exp(1j * np.deg2rad(-phi))])
        t.update(n_wspd=len(wspd), n_phi=len(phi), sol=wspd[None, :, None] * e[:, None, :])  # [sign][i_wspd][i_phi] :236-237
    return t


def co_codes(idx, wind_co, tab):
    """Co-pol grid codes from an oracle run: idx[..., 0:2] = (i_wspd, i_phi) (-1: no search), wind_co its co-pol output (the sign
    bit: the -phi solution was stored; (nan, 0) marks the early exits :198-207, (nan, nan) no co-pol search :250)."""
    iw, ip = idx[..., 0].astype(np.int64), idx[..., 1].astype(np.int64)
    have = iw >= 0
    flat = np.where(have, iw * tab["n_phi"] + ip, 0)
    code = np.where(np.isnan(wind_co.imag), CODE_NAN, CODE_NAN_RE).astype(np.uint32)
    if have.any():
        plus = tab["sol"][0].reshape(-1)[flat]
        sign = have & (wind_co != plus)
        code = np.where(have, flat | (sign.astype(np.int64) << 30), code).astype(np.uint32)
    return code


def cross_from_codes(code_co, inc, s_cr_db, dsig, tab, dual_select=False):
    """(code_cr uint32, wind_dual complex128) of every pixel; inputs of one shape, s_cr_db already in dB."""
    shape = np.shape(inc)
    code_co = np.broadcast_to(np.asarray(code_co, dtype=np.uint32), shape).ravel()
    inc_1d = np.asarray(inc, dtype=np.float64).ravel()
    s_1d = np.broadcast_to(np.asarray(s_cr_db, dtype=np.float64), shape).ravel()
    dsig_1d = np.broadcast_to(np.asarray(dsig, dtype=np.float64), shape).ravel()
    n = inc_1d.size
    out_cr = np.empty(n, dtype=np.complex128)
    code_cr = np.empty(n, dtype=np.uint32)
    plane = tab["n_wspd"] * tab["n_phi"]
    np_wspd_lut_cr, np_inc_cr_dim, np_sigma0_cr_lut_db = tab["wspd_cr"], tab["inc_cr_dim"], tab["cr_lut"]
    dwspd_fg = 2
    with np.errstate(all="ignore"):
        for i in range(n):
            one_inc, one_sigma0_cr_db, one_dsig_cr = inc_1d[i], s_1d[i], dsig_1d[i]
            c = int(code_co[i])
            flat = c & 0x3FFFFFFF
            grid_code = not (c & 0x80000000) and flat < plane
            if np.isnan(one_inc) or (c != CODE_NAN and not grid_code):  # :198-207 (the ancillary exit is in the code)
                out_cr[i] = np.nan
                code_cr[i] = CODE_NAN_RE
                continue
            wind_co = tab["sol"][(c >> 30) & 1].reshape(-1)[flat] if grid_code else np.nan * 1j  # :247 / :250
            icr = CODE_NO_INDEX
            if not np.isnan(one_sigma0_cr_db) and not np.isnan(one_dsig_cr):  # :252
                i_inc = np.argmin(np.abs(np_inc_cr_dim - one_inc))
                np_sigma0_cr_lut_db_inc = np_sigma0_cr_lut_db[:, i_inc]
                Jwind_cr = ((np_wspd_lut_cr - np.abs(wind_co)) / dwspd_fg) ** 2.0
                Jsig_cr = ((np_sigma0_cr_lut_db_inc - one_sigma0_cr_db) / one_dsig_cr) ** 2.0
                if not np.isnan(np.abs(wind_co)):
                    J_cr = Jsig_cr + Jwind_cr
                else:
                    J_cr = Jsig_cr
                icr = int(np.argmin(J_cr))
                wspd_dual = np_wspd_lut_cr[icr]
                if not np.isnan(np.abs(wind_co)):
                    phi_dual = np.angle(wind_co)
                else:
                    phi_dual = 0
                wind_dual = wspd_dual * np.exp(1j * phi_dual)
            else:
                wind_dual = np.nan * 1j  # :278
            if dual_select and ((np.abs(wind_co) < 5) | (np.abs(wind_dual) < 5)):  # :426-428
                wind_dual = wind_co
                icr |= CODE_PICK_CO
            out_cr[i] = wind_dual
            code_cr[i] = icr
    return code_cr.reshape(shape), out_cr.reshape(shape)
