// The 4-byte grid codes (xsw.h: out_code_co, out_code_cr), stated once: their bits, the two ways of reading each, the one
// way of writing each, and the complex winds a pair of codes stands for.  Plain C++17 for the host compiler and hipcc alike
// (tests/test_host_codes.py builds it alone); DESIGN.md section 16.
//
//   co-pol     bit 31 set: not a grid code (XSW_CODE_NAN_RE = (nan, 0): incidence / ancillary wind NaN; XSW_CODE_NAN =
//              (nan, nan): no search ran; anything else: a code of no LUT).  Bit 30: the -phi choice.  Bits 0..29: the flat
//              index i_wspd * n_phi + i_phi, a grid point of THIS LUT only below plane = n_wspd * n_phi.
//   cross-pol  XSW_CODE_NAN_RE as above.  Bit 30 (XSW_CODE_PICK_CO): the dual select returned the co-pol wind.  Bits 0..29:
//              i_wspd_cr, XSW_CODE_NO_INDEX: no cross-pol search ran.  No producer sets bit 31 otherwise ("foreign").
//
// Table sizes are long long: after inlining each caller's own 32- or 64-bit comparison comes out.
#pragma once
#include "xsw.h"

#ifdef __HIPCC__
#define XSW_HD __host__ __device__
#else
#define XSW_HD
#endif

namespace xsw {

enum : unsigned { CODE_INDEX = XSW_CODE_NO_INDEX /* bits 0..29 */, CODE_NOT_GRID = 0x80000000u /* bit 31 */ };

// A code with its readings; each is evaluated where it is asked for, so a reader pays for what it uses.
struct CoCode {
    unsigned code;
    long long plane;
    XSW_HD bool nan_re() const { return code == XSW_CODE_NAN_RE; }
    XSW_HD bool nan() const { return code == XSW_CODE_NAN; }
    XSW_HD unsigned flat() const { return code & CODE_INDEX; }
    XSW_HD unsigned sign() const { return (code >> 30) & 1u; }
    // the code names a grid point of this LUT
    XSW_HD bool grid() const { return !(code & CODE_NOT_GRID) && (long long)flat() < plane; }
    // [sign][i_wspd][i_phi] of `sol` and `dual_dir`
    XSW_HD long long k() const { return (long long)flat() + (long long)sign() * plane; }
};
XSW_HD inline CoCode co_decode(unsigned code, long long plane) { return CoCode{code, plane}; }
XSW_HD inline unsigned co_encode(unsigned flat, unsigned sign) { return flat | (sign << 30); }

struct CrCode {
    unsigned code;
    XSW_HD bool nan_re() const { return code == XSW_CODE_NAN_RE; }
    XSW_HD bool foreign() const { return (code & CODE_NOT_GRID) && !nan_re(); }
    XSW_HD bool pick_co() const { return (code & XSW_CODE_PICK_CO) != 0; }
    XSW_HD unsigned index() const { return code & CODE_INDEX; }  // XSW_CODE_NO_INDEX: none
};
XSW_HD inline CrCode cr_decode(unsigned code) { return CrCode{code}; }
// index: i_wspd_cr, or XSW_CODE_NO_INDEX for none; pick_co: 0 or 1, as co_encode's sign
XSW_HD inline unsigned cr_encode(unsigned index, unsigned pick_co) { return index | (pick_co ? XSW_CODE_PICK_CO : 0u); }

// "The code holds a cross-pol index of this LUT": TWO rules, which differ on foreign codes alone (0x80000003 is no wind to
// the strict one, index 3 to the lenient one).  No producer writes a foreign cross-pol code, so no result depends on it today;
// each rule keeps the readers it had, and making them one is a change of behaviour left for later.
//   strict: the expansion to winds (expand_cr: k_expand, expand_host)
XSW_HD inline bool cr_index_strict(const CrCode &d, long long n_wcr) { return !d.nan_re() && !d.foreign() && (long long)d.index() < n_wcr; }
//   lenient: the cost and uncertainty passes (k_cost_cr, k_unc_cr)
XSW_HD inline bool cr_index_lenient(const CrCode &d, long long n_wcr)
{
    return !d.nan_re() && d.index() != XSW_CODE_NO_INDEX && (long long)d.index() < n_wcr;
}

// The complex winds a pixel's two codes stand for (xsw_expand_codes), in two halves so that a caller stores the first before it
// reads the second code.  read(table, k) -> Wind is entry k of a [..][2] table: one 16-byte load on the device, two doubles on
// the host.  expand_co: the co-pol wind, from `sol`; returns the grid point it found there, expand_cr's input.
struct Wind { double re, im; };
struct CoPoint { bool have; long long k; };
template <typename Read>
XSW_HD inline CoPoint expand_co(unsigned code, long long plane, const double *sol, Read read, Wind &co)
{
    const double nan = __builtin_nan("");
    const CoCode a = co_decode(code, plane);
    CoPoint p{false, 0};
    co = Wind{nan, nan};  // XSW_CODE_NAN, or not a code of this LUT
    if (a.nan_re()) co.im = 0.0;
    else if (a.grid()) {
        p.k = a.k();
        co = read(sol, p.k);
        p.have = true;
    }
    return p;
}
// expand_cr: the cross-pol wind -- the co-pol one (XSW_CODE_PICK_CO), or wcr[index] along dual_dir in store_pixel's operation order
template <typename Read>
XSW_HD inline Wind expand_cr(unsigned code, const CoPoint &p, const Wind &co, long long n_wcr, const double *dual_dir, const double *wcr, Read read)
{
    const double nan = __builtin_nan("");
    const CrCode b = cr_decode(code);
    Wind cr{nan, nan};
    if (b.nan_re()) cr.im = 0.0;
    else if (b.foreign()) { }
    else if (b.pick_co()) cr = co;
    else if (cr_index_strict(b, n_wcr)) {
        const double wd = wcr[b.index()];
        if (p.have) { const Wind u = read(dual_dir, p.k); cr.re = wd * u.re; cr.im = wd * u.im + 0.0 * u.re; }
        else { cr.re = wd; cr.im = 0.0; }
    }
    return cr;
}

}  // namespace xsw
