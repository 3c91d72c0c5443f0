// The value of the minimum the inversion found, from STORED grid codes (xsw.h: xsw_cost_from_codes, xsw_cost_cr_from_codes):
// J_co = Jwind_co + Jsig_co (windspeed.py:216-225) and J_cr = Jsig_cr [+ Jwind_cr] (:257-264) at the grid point the code
// names, their two terms, and the forward-model residual lut_db - sigma0_db there.  The reference forms J, takes its arg-min
// and drops the value; the searches here do the same, so this is a pass of its own over the codes -- no second search.
//
// One pixel per lane, no LDS, no cross-lane work: the rasters are read coalesced (float32 rasters: co-pol 4 B code + 4 B
// incidence + 4 B sigma0 + 8 B ancillary wind = 20 B, cross-pol 4 + 4 + 4 + 4 [+ 4 B dsig_cr raster] = 16-20 B), ONE 8-byte LUT
// entry is gathered per pixel (co[i_inc][i_wspd][i_phi], or cr[i_inc][i_wspd_cr]; the axis values w, cphi, sphi, abs_co, wcr are
// small tables that stay in cache), and 8 B (float64) or 4 B (float32) are written per requested output.  All arithmetic is
// float64 in exact_J_co's / exact_J_cr's operation order (xsw_device.hpp; the file is compiled with -ffp-contract=off), so
// J is bit for bit the J.min() of the reference's dense cost array; TO = float is one final rounding.
//
// NaN rules.  Co-pol: a pixel whose code is no grid code of the context's co-pol LUT (XSW_CODE_NAN, XSW_CODE_NAN_RE, bit 31
// set, or a flat index at or beyond n_wspd * n_phi: nothing is read from a table), or whose incidence is NaN, is NaN in all
// four outputs.  Cross-pol: the same for a pixel whose cross-pol code says that no search ran (XSW_CODE_NAN_RE, index
// XSW_CODE_NO_INDEX, an index at or beyond n_wspd_cr) or whose incidence is NaN; XSW_CODE_PICK_CO is ignored (the cost is the
// cross-pol search's, whichever wind the select returned); without a co-pol wind (code_co no grid code) Jwind is NaN and
// J = Jsig.  A NaN sigma0 / ancillary wind / dsig_cr next to a code that names a grid point gives NaN by the arithmetic.
#pragma once
#include "xsw_device.hpp"  // DevTables, to_db, nearest_index, ld, Cx
#include "xsw_host.hpp"    // CostArgs

namespace xsw {

// J_co of windspeed.py:216-225 at grid point (iw, ip) of incidence slice i_inc, with its terms and lut_db - sigma0_db: the ONE
// statement of the co-pol cost from stored codes (k_cost_co: at the code's point; k_unc_co, xsw_uncertainty.hpp: at its nine
// stencil points).  a, b: Re / Im (|Im| for a 0..180 LUT) of the ancillary wind.  A term not wanted stays NaN, and J with it.
__device__ __forceinline__ double cost_co_at(const DevTables &L, int i_inc, int iw, int ip, double s_db, double a, double b, double dsig_co,
                                             bool want_wind, bool want_sig, double &Jsig, double &Jwind, double &res)
{
    const double lutv = L.co[((size_t)i_inc * (size_t)L.n_w + (size_t)iw) * (size_t)L.phi_pad + (size_t)ip];
    res = lutv - s_db;
    if (want_wind) {  // exact_J_co's order
        const double w = L.w[iw];
        const double t1 = (w * L.cphi[ip] - a) * 0.5;
        const double t2 = (w * L.sphi[ip] - b) * 0.5;
        Jwind = t1 * t1 + t2 * t2;
    }
    if (want_sig) {
        const double d = (lutv - s_db) / dsig_co;
        Jsig = d * d;
    }
    return Jwind + Jsig;
}

// J_cr of windspeed.py:257-264 at cross-pol speed index icr of incidence row i_inc_cr, likewise (k_cost_cr; k_unc_cr at its
// three stencil points).  have_co: the co-pol code names grid point `flat` of the co-pol LUT, whose |wind_co| enters Jwind.
__device__ __forceinline__ double cost_cr_at(const DevTables &L, int i_inc_cr, unsigned icr, double s_db, double dsig, bool have_co, unsigned flat,
                                             bool want_wind, bool want_sig, double &Jsig, double &Jwind, double &res)
{
    const double lutv = L.cr[(size_t)i_inc_cr * (size_t)L.wcr_pad + (size_t)icr];
    res = lutv - s_db;
    if (want_sig) {
        const double d = (lutv - s_db) / dsig;
        Jsig = d * d;
    }
    double J = Jsig;
    if (have_co && want_wind) {  // exact_J_cr's order
        const double t = (L.wcr[icr] - L.abs_co[flat]) * 0.5;
        Jwind = t * t;
        J = Jsig + Jwind;
    }
    return J;
}

// co-pol: windspeed.py:212-225 at (i_wspd, i_phi) = (flat / n_phi, flat % n_phi); bit 30 (the -phi choice) does not enter the cost
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_cost_co(DevTables L, CostArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const bool want_wind = A.out_J || A.out_Jwind, want_sig = A.out_J || A.out_Jsig;  // (uniform)
    const CoCode code = co_decode(A.code_co[i], (unsigned)(L.n_w * L.n_phi));
    const double inc = ld<T>(A.inc, i);
    const double s_db = to_db(((const T *)A.s)[i], A.is_db);
    double a = 0.0, b = 0.0;
    if (want_wind) anc_at<T>(A.anc, i, L.phi_180, a, b);
    double J = nan, Jsig = nan, Jwind = nan, res = nan;
    if (code.grid() && inc == inc) {
        const int i_inc = nearest_index(L.inc, L.n_inc, inc, L.inc_uniform != 0, L.inc0, L.inv_incstep);
        const int iw = (int)(code.flat() / (unsigned)L.n_phi), ip = (int)(code.flat() - (unsigned)iw * (unsigned)L.n_phi);
        J = cost_co_at(L, i_inc, iw, ip, s_db, a, b, A.dsig_co, want_wind, want_sig, Jsig, Jwind, res);
    }
    store_opt<TO>(A.out_J, i, J);
    store_opt<TO>(A.out_Jsig, i, Jsig);
    store_opt<TO>(A.out_Jwind, i, Jwind);
    store_opt<TO>(A.out_res, i, res);
}

// cross-pol: windspeed.py:254-264 at i_wspd_cr = the code's index; have_co / |wind_co| from the co-pol code as in k_cross_from_codes
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_cost_cr(DevTables L, CostArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const bool want_wind = A.out_J || A.out_Jwind, want_sig = A.out_J || A.out_Jsig;  // (uniform)
    const CrCode code_cr = cr_decode(A.code_cr[i]);
    const CoCode code = co_decode((A.code_co && want_wind) ? A.code_co[i] : XSW_CODE_NAN, (unsigned)(L.n_w * L.n_phi));
    const double inc = ld<T>(A.inc, i);
    const T x = ((const T *)A.s)[i];
    const double s_db = to_db(x, A.is_db);
    double dsig = nan;
    if (want_sig) dsig = dsig_cr_at<T>(A.dsig_cr, i, x, A.dsig_cr_scalar);
    const bool searched = cr_index_lenient(code_cr, (unsigned)L.n_wcr) && inc == inc;
    double J = nan, Jsig = nan, Jwind = nan, res = nan;
    if (searched) {
        const int i_inc_cr = nearest_index(L.inc_cr, L.n_inc_cr, inc, L.inc_cr_uniform != 0, L.inc_cr0, L.inv_inccrstep);
        J = cost_cr_at(L, i_inc_cr, code_cr.index(), s_db, dsig, code.grid(), code.flat(), want_wind, want_sig, Jsig, Jwind, res);
    }
    store_opt<TO>(A.out_J, i, J);
    store_opt<TO>(A.out_Jsig, i, Jsig);
    store_opt<TO>(A.out_Jwind, i, Jwind);
    store_opt<TO>(A.out_res, i, res);
}

}  // namespace xsw
