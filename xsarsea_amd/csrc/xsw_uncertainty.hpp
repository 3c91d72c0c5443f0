// The WIDTH of the minimum the inversion found, from STORED grid codes (xsw.h: xsw_uncertainty_from_codes,
// xsw_uncertainty_cr_from_codes): the curvature of J_co (windspeed.py:216-225) over the 3 x 3 grid points around the one the
// code names, of J_cr (:257-264) over the 3 around the cross-pol index -- second differences on the LUT axes' own, possibly
// non-uniform, spacings -- inverted to the standard deviations of wind speed and direction and their correlation (posterior
// ~ exp(-J / 2): covariance = 2 H^-1).  The reference drops J after its arg-min and offers nothing of the kind; like the cost
// pass (xsw_cost.hpp) this needs no second search.
//
// One pixel per lane, no LDS, no cross-lane work.  The rasters are read coalesced (float32 rasters: co-pol 4 B code + 4 B
// incidence + 4 B sigma0 + 8 B ancillary wind = 20 B, cross-pol 4 + 4 + 4 + 4 [+ 4 B dsig_cr raster] = 16-20 B).  Co-pol gathers
// three 24-byte runs co[i_inc][iw + k][ip - 1 .. ip + 1], k = -1, 0, 1, whose rows lie phi_pad * 8 bytes apart: three cache
// lines per pixel (four to six when a run straddles a line) where k_cost_co touches one; cross-pol gathers one 24-byte run
// cr[i_inc][icr - 1 .. icr + 1].  Written: 4 or 8 B per requested real output and 1 B of flag.  Every J of a stencil is
// cost_co_at / cost_cr_at (xsw_cost.hpp), the statement k_cost_co / k_cost_cr evaluate, in float64 with -ffp-contract=off: each
// is bit for bit an element of the reference's dense cost array.  The differences, the determinant, the IEEE divisions and
// square roots after them are float64 as well; TO = float is one final rounding.
//
// Flags (XSW_UNC_*, uint8): NO_SOLUTION the code is no grid code of the LUT or the incidence is NaN (k_cost_co's / k_cost_cr's
// rules); WSPD_BORDER / PHI_BORDER the point lies on the first or last index of that axis (no wrap of a 0..360 axis, no mirror
// of a 0..180 one: the folded cost is not symmetric about 0 / 180 deg because of |Im anc|); NOT_CONVEX interior, but not
// (Jww > 0 and Jpp > 0 and det > 0) -- which a NaN sigma0 / ancillary wind / dsig_cr next to a valid code also ends in.  Any
// flag: the real outputs are NaN; for the first three nothing of a LUT is read.  A pixel on a border diverges from its wave's
// interior pixels at ONE branch (it skips the stencil); the outputs nobody asked for are skipped under wave-uniform conditions.
#pragma once
#include "xsw_cost.hpp"  // cost_co_at, cost_cr_at; DevTables, to_db, nearest_index, ld, Cx
#include "xsw_host.hpp"  // UncArgs

namespace xsw {

// second difference of (Jm, J0, Jp) at spacings hm (below) and hp (above)
__device__ __forceinline__ double unc_d2(double Jm, double J0, double Jp, double hm, double hp)
{
    return 2.0 * ((Jp - J0) / hp + (Jm - J0) / hm) / (hp + hm);
}

template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_unc_co(DevTables L, UncArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const CoCode code = co_decode(A.code_co[i], (unsigned)(L.n_w * L.n_phi));
    const double inc = ld<T>(A.inc, i);
    const double s_db = to_db(((const T *)A.s)[i], A.is_db);
    double a, b;
    anc_at<T>(A.anc, i, L.phi_180, a, b);
    unsigned flag = XSW_UNC_NO_SOLUTION;
    double wspd_std = nan, dir_std = nan, corr = nan;
    if (code.grid() && inc == inc) {
        const int iw = (int)(code.flat() / (unsigned)L.n_phi), ip = (int)(code.flat() - (unsigned)iw * (unsigned)L.n_phi);
        flag = ((iw == 0 || iw == L.n_w - 1) ? XSW_UNC_WSPD_BORDER : 0u) | ((ip == 0 || ip == L.n_phi - 1) ? XSW_UNC_PHI_BORDER : 0u);
        if (!flag) {  // 1 <= iw <= n_w - 2 and 1 <= ip <= n_phi - 2: the stencil lies inside the table
            const int i_inc = nearest_index(L.inc, L.n_inc, inc, L.inc_uniform != 0, L.inc0, L.inv_incstep);
            double J[3][3], unused_sig = nan, unused_wind = nan, unused_res;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int l = 0; l < 3; ++l)
                    J[k][l] = cost_co_at(L, i_inc, iw + k - 1, ip + l - 1, s_db, a, b, A.dsig_co, true, true, unused_sig, unused_wind, unused_res);
            const double w0 = L.w[iw], p0 = L.phi[ip];
            const double hwm = w0 - L.w[iw - 1], hwp = L.w[iw + 1] - w0, hpm = p0 - L.phi[ip - 1], hpp = L.phi[ip + 1] - p0;
            const double Jww = unc_d2(J[0][1], J[1][1], J[2][1], hwm, hwp);
            const double Jpp = unc_d2(J[1][0], J[1][1], J[1][2], hpm, hpp);
            const double Jwp = ((J[2][2] - J[2][0]) - (J[0][2] - J[0][0])) / ((hwp + hwm) * (hpp + hpm));
            const double det = Jww * Jpp - Jwp * Jwp;
            if (Jww > 0.0 && Jpp > 0.0 && det > 0.0) {
                if (A.out_wspd_std) wspd_std = sqrt(2.0 * Jpp / det);  // (uniform)
                if (A.out_dir_std) dir_std = sqrt(2.0 * Jww / det);
                if (A.out_corr) corr = -Jwp / sqrt(Jww * Jpp);
            } else {
                flag = XSW_UNC_NOT_CONVEX;
            }
        }
    }
    store_opt<TO>(A.out_wspd_std, i, wspd_std);
    store_opt<TO>(A.out_dir_std, i, dir_std);
    store_opt<TO>(A.out_corr, i, corr);
    if (A.out_flag) ((unsigned char *)A.out_flag)[i] = (unsigned char)flag;
}

// cross-pol: the 1-D analogue on J_cr at icr - 1, icr, icr + 1; have_co / |wind_co| from the co-pol code as in k_cost_cr
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_unc_cr(DevTables L, UncArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const CrCode code_cr = cr_decode(A.code_cr[i]);
    const unsigned icr = code_cr.index();
    const CoCode code = co_decode(A.code_co ? A.code_co[i] : XSW_CODE_NAN, (unsigned)(L.n_w * L.n_phi));
    const double inc = ld<T>(A.inc, i);
    const T x = ((const T *)A.s)[i];
    const double s_db = to_db(x, A.is_db);
    const double dsig = dsig_cr_at<T>(A.dsig_cr, i, x, A.dsig_cr_scalar);
    const bool searched = cr_index_lenient(code_cr, (unsigned)L.n_wcr) && inc == inc;
    unsigned flag = XSW_UNC_NO_SOLUTION;
    double wspd_std = nan;
    if (searched) {
        flag = (icr == 0u || icr == (unsigned)L.n_wcr - 1u) ? XSW_UNC_WSPD_BORDER : 0u;
        if (!flag) {  // 1 <= icr <= n_wcr - 2
            const int i_inc_cr = nearest_index(L.inc_cr, L.n_inc_cr, inc, L.inc_cr_uniform != 0, L.inc_cr0, L.inv_inccrstep);
            double J[3], unused_sig = nan, unused_wind = nan, unused_res;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                J[k] = cost_cr_at(L, i_inc_cr, icr + (unsigned)k - 1u, s_db, dsig, code.grid(), code.flat(), true, true, unused_sig, unused_wind, unused_res);
            const double w0 = L.wcr[icr];
            const double Jww = unc_d2(J[0], J[1], J[2], w0 - L.wcr[icr - 1u], L.wcr[icr + 1u] - w0);
            if (Jww > 0.0) {
                if (A.out_wspd_std) wspd_std = sqrt(2.0 / Jww);  // (uniform)
            } else {
                flag = XSW_UNC_NOT_CONVEX;
            }
        }
    }
    store_opt<TO>(A.out_wspd_std, i, wspd_std);
    if (A.out_flag) ((unsigned char *)A.out_flag)[i] = (unsigned char)flag;
}

}  // namespace xsw
