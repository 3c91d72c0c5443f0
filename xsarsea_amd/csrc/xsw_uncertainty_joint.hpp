// The WIDTH of the minimum of the JOINT dual-pol cost, from STORED grid codes (xsw.h: xsw_uncertainty_joint_from_codes; DESIGN.md
// section 20): the curvature of
//     J(iw, ip) = (Jwind_co(iw, ip) + Jsig_co(iw, ip)) + Jsig_cr(iw)
// -- the function xsw_joint_from_codes minimises (xsw_joint.hpp), where k_unc_co (xsw_uncertainty.hpp) takes the curvature of its
// first two terms alone -- over the 3 x 3 grid points around the one the code names, inverted to the standard deviations of wind
// speed and direction and their correlation, and carried on to the (u, v) components the wind is returned in: the standard
// deviations of Re / Im of the complex wind and their correlation, a 2 x 2 change of variables on the same Hessian.
//
// One pixel per lane, no LDS, no cross-lane work, no search.  The rasters are read coalesced (float32 rasters: 4 B code + 4 B
// incidence + 4 B sigma0_co + 8 B ancillary wind + 4 B sigma0_cr [+ 4 B dsig_cr raster] = 24-28 B).  Gathered per pixel: k_unc_co's
// three 24-byte runs co[i_inc][iw + k][ip - 1 .. ip + 1], and for each of the three speed rows the two entries of the cross-pol cell
// that holds w[iw + k] (joint_jsig_cr: with equal steps on the two speed axes neighbouring rows share entries).  Written: 4 or 8 B
// per requested real output and 1 B of flag.  Every J of the stencil is cost_co_at (xsw_cost.hpp) + joint_jsig_cr (xsw_joint.hpp),
// the statements k_joint_from_codes scores its candidates with, in float64 with -ffp-contract=off: each is bit for bit an element
// of the dense joint cost of tests/joint_ref.py.  Everything after the stencil is float64 + - * / sqrt; TO = float is one rounding.
//
// Flags: XSW_UNC_NO_SOLUTION / WSPD_BORDER / PHI_BORDER / NOT_CONVEX are k_unc_co's, tested in its order, and mean NaN in every
// real output; for the first three nothing of any table is read.  XSW_UNC_NO_CROSSPOL marks a pixel whose sigma0_cr or dsig_cr is
// NaN, whatever its other bits: the joint inversion kept the co-pol answer there, the stencil leaves the cross-pol term out, and
// the real outputs are k_unc_co's bit for bit.  It alone does not mean NaN.  A stencil that is not finite (dsig_cr == 0, an
// infinite sigma0_cr, a NaN sigma0_co or ancillary wind, a non-finite table entry) fails the comparisons: NOT_CONVEX.
//
// Every table read stays in bounds: the stencil runs only for 1 <= iw <= n_w - 2 and 1 <= ip <= n_phi - 2, joint_jsig_cr clamps
// the speed into the cross-pol axis and reads the two entries of one of its cells (or entry 0 of a one-entry axis), the incidence
// rows come from nearest_index on their own axes, and the rasters are read and written at i < n only.
#pragma once
#include "xsw_cost.hpp"         // cost_co_at; DevTables, to_db, nearest_index, ld, anc_at, dsig_cr_at, store_opt
#include "xsw_joint.hpp"        // joint_jsig_cr
#include "xsw_uncertainty.hpp"  // unc_d2
#include "xsw_host.hpp"         // UncJointArgs

#ifndef XSW_UNCJ_WAVES
#define XSW_UNCJ_WAVES 7  // waves per SIMD asked for: 68-70 VGPRs, no scratch (8 would cap at 64 VGPRs and spill 12 bytes per lane)
#endif

namespace xsw {

template <typename T, typename TO>
__global__ __launch_bounds__(256, XSW_UNCJ_WAVES) void k_unc_joint(DevTables L, UncJointArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const bool want_uv = A.out_u_std || A.out_v_std || A.out_corr_uv;  // (uniform)
    const CoCode code = co_decode(A.code_co[i], (unsigned)(L.n_w * L.n_phi));
    const double inc = ld<T>(A.inc, i);
    const double s_co = to_db(((const T *)A.s_co)[i], A.is_db);
    const T x_cr = ((const T *)A.s_cr)[i];
    const double s_cr = to_db(x_cr, A.is_db);
    const double dsig = dsig_cr_at<T>(A.dsig_cr, i, x_cr, A.dsig_cr_scalar);
    double a, b;
    anc_at<T>(A.anc, i, L.phi_180, a, b);
    const bool cross = s_cr == s_cr && dsig == dsig;  // (else: no cross-pol information, the co-pol stencil)
    unsigned flag = XSW_UNC_NO_SOLUTION;
    double wspd_std = nan, dir_std = nan, corr = nan, u_std = nan, v_std = nan, corr_uv = nan;
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
                    J[k][l] = cost_co_at(L, i_inc, iw + k - 1, ip + l - 1, s_co, a, b, A.dsig_co, true, true, unused_sig, unused_wind, unused_res);
            if (cross) {
                const int i_inc_cr = nearest_index(L.inc_cr, L.n_inc_cr, inc, L.inc_cr_uniform != 0, L.inc_cr0, L.inv_inccrstep);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double r = joint_jsig_cr(L, i_inc_cr, iw + k - 1, s_cr, dsig);
#pragma unroll
                    for (int l = 0; l < 3; ++l) J[k][l] = J[k][l] + r;  // J_co + Jsig_cr: k_joint_from_codes' association
                }
            }
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
                if (want_uv) {  // covariance 2 H^-1 of (w, direction in degrees), carried to u = w cos, v = w sin of the direction:
                    // the table's phi or, with bit 30, -phi, which turns the sign of sin and of the speed-direction covariance
                    const double Sww = 2.0 * Jpp / det, Spp = 2.0 * Jww / det, Swp = code.sign() ? 2.0 * Jwp / det : -2.0 * Jwp / det;
                    const double c = L.cphi[ip], s = code.sign() ? -L.sphi[ip] : L.sphi[ip];
                    const double r = 0.017453292519943295;
                    const double tu = -(w0 * s) * r, tv = (w0 * c) * r;  // du / dphi, dv / dphi per degree
                    const double var_u = (c * c) * Sww + 2.0 * (c * tu) * Swp + (tu * tu) * Spp;
                    const double var_v = (s * s) * Sww + 2.0 * (s * tv) * Swp + (tv * tv) * Spp;
                    if (A.out_u_std) u_std = sqrt(var_u);
                    if (A.out_v_std) v_std = sqrt(var_v);
                    if (A.out_corr_uv) {
                        const double cov_uv = (c * s) * Sww + (c * tv + s * tu) * Swp + (tu * tv) * Spp;
                        corr_uv = cov_uv / sqrt(var_u * var_v);
                    }
                }
            } else {
                flag = XSW_UNC_NOT_CONVEX;
            }
        }
    }
    store_opt<TO>(A.out_wspd_std, i, wspd_std);
    store_opt<TO>(A.out_dir_std, i, dir_std);
    store_opt<TO>(A.out_corr, i, corr);
    store_opt<TO>(A.out_u_std, i, u_std);
    store_opt<TO>(A.out_v_std, i, v_std);
    store_opt<TO>(A.out_corr_uv, i, corr_uv);
    if (A.out_flag) ((unsigned char *)A.out_flag)[i] = (unsigned char)(flag | (cross ? 0u : XSW_UNC_NO_CROSSPOL));
}

}  // namespace xsw
