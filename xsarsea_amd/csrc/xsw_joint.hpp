// The joint dual-pol inversion from STORED co-pol grid codes (xsw.h: xsw_joint_from_codes): per pixel the grid
// wind (iw, ip) of the co-pol LUT that minimises ONE cost over both observations and the a-priori wind,
//     J(iw, ip) = (Jwind_co(iw, ip) + Jsig_co(iw, ip)) + Jsig_cr(iw),
// the first two terms cost_co_at's statements (xsw_cost.hpp), the third the cross-pol table read at the co-pol speed w[iw]:
// linearly interpolated along the cross-pol speed axis with xsw_forward.hpp's statements, held constant beyond that axis' ends,
// at the nearest cross-pol incidence row.  Ties go to the smallest flat index iw * n_phi + ip: numpy.argmin of the dense array.
// All arithmetic is float64 with IEEE + - * / only (the file is compiled with -ffp-contract=off); tests/joint_ref.py restates it.
//
// Why a window is enough.  Every term is >= 0 and float64 addition is monotone, so with J_ub = J at the input code's own grid
// point a candidate whose Jwind_co exceeds J_ub, or that lies on a speed row with Jsig_cr(iw) > J_ub, scores above J_ub and
// cannot be the arg-min.  box_from_jub (xsw_device.hpp) holds every candidate with Jwind_co <= J_ub; the rows are tested one
// by one.  Inside what survives every candidate is scored with the exact statements: no screening form, no re-scoring, the
// running minimum is lexicographic in (J, flat index).  A pixel admitted to the search has a finite J_ub, hence finite inputs,
// and the tables are finite (the entry refuses others), so no score is NaN.
//
// Work decomposition: 256 threads, each wave owns 64 consecutive pixels.  PER LANE (one pixel each): load, decode, gates, J_ub, the
// window.  The wave then takes its searched pixels one at a time, the pixel's arguments wave-uniform (readlane): the lanes fill
// the wave's LDS array with Jsig_cr of the window's rows (one cell look-up, two table loads, two divisions per row), then
// sweep the window, directions on the lanes, G = 64 / width rows side by side when the window is narrower than the wave; a lane
// skips a row whose LDS entry exceeds its own running minimum (a real candidate's score, so the argument above holds for it).
// A window of more than XSW_JOINT_ROWS rows computes the row term where it is used.  A table with non-uniform axes
// (!L.prunable) has no box: the window is the whole grid.  Every table read lies inside [0, n_w) x [0, n_phi) by the
// window's clamps; the LDS index lies inside [0, XSW_JOINT_ROWS) by the same test that chooses the LDS route.
#pragma once
#include "xsw_device.hpp"   // DevTables, to_db, nearest_index, box_from_jub, wave_argmin, angle_of_quotient, Cx
#include "xsw_host.hpp"     // JointArgs
#include "xsw_cost.hpp"     // cost_co_at
#include "xsw_forward.hpp"  // cell_hi, lerp_slope, lerp_at

#ifndef XSW_JOINT_ROWS
#define XSW_JOINT_ROWS 512  // speed rows of a window whose Jsig_cr is kept in LDS: 4 KB per wave (the default table has 501 rows)
#endif
#ifndef XSW_JOINT_WAVES
#define XSW_JOINT_WAVES 6  // waves per SIMD asked for: 75 VGPRs, no scratch (8 would cap at 64 VGPRs and spill 52 bytes per lane)
#endif

namespace xsw {

// Jsig_cr of co-pol speed row iw (rule 3): the cross-pol table at x = clamp(w[iw], wcr[0], wcr[n_wcr - 1]).
__device__ __forceinline__ double joint_jsig_cr(const DevTables &L, int i_inc_cr, int iw, double s_cr, double dsig)
{
    const double *__restrict__ row = L.cr + (size_t)i_inc_cr * (size_t)L.wcr_pad;
    double crw = row[0];
    if (L.n_wcr >= 2) {
        const double x = fmin(fmax(L.w[iw], L.wcr[0]), L.wcr[L.n_wcr - 1]);
        const int k = cell_hi(L.wcr, L.n_wcr, x, L.wcr0, L.inv_wcrstep);
        crw = lerp_at(lerp_slope(row[k - 1], row[k], L.wcr[k - 1], L.wcr[k]), x, L.wcr[k - 1], row[k - 1]);
    }
    const double d = (crw - s_cr) / dsig;
    return d * d;
}

// The +-phi choice of a 0..180 LUT for grid point (iw, ip): store_pixel's rule (windspeed.py:234-242), restated.  a_im: unfolded.
__device__ __forceinline__ unsigned joint_sign(const DevTables &L, int iw, int ip, double a_re, double a_im)
{
    if (!L.phi_180) return 0u;
    const double w = L.w[iw];
    const double2 e1 = ((const double2 *)L.out_dir)[ip], e2 = ((const double2 *)L.out_dir)[L.n_phi + ip];
    const double s1r = w * e1.x, s1i = w * e1.y + 0.0 * e1.x, s2r = w * e2.x, s2i = w * e2.y + 0.0 * e2.x;
    const double xs = a_im * e1.y, mag = fabs(a_re) + fabs(a_im);
    const bool clear = fabs(xs) > 1e-9 * mag && mag > 1e-100 && mag < 1e100 && w > 1e-100 && w < 1e100 && e2.y == -e1.y && e2.x == e1.x;
    bool second = xs < 0.0;
    if (!clear) {
        const double d1 = angle_of_quotient(a_re, a_im, s1r, s1i);
        const double d2 = angle_of_quotient(a_re, a_im, s2r, s2i);
        second = !(fabs(d1) <= fabs(d2));
    }
    return second ? 1u : 0u;
}

// LDS: 4 waves x XSW_JOINT_ROWS x 8 B = 16 KB per workgroup, ten workgroups per CU: the register budget (XSW_JOINT_WAVES per
// SIMD) decides the occupancy, not the LDS.
template <typename T, typename TO>
__global__ __launch_bounds__(256, XSW_JOINT_WAVES) void k_joint_from_codes(DevTables L, JointArgs A)
{
    __shared__ double rows_lds[4][XSW_JOINT_ROWS];
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const int lane = threadIdx.x & 63;
    double *__restrict__ rl = rows_lds[threadIdx.x >> 6];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i - lane >= A.n) return;  // wave-uniform: the cooperative sweep below needs whole waves
    const bool in = i < A.n;
    const long long il = in ? i : A.n - 1;

    // ---- per lane: load, decode, gates (rule 6), J_ub and the window
    const CoCode code = co_decode(A.code_co[il], (long long)L.n_w * L.n_phi);
    const double inc = ld<T>(A.inc, il);
    const double s_co = to_db(((const T *)A.s_co)[il], A.is_db);
    const T x_cr = ((const T *)A.s_cr)[il];
    const double s_cr = to_db(x_cr, A.is_db);
    const double dsig = dsig_cr_at<T>(A.dsig_cr, il, x_cr, A.dsig_cr_scalar);
    double a, a_im;
    anc_at<T>(A.anc, il, false, a, a_im);
    const double b = L.phi_180 ? fabs(a_im) : a_im;

    unsigned out_code = code.code;  // XSW_CODE_NAN / XSW_CODE_NAN_RE keep their code
    double J = nan, Jwind = nan, Jsig = nan, Jcr = nan, res = nan;
    int i_inc = 0, i_inc_cr = 0, my_flat = 0;
    bool search = false;
    CoWindow W;
    W.w_lo = 0; W.w_hi = L.n_w - 1; W.ip_lo = 0; W.ip_hi = L.n_phi - 1;
    if (!code.nan() && !code.nan_re()) {
        if (!code.grid() || inc != inc) out_code = XSW_CODE_NAN_RE;
        else {
            i_inc = nearest_index(L.inc, L.n_inc, inc, L.inc_uniform != 0, L.inc0, L.inv_incstep);
            my_flat = (int)code.flat();
            const int iw = my_flat / L.n_phi, ip = my_flat - iw * L.n_phi;
            J = cost_co_at(L, i_inc, iw, ip, s_co, a, b, A.dsig_co, true, true, Jsig, Jwind, res);
            if (s_cr == s_cr && dsig == dsig) {  // (else: no cross-pol information: the co-pol answer and its cost)
                i_inc_cr = nearest_index(L.inc_cr, L.n_inc_cr, inc, L.inc_cr_uniform != 0, L.inc_cr0, L.inv_inccrstep);
                Jcr = joint_jsig_cr(L, i_inc_cr, iw, s_cr, dsig);
                J = J + Jcr;  // J_ub
                if (fabs(J) <= 1.7976931348623157e308) {
                    search = in;
                    if (L.prunable) {
                        const double mag = (double)__builtin_sqrtf((float)(a * a + b * b));  // load_pixel's window geometry
                        double th = (double)atan2f((float)b, (float)a) * 57.295779513082320877;
                        if (th < L.phi0) th += 360.0;
                        W = box_from_jub(L, mag, th, J);
                    }
                } else {
                    out_code = XSW_CODE_NAN;
                    J = nan; Jwind = nan; Jsig = nan; Jcr = nan;
                }
            }
        }
    }

    // ---- the wave takes its searched pixels one at a time; every argument of the sweep is wave-uniform
    unsigned long long todo = __ballot(search), ncand = 0;
    const int npx = __popcll(todo);
    while (todo) {
        const int p = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int u_inc = rd_lane_i(i_inc, p), u_inc_cr = rd_lane_i(i_inc_cr, p);
        const double u_sco = rd_lane_d(s_co, p), u_scr = rd_lane_d(s_cr, p), u_dsig = rd_lane_d(dsig, p), u_a = rd_lane_d(a, p), u_b = rd_lane_d(b, p);
        const int w_lo = max(rd_lane_i(W.w_lo, p), 0), w_hi = min(rd_lane_i(W.w_hi, p), L.n_w - 1);
        const int ip_lo = max(rd_lane_i(W.ip_lo, p), 0), ip_hi = min(rd_lane_i(W.ip_hi, p), L.n_phi - 1);
        double bestJ = rd_lane_d(J, p);   // J_ub, the score of a real candidate:
        int bestI = rd_lane_i(my_flat, p);  // the input code's point
        const int nrows = w_hi - w_lo + 1, ncols = ip_hi - ip_lo + 1;
        const bool in_lds = nrows <= XSW_JOINT_ROWS;
        if (in_lds) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the previous pixel's reads are done
            __builtin_amdgcn_wave_barrier();
            for (int r = lane; r < nrows; r += 64) rl[r] = joint_jsig_cr(L, u_inc_cr, w_lo + r, u_scr, u_dsig);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        for (int c0 = 0; c0 < ncols; c0 += 64) {
            const int width = min(64, ncols - c0), G = 64 / width, mdiv = (65536 + width - 1) / width;  // chunk_geom's layout
            const int grp = (lane * mdiv) >> 16, col = lane - grp * width;
            const bool act = grp < G;
            const int ip = ip_lo + c0 + (act ? col : 0);
            for (int row0 = w_lo; row0 <= w_hi; row0 += G) {
                const int iw = min(row0 + grp, w_hi);
                bool ok = act && row0 + grp <= w_hi;
                double r = inf;
                if (in_lds) r = rl[iw - w_lo];
                else if (ok) r = joint_jsig_cr(L, u_inc_cr, iw, u_scr, u_dsig);
                ok = ok && r <= bestJ;
                const unsigned long long live = __ballot(ok);
                if (!live) continue;  // wave-uniform
                ncand += (unsigned long long)__popcll(live);
                if (ok) {
                    double t_sig, t_wind, t_res;
                    const double Jc = cost_co_at(L, u_inc, iw, ip, u_sco, u_a, u_b, A.dsig_co, true, true, t_sig, t_wind, t_res) + r;
                    const int flat = iw * L.n_phi + ip;
                    if (Jc < bestJ || (Jc == bestJ && flat < bestI)) { bestJ = Jc; bestI = flat; }
                }
            }
        }
        wave_argmin(bestJ, bestI);
        if (lane == p) my_flat = bestI;
    }
    if (A.stats && lane == 0 && npx) {  // (vector atomics; xsw_stats_enable)
        atomicAdd(&A.stats[0], (unsigned long long)npx);
        atomicAdd(&A.stats[1], ncand);
    }
    if (!in) return;

    // ---- per lane again: the terms at the joint point, in the statements they were scored with; the -phi choice; the stores
    if (search) {
        const int iw = my_flat / L.n_phi, ip = my_flat - iw * L.n_phi;
        J = cost_co_at(L, i_inc, iw, ip, s_co, a, b, A.dsig_co, true, true, Jsig, Jwind, res);
        Jcr = joint_jsig_cr(L, i_inc_cr, iw, s_cr, dsig);
        J = J + Jcr;
        out_code = co_encode((unsigned)my_flat, joint_sign(L, iw, ip, a, a_im));
    }
    if (A.out_code) A.out_code[i] = out_code;
    store_opt<TO>(A.out_J, i, J);
    store_opt<TO>(A.out_Jwind, i, Jwind);
    store_opt<TO>(A.out_Jsig_co, i, Jsig);
    store_opt<TO>(A.out_Jsig_cr, i, Jcr);
}

}  // namespace xsw
