// Wind speed at a known direction (xsw.h: xsw_wspd_solve, xsw_wspd_solve_cr): the inverse, along the wind-speed axis, of the table
// k_lut_eval_co / k_lut_eval_cr evaluate.  Per pixel sigma0 in dB (s), incidence and direction are given; the table's column at that
// incidence and direction is c(k) = lerp over direction of the two incidence lerps of co[.][k][.] (cross-pol: the incidence lerp of
// cr[.][k]), in lerp_axis's two statements, and the answer is the LOWEST speed at which the piecewise linear curve through
// (aw[k], c(k)) takes the value s: a bisection over the leading rows, where every column of both incidence slices is
// non-decreasing (DevTables::mono_rows; cross-pol: cr_monotone), then a scan of the rows past them.  DESIGN.md section 17 states
// the definition once; tests/solve_ref.py restates it in numpy.  IEEE float64 + - * / only; the file is compiled with
// -ffp-contract=off, so every output equals the restatement bit for bit.
//
// One pixel per lane, no LDS, no cross-lane work, as k_lut_eval_co: the rasters are read coalesced (float32 rasters: 12 B per
// pixel, cross-pol 8 B), every c(k) gathers two pairs co[i][k][p_lo .. p_lo + 1] in two incidence planes (cross-pol: two entries),
// a pair as two 8-byte loads (next_entry), 4 or 8 B are written per requested real output and 1 B of flag.  The lanes of a wave
// bisect the same range, so their trip counts differ by at most one; the scan past the monotone rows diverges, and only the
// pixels brighter than the top of those rows take it.
#pragma once
#include "xsw_device.hpp"   // DevTables, ld, store_opt
#include "xsw_forward.hpp"  // cell_hi, lerp_slope, lerp_at, inside, next_entry
#include "xsw_host.hpp"     // SolveArgs

namespace xsw {

// c(k) of one pixel: its cell on the incidence axis (and, co-pol, on the direction axis) and the coordinates in it
struct SolveColCo {
    const double *__restrict__ lo;  // co[il][0][pl]; the other incidence plane is `plane` entries on
    size_t row, plane, nx;
    double i0, i1, p0, p1, inc, p;
    __device__ __forceinline__ double operator()(int k) const
    {
        const double *__restrict__ a = lo + (size_t)k * row, *__restrict__ b = a + plane;
        const double u0 = lerp_at(lerp_slope(a[0], b[0], i0, i1), inc, i0, a[0]);
        const double u1 = lerp_at(lerp_slope(a[nx], b[nx], i0, i1), inc, i0, a[nx]);
        return lerp_at(lerp_slope(u0, u1, p0, p1), p, p0, u0);
    }
};
struct SolveColCr {
    const double *__restrict__ lo;  // cr[il][0]; the other incidence row is `pitch` entries on
    size_t pitch;
    double i0, i1, inc;
    __device__ __forceinline__ double operator()(int k) const { return lerp_at(lerp_slope(lo[k], lo[pitch + k], i0, i1), inc, i0, lo[k]); }
};

// The search and the solution for one pixel whose column is `c`: M leading rows are bisected (M < 2: none), the rows from
// max(M - 1, 0) on are scanned.  n_w >= 2.  Every c(k) is of k in [0, n_w - 1].  The bisection keeps the node values it has
// seen at its final bounds, which are the ones the solution needs: c is a pure function of k, so nothing changes but the loads.
// nx: next_entry(), which keeps the two axis values of the cell two 8-byte loads as well.
template <typename Col>
__device__ __forceinline__ void solve_column(const Col &c, const double *__restrict__ aw, size_t nx, int n_w, int M, double s, double &w,
                                             double &sens, int &flag)
{
    int k = -1;
    double ck = 0.0, ck1 = 0.0;
    if (M >= 2) {
        int lo = 0, hi = M - 1;
        double below = 0.0, at_hi = 0.0;  // c(lo - 1) once lo has moved, c(hi) once hi has
        bool hi_seen = false;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const double v = c(mid);
            if (v < s) { lo = mid + 1; below = v; }
            else { hi = mid; at_hi = v; hi_seen = true; }
        }
        const double cj = hi_seen ? at_hi : c(lo);
        if (cj >= s && lo > 0) { k = lo - 1; ck = below; ck1 = cj; }
        else if (lo == 0 && cj == s) { k = 0; ck = cj; ck1 = c(1); }
    }
    if (k < 0) {
        int q = max(M - 1, 0);
        double a = c(q);
#pragma unroll 1
        for (; q < n_w - 1; ++q) {
            const double b = c(q + 1);
            if ((a <= s && s <= b) || (b <= s && s <= a)) { k = q; ck = a; ck1 = b; flag = XSW_SOLVE_TAIL; break; }  // min <= s <= max; never with a NaN
            a = b;
        }
    }
    if (k < 0) {
        const double c0 = c(0);
        flag = s < c0 ? XSW_SOLVE_BELOW : s > c0 ? XSW_SOLVE_ABOVE : XSW_SOLVE_NAN;  // (neither: a NaN in the table)
        return;
    }
    const double w0 = aw[k], w1 = aw[(size_t)k + nx];
    const double slope = (ck1 - ck) / (w1 - w0);
    double x = ck1 == ck ? w0 : w0 + (s - ck) / slope;
    x = x < w0 ? w0 : x;
    x = x > w1 ? w1 : x;
    w = x;
    sens = 1.0 / slope;
}

template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_wspd_solve_co(DevTables L, SolveArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const double inc = ld<T>(A.inc, i), s = ld<T>(A.s, i);
    double p = ld<T>(A.phi, i);
    if (A.fold_phi) {  // as k_lut_eval_co
        p = fmod(p, 360.0);
        if (p < 0.0) p = p + 360.0;
        if (p > L.phi_last) p = 360.0 - p;
    }
    double w = nan, sens = nan;
    int flag = XSW_SOLVE_NAN;
    if (inside(inc, L.inc[0], L.inc[L.n_inc - 1]) && inside(p, L.phi0, L.phi_last) && fabs(s) <= 1.79769313486231570815e308) {
        const int ih = cell_hi(L.inc, L.n_inc, inc, L.inc0, L.inv_incstep), il = ih - 1;
        const int ph = cell_hi(L.phi, L.n_phi, p, L.phi0, L.inv_dphi), pl = ph - 1;
        SolveColCo c;
        c.row = (size_t)L.phi_pad; c.plane = (size_t)L.n_w * c.row; c.nx = next_entry();
        c.lo = L.co + (size_t)il * c.plane + (size_t)pl;
        c.i0 = L.inc[il]; c.i1 = L.inc[ih]; c.p0 = L.phi[pl]; c.p1 = L.phi[ph]; c.inc = inc; c.p = p;
        flag = 0;
        solve_column(c, L.w, c.nx, L.n_w, min(L.mono_rows[il], L.mono_rows[ih]), s, w, sens, flag);
    }
    store_opt<TO>(A.out_wspd, i, w);
    store_opt<TO>(A.out_sens, i, sens);
    if (A.out_flag) ((unsigned char *)A.out_flag)[i] = (unsigned char)flag;
}

// cross-pol: the 1-D inversion of cr[i][w] at the pixel's incidence; all rows are bisected when every row of the table rises
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_wspd_solve_cr(DevTables L, SolveArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const double inc = ld<T>(A.inc, i), s = ld<T>(A.s, i);
    double w = nan, sens = nan;
    int flag = XSW_SOLVE_NAN;
    if (inside(inc, L.inc_cr[0], L.inc_cr[L.n_inc_cr - 1]) && fabs(s) <= 1.79769313486231570815e308) {
        const int ih = cell_hi(L.inc_cr, L.n_inc_cr, inc, L.inc_cr0, L.inv_inccrstep), il = ih - 1;
        SolveColCr c;
        c.pitch = (size_t)L.wcr_pad;
        c.lo = L.cr + (size_t)il * c.pitch;
        c.i0 = L.inc_cr[il]; c.i1 = L.inc_cr[ih]; c.inc = inc;
        flag = 0;
        solve_column(c, L.wcr, next_entry(), L.n_wcr, L.cr_monotone ? L.n_wcr : 0, s, w, sens, flag);
    }
    store_opt<TO>(A.out_wspd, i, w);
    store_opt<TO>(A.out_sens, i, sens);
    if (A.out_flag) ((unsigned char *)A.out_flag)[i] = (unsigned char)flag;
}

}  // namespace xsw
