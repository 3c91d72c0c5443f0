// The forward operator on rasters (xsw.h: xsw_lut_eval, xsw_lut_eval_cr): sigma0 in dB that the context's CURRENT table predicts
// for a wind field, and the derivatives of that interpolant with respect to wind speed and direction.  Per pixel the table is
// interpolated linearly, one axis after the other (incidence, wind speed, direction), in the statements of
// xsarsea_amd/windspeed/lut.py lerp_axis -- slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (x - x_lo) + y_lo -- so sigma0_db is
// bit for bit what LutModel.__call__ gives for that point (IEEE float64 + - * / only; the file is compiled with
// -ffp-contract=off).  DESIGN.md section 15 states the definition once; tests/forward_ref.py restates it in numpy.
//
// One pixel per lane, no LDS, no cross-lane work, as k_cost_co: the rasters are read coalesced (float32 rasters: 4 B incidence +
// 4 B wind speed + 4 B direction = 12 B, cross-pol 8 B), the cell's entries are gathered -- co-pol eight, as four pairs
// co[i][w][p_lo .. p_lo + 1] in two incidence planes n_w * phi_pad * 8 bytes apart; cross-pol four, as two pairs
// cr[i][w_lo .. w_lo + 1] -- the axis values come from the small axis tables, which stay in cache, and 4 B (float32) or 8 B
// (float64) are written per requested output.  A pair starts at any entry of its row, so it is only 8-byte aligned: it is read
// as two 8-byte loads, never as one 16-byte load.
//
// NaN in every output where a coordinate is NaN or lies outside [axis[0], axis[n - 1]] (the direction: after the fold); such a
// pixel reads nothing of the table.
#pragma once
#include "xsw_device.hpp"  // DevTables, ld
#include "xsw_host.hpp"    // FwdArgs

namespace xsw {

// numpy.searchsorted(ax, x) (side left: the first index with ax[k] >= x) clipped to [1, n - 1]: the upper node of the cell that
// lerp_axis interpolates x in; a value equal to node j > 0 takes the cell below it.  The caller has checked ax[0] <= x <= ax[n - 1]
// and n >= 2.  The search starts from the bin a uniform axis would put x in (x0 = ax[0], inv_step = (n - 1) / (ax[n - 1] - ax[0]))
// and moves at most three nodes; what decides is the invariant (k == 0 or ax[k - 1] < x) and ax[k] >= x, and an axis on which
// the computed bin is further off (a non-uniform one) is bisected.  Every read is of ax[0 .. n - 1].  Both parts earn their place:
// the bisection alone is correct everywhere but costs ceil(log2(n)) dependent loads per axis (9 + 9 + 8 on the default table) and
// was measured at twice the time of the whole kernel (9.84 ms against 4.96 ms on 20000 x 20000 pixels);
// the computed bin alone is wrong on a non-uniform axis.
__device__ __forceinline__ int cell_hi(const double *__restrict__ ax, int n, double x, double x0, double inv_step)
{
    const double g = fmin(fmax((x - x0) * inv_step, 0.0), (double)(n - 1));
    int k = (int)ceil(g);  // [0, n - 1]
    bool ok = false;
#pragma unroll 1
    for (int it = 0; it < 3 && !ok; ++it) {
        const double below = ax[max(k - 1, 0)], here = ax[k];
        const bool down = k > 0 && !(below < x), up = k < n - 1 && here < x;
        k += (up ? 1 : 0) - (down ? 1 : 0);
        ok = !up && !down;
    }
    if (!ok) {
        int lo = 0, hi = n - 1;  // x <= ax[n - 1]: the lower bound is at most n - 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ax[mid] < x) lo = mid + 1; else hi = mid;
        }
        k = lo;
    }
    return max(k, 1);
}

// lerp_axis's two statements; `slope` is kept by the callers that differentiate
__device__ __forceinline__ double lerp_slope(double y_lo, double y_hi, double x_lo, double x_hi) { return (y_hi - y_lo) / (x_hi - x_lo); }
__device__ __forceinline__ double lerp_at(double slope, double x, double x_lo, double y_lo) { return slope * (x - x_lo) + y_lo; }

__device__ __forceinline__ bool inside(double x, double first, double last) { return x >= first && x <= last; }  // (false for NaN)

// 1, as a value the compiler cannot see through: a pair's second entry is then no provable neighbour of its first, and the two
// 8-byte loads are not merged into one 16-byte load at an address that is only 8-byte aligned (pairs start at any entry of a row;
// rows are a multiple of 32 bytes apart).  No instruction is emitted.
__device__ __forceinline__ size_t next_entry()
{
    size_t one = 1;
    asm volatile("" : "+v"(one));
    return one;
}

// co-pol: incidence for the four (w, p) corners, then wind speed for the two directions, then direction
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_lut_eval_co(DevTables L, FwdArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const bool want_sp = A.out_db || A.out_dphi, want_dw = A.out_dwspd != nullptr;  // (uniform)
    const double inc = ld<T>(A.inc, i), wspd = ld<T>(A.wspd, i);
    double p = ld<T>(A.phi, i);
    bool reflected = false;
    if (A.fold_phi) {  // sigma0(phi) = sigma0(-phi): a table that ends below the direction takes its mirror image
        p = fmod(p, 360.0);
        if (p < 0.0) p = p + 360.0;
        reflected = p > L.phi_last;
        if (reflected) p = 360.0 - p;
    }
    double db = nan, dwspd = nan, dphi = nan;
    if (inside(inc, L.inc[0], L.inc[L.n_inc - 1]) && inside(wspd, L.w0, L.w[L.n_w - 1]) && inside(p, L.phi0, L.phi_last)) {
        const int ih = cell_hi(L.inc, L.n_inc, inc, L.inc0, L.inv_incstep), il = ih - 1;
        const int wh = cell_hi(L.w, L.n_w, wspd, L.w0, L.inv_wstep), wl = wh - 1;
        const int ph = cell_hi(L.phi, L.n_phi, p, L.phi0, L.inv_dphi), pl = ph - 1;
        const size_t row = (size_t)L.phi_pad, plane = (size_t)L.n_w * row;
        const double *__restrict__ lo = L.co + (size_t)il * plane + (size_t)wl * row + (size_t)pl;  // co[il][wl][pl]
        const double *__restrict__ hi = lo + plane;                                                    // co[ih][wl][pl]
        const size_t nx = next_entry();
        const double i0 = L.inc[il], i1 = L.inc[ih], w0 = L.w[wl], w1 = L.w[wh], p0 = L.phi[pl], p1 = L.phi[ph];
        // v[a][b]: speed node a, direction node b of the cell, at the pixel's incidence
        const double v00 = lerp_at(lerp_slope(lo[0], hi[0], i0, i1), inc, i0, lo[0]);
        const double v01 = lerp_at(lerp_slope(lo[nx], hi[nx], i0, i1), inc, i0, lo[nx]);
        const double v10 = lerp_at(lerp_slope(lo[row], hi[row], i0, i1), inc, i0, lo[row]);
        const double v11 = lerp_at(lerp_slope(lo[row + nx], hi[row + nx], i0, i1), inc, i0, lo[row + nx]);
        const double s0 = lerp_slope(v00, v10, w0, w1), s1 = lerp_slope(v01, v11, w0, w1);
        if (want_sp) {
            const double u0 = lerp_at(s0, wspd, w0, v00), u1 = lerp_at(s1, wspd, w0, v01);
            const double sp = lerp_slope(u0, u1, p0, p1);
            db = lerp_at(sp, p, p0, u0);
            dphi = reflected ? -sp : sp;
        }
        if (want_dw) dwspd = lerp_at(lerp_slope(s0, s1, p0, p1), p, p0, s0);  // the same lerp statement on the two speed slopes
    }
    store_opt<TO>(A.out_db, i, db);
    store_opt<TO>(A.out_dwspd, i, dwspd);
    store_opt<TO>(A.out_dphi, i, dphi);
}

// cross-pol: the 2-D analogue on cr[i][w]: incidence, then wind speed; no direction
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_lut_eval_cr(DevTables L, FwdArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const double inc = ld<T>(A.inc, i), wspd = ld<T>(A.wspd, i);
    double db = nan, dwspd = nan;
    if (inside(inc, L.inc_cr[0], L.inc_cr[L.n_inc_cr - 1]) && inside(wspd, L.wcr0, L.wcr[L.n_wcr - 1])) {
        const int ih = cell_hi(L.inc_cr, L.n_inc_cr, inc, L.inc_cr0, L.inv_inccrstep), il = ih - 1;
        const int wh = cell_hi(L.wcr, L.n_wcr, wspd, L.wcr0, L.inv_wcrstep), wl = wh - 1;
        const double *__restrict__ lo = L.cr + (size_t)il * (size_t)L.wcr_pad + (size_t)wl;  // cr[il][wl]
        const double *__restrict__ hi = lo + (size_t)L.wcr_pad;
        const size_t nx = next_entry();
        const double i0 = L.inc_cr[il], i1 = L.inc_cr[ih], w0 = L.wcr[wl], w1 = L.wcr[wh];
        const double v0 = lerp_at(lerp_slope(lo[0], hi[0], i0, i1), inc, i0, lo[0]);
        const double v1 = lerp_at(lerp_slope(lo[nx], hi[nx], i0, i1), inc, i0, lo[nx]);
        dwspd = lerp_slope(v0, v1, w0, w1);
        db = lerp_at(dwspd, wspd, w0, v0);
    }
    store_opt<TO>(A.out_db, i, db);
    store_opt<TO>(A.out_dwspd, i, dwspd);
}

}  // namespace xsw
