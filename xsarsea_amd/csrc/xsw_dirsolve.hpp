// Wind direction at a known speed (xsw.h: xsw_dir_solve): the inverse, along the direction axis, of the table k_lut_eval_co
// evaluates.  Per pixel sigma0 in dB (s), incidence and wind speed are given; the table's column at that incidence and speed is
// d(j) = lerp over speed of the two incidence lerps of co[.][wl][j] and co[.][wh][j], in lerp_axis's two statements -- section 15's
// order, so d(pl), d(ph) are k_lut_eval_co's u0, u1 bit for bit -- and the answer is EVERY direction at which the piecewise linear
// curve through (phi[j], d(j)) takes the value s: all cells are scanned in ascending order, the first two solutions are stored,
// all are counted, and, given a reference direction, the one nearest to it (mirror images included) is selected.  DESIGN.md
// section 18 states the definition once; tests/dirsolve_ref.py restates it in numpy.  IEEE float64 + - * / (and fmod, which is
// exact) only; the file is compiled with -ffp-contract=off, so every output equals the restatement bit for bit.
//
// One pixel per lane, no LDS, no cross-lane work, as k_lut_eval_co: the rasters are read coalesced (float32 rasters: 12 B per
// pixel, 16 B with the reference direction), the lane walks the four rows co[il | ih][wl | wh][0 .. n_phi - 1] from entry 0.  A row
// starts phi_pad * 8 bytes after its predecessor and phi_pad is a multiple of 4, so a row is 32-byte aligned and the walk reads
// node PAIRS as aligned 16-byte loads (unlike section 15's pairs, which start at any entry): the second entry of the last pair of
// an odd n_phi is padding inside the row, read and not used.  The node index is the same in every lane of a wave, so the axis values
// are scalar loads; neighbouring pixels share incidence cells and nearby speed rows, so the rows stay in L2.  Three float64
// divisions per node; the solution's own arithmetic runs only in the cells that hold one.  4 or 8 B are written per requested
// real output, 1 B per uint8 one.
#pragma once
#include "xsw_device.hpp"   // DevTables, ld, store_opt
#include "xsw_forward.hpp"  // cell_hi, lerp_slope, lerp_at, inside
#include "xsw_host.hpp"     // DirArgs

namespace xsw {

// the distance on the circle between candidate c and the reference direction, in [0, 180] (NaN with a NaN among them)
__device__ __forceinline__ double dir_distance(double c, double near)
{
    double r = fmod(c - near, 360.0);
    if (r < 0.0) r = r + 360.0;
    return r > 180.0 ? 360.0 - r : r;
}

// What one pixel has found so far, and the visit of node j with value d: the closest node, then the cell (j - 1, j).
struct DirScan {
    double s, near;
    double prev, p_prev;         // d(j - 1), phi[j - 1]
    double phi1, phi2, sens1, sens2, phi_near, sens_near, best_dist, phi_closest, closest_err;
    int count;
    bool have_closest, fold, want_near;

    __device__ __forceinline__ void candidate(double c, double sens)
    {
        const double dist = dir_distance(c, near);
        if (dist < best_dist) { best_dist = dist; phi_near = c; sens_near = sens; }  // (strict: the earlier one on a tie; never with a NaN)
    }
    __device__ __forceinline__ void visit(int j, int last, double d, double p)
    {
        const double err = fabs(d - s);
        if (fabs(d) <= 1.79769313486231570815e308 && (!have_closest || err < closest_err)) { have_closest = true; closest_err = err; phi_closest = p; }
        if (j > 0) {
            const double a = prev, p0 = p_prev;
            if ((a <= s && s < d) || (a >= s && s > d) || (j == last && s == d && a == a)) {  // (never with a NaN node)
                const double slope = (d - a) / (p - p0);
                double x = d == a ? p0 : p0 + (s - a) / slope;
                x = x < p0 ? p0 : x;
                x = x > p ? p : x;
                const double sens = 1.0 / slope;
                const bool first = count == 0, second = count == 1;  // (selects, not conditional stores: the four stay in registers)
                phi1 = first ? x : phi1; sens1 = first ? sens : sens1;
                phi2 = second ? x : phi2; sens2 = second ? sens : sens2;
                count += 1;
                if (want_near) {
                    candidate(x, sens);
                    if (fold) candidate(-x, -sens);  // the mirror image: sigma0(phi) = sigma0(-phi)
                }
            }
        }
        prev = d;
        p_prev = p;
    }
};

// 4 waves per SIMD asked for, not the 8 of the other raster passes: the scan carries thirteen float64 values per pixel besides the
// four rows in flight and spills at 64 VGPRs.  The pass is bound by its divisions, not by memory latency.
template <typename T, typename TO>
__global__ __launch_bounds__(256, 4) void k_dir_solve_co(DevTables L, DirArgs A)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const double nan = __builtin_nan("");
    const double inc = ld<T>(A.inc, i), s = ld<T>(A.s, i), wspd = ld<T>(A.wspd, i);
    DirScan q;
    q.s = s; q.near = A.near ? ld<T>(A.near, i) : nan;
    q.prev = nan; q.p_prev = nan;
    q.phi1 = nan; q.phi2 = nan; q.sens1 = nan; q.sens2 = nan; q.phi_near = nan; q.sens_near = nan; q.phi_closest = nan;
    q.best_dist = 1e300; q.closest_err = 0.0;
    q.count = 0; q.have_closest = false; q.fold = A.fold_phi != 0; q.want_near = A.near && (A.out_phi_near || A.out_sens_near);
    int flag = XSW_DIR_NAN;
    if (inside(inc, L.inc[0], L.inc[L.n_inc - 1]) && inside(wspd, L.w0, L.w[L.n_w - 1]) && fabs(s) <= 1.79769313486231570815e308) {
        const int ih = cell_hi(L.inc, L.n_inc, inc, L.inc0, L.inv_incstep), il = ih - 1;
        const int wh = cell_hi(L.w, L.n_w, wspd, L.w0, L.inv_wstep), wl = wh - 1;
        const size_t row = (size_t)L.phi_pad, plane = (size_t)L.n_w * row;
        const double *__restrict__ r00 = L.co + (size_t)il * plane + (size_t)wl * row;  // co[il][wl][0]: 32-byte aligned, as the three others
        const double *__restrict__ r10 = r00 + plane, *__restrict__ r01 = r00 + row, *__restrict__ r11 = r01 + plane;  // [ih][wl], [il][wh], [ih][wh]
        const double i0 = L.inc[il], i1 = L.inc[ih], w0 = L.w[wl], w1 = L.w[wh];
        const int n_phi = L.n_phi, last = n_phi - 1;
        double d0 = nan;
#pragma unroll 1
        for (int j = 0; j < n_phi; j += 2) {  // j even and j + 1 < phi_pad (a multiple of 4 >= n_phi): every read is inside its row
            const double2 a = *(const double2 *)(r00 + j), b = *(const double2 *)(r10 + j), c = *(const double2 *)(r01 + j), e = *(const double2 *)(r11 + j);
            const double v0 = lerp_at(lerp_slope(a.x, b.x, i0, i1), inc, i0, a.x), v1 = lerp_at(lerp_slope(c.x, e.x, i0, i1), inc, i0, c.x);
            const double d = lerp_at(lerp_slope(v0, v1, w0, w1), wspd, w0, v0);
            if (j == 0) d0 = d;
            q.visit(j, last, d, L.phi[j]);
            if (j + 1 < n_phi) {
                const double y0 = lerp_at(lerp_slope(a.y, b.y, i0, i1), inc, i0, a.y), y1 = lerp_at(lerp_slope(c.y, e.y, i0, i1), inc, i0, c.y);
                q.visit(j + 1, last, lerp_at(lerp_slope(y0, y1, w0, w1), wspd, w0, y0), L.phi[j + 1]);
            }
        }
        flag = q.count > 2 ? XSW_DIR_MORE : 0;
        if (q.count == 0) flag = s < d0 ? XSW_DIR_BELOW : s > d0 ? XSW_DIR_ABOVE : XSW_DIR_NAN;  // (neither: a NaN in the table)
    }
    store_opt<TO>(A.out_phi1, i, q.phi1);
    store_opt<TO>(A.out_phi2, i, q.phi2);
    store_opt<TO>(A.out_sens1, i, q.sens1);
    store_opt<TO>(A.out_sens2, i, q.sens2);
    store_opt<TO>(A.out_phi_near, i, q.phi_near);
    store_opt<TO>(A.out_sens_near, i, q.sens_near);
    store_opt<TO>(A.out_phi_closest, i, q.phi_closest);
    if (A.out_count) ((unsigned char *)A.out_count)[i] = (unsigned char)min(q.count, 255);
    if (A.out_flag) ((unsigned char *)A.out_flag)[i] = (unsigned char)flag;
}

}  // namespace xsw
