// From direction histograms to the inversion's a-priori wind raster: the kernels behind xsarsea_amd.streaks and their C ABI
// (xsw_streaks_peak / xsw_streaks_resolve / xsw_streaks_ancillary, include/xsw.h).  The steps are those of the reference's
// notebook docs/examples/streaks.ipynb (mean of the histograms over pol / downscale_factor / window_size, circ_smooth, peak
// bin), followed by what an operational chain does with the result.
//
//   k_streaks_peak       one wave per window: NaN-skipping mean of the histograms over the leading axes, the four circular
//                        smoothing passes (Bx, Bx2, Bx4, Bx8) in LDS, first arg-max of the NaN-filled result
//   k_streaks_resolve    one thread per window: the 180 degree ambiguity of the unit vector removed against the a-priori wind
//   k_streaks_ancillary  the full-raster pass: per pixel the bilinear blend of the resolved window directions, normalised and
//                        scaled by |a-priori wind|; 16 B read and 16 B written per pixel
//
// Sums are float64 in a fixed order; -ffp-contract=off (xsarsea_amd/_build.py) keeps them free of contractions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "xsw_host.hpp"
#include "xsw_run.hpp"

namespace {

constexpr int PEAK_MIN_ANGLES = 8;
constexpr int PEAK_MAX_ANGLES = 512;  // 8 bins per lane
constexpr int PEAK_WAVES = 4;         // windows per workgroup

// ------------------------------------------------------------------------------------------------------- k_streaks_peak
// weight is [C][nw][n], used_ratio [C][nw]; window w of the workgroup's wave: lane l owns the bins l, l + 64, ...
//   m[a]  = (sum over c, in order, of the non-NaN weight[c][w][a]) / their count          (all NaN: NaN)
//   m     = circ_smooth(m) with `smooth`: out[i] = 0 + B[0] x[i - h] + B[1] x[i - h + 1] + ... (every tap multiplies, the zero
//           ones too, as gradients.circ_smooth's loop does), indices modulo n
//   index = first arg-max of (isnan(m) ? 0 : m), weight_out = m[index], ratio_out = NaN-skipping mean of used_ratio[c][w]
__global__ __launch_bounds__(64 * PEAK_WAVES) void k_streaks_peak(const double *__restrict__ weight, const double *__restrict__ used_ratio,
                                                                  long long C, long long nw, int n, int smooth, int *__restrict__ index,
                                                                  double *__restrict__ weight_out, double *__restrict__ ratio_out)
{
    __shared__ double buf[PEAK_WAVES][2][PEAK_MAX_ANGLES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long win = (long long)blockIdx.x * PEAK_WAVES + wave;
    const bool live = win < nw;
    const long long w = live ? win : nw - 1;  // a wave past the last window recomputes it and stores nothing
    double *x = buf[wave][0], *y = buf[wave][1];
    for (int a = lane; a < n; a += 64) {
        double s = 0.0;
        long long cnt = 0;
        for (long long c = 0; c < C; ++c) {
            const double v = weight[(c * nw + w) * n + a];
            if (!isnan(v)) { s += v; ++cnt; }
        }
        x[a] = cnt ? s / (double)cnt : __builtin_nan("");
    }
    __syncthreads();
    if (smooth) {
        for (int h = 1; h <= 8; h <<= 1) {
            for (int i = lane; i < n; i += 64) {
                double s = 0.0;
                for (int j = 0; j <= 2 * h; ++j) {
                    const double b = (j == 0 || j == 2 * h) ? 0.25 : (j == h ? 0.5 : 0.0);
                    int k = (i + j - h) % n;
                    if (k < 0) k += n;
                    s = s + b * x[k];
                }
                y[i] = s;
            }
            __syncthreads();
            double *t = x;
            x = y;
            y = t;
        }
    }
    constexpr int NONE = 0x7fffffff;
    double bv = 0.0;
    int bi = NONE;
    for (int a = lane; a < n; a += 64) {
        const double m = x[a], f = isnan(m) ? 0.0 : m;
        if (bi == NONE || f > bv) { bv = f; bi = a; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oi != NONE && (bi == NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (live && lane == 0) {
        index[win] = bi;
        weight_out[win] = x[bi];
        double s = 0.0;
        long long cnt = 0;
        for (long long c = 0; c < C; ++c) {
            const double v = used_ratio[c * nw + win];
            if (!isnan(v)) { s += v; ++cnt; }
        }
        ratio_out[win] = cnt ? s / (double)cnt : __builtin_nan("");
    }
}

// ---------------------------------------------------------------------------------------------------- k_streaks_resolve
// d = dirs[w] negated when Re(d conj(a)) = d.x a.x + d.y a.y < 0 (a zero dot product keeps d); NaN + NaN j where d or the
// window's weight is NaN, where a has a NaN part or is 0, or below the thresholds (a NaN threshold is "not given").
__global__ __launch_bounds__(256) void k_streaks_resolve(const double2 *__restrict__ dirs, const double *__restrict__ weight,
                                                         const double *__restrict__ used_ratio, const double2 *__restrict__ anc, long long nw,
                                                         double min_weight, double min_ratio, double2 *__restrict__ out)
{
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    double2 d = dirs[w];
    const double2 a = anc[w];
    const double wt = weight[w], ur = used_ratio[w];
    const bool bad = isnan(d.x) || isnan(d.y) || isnan(wt) || isnan(a.x) || isnan(a.y) || (a.x == 0.0 && a.y == 0.0) || wt < min_weight ||
                     ur < min_ratio;
    const double dot = d.x * a.x + d.y * a.y;
    if (dot < 0.0) d = make_double2(-d.x, -d.y);
    out[w] = bad ? make_double2(__builtin_nan(""), __builtin_nan("")) : d;
}

// -------------------------------------------------------------------------------------------------- k_streaks_ancillary
// The four corner directions of one bracket, NaN corners as zeros: adding w * 0 to a sum that starts at +0 leaves the bits a
// skipped term would (the sum is never -0).
struct Corners {
    double2 c00, c01, c10, c11;
};

__device__ inline double2 corner(const double2 *__restrict__ dirs, int i, int j, int ns)
{
    const double2 d = dirs[(long long)i * ns + j];
    return (isnan(d.x) || isnan(d.y)) ? make_double2(0.0, 0.0) : d;
}

__device__ inline double2 blend(double2 a, const Corners &q, double wl0, double wl1, double ws0, double ws1)
{
    const double w00 = wl0 * ws0, w01 = wl0 * ws1, w10 = wl1 * ws0, w11 = wl1 * ws1;
    double vx = 0.0, vy = 0.0;
    vx += w00 * q.c00.x; vy += w00 * q.c00.y;
    vx += w01 * q.c01.x; vy += w01 * q.c01.y;
    vx += w10 * q.c10.x; vy += w10 * q.c10.y;
    vx += w11 * q.c11.x; vy += w11 * q.c11.y;
    if (isnan(a.x) || isnan(a.y)) return make_double2(__builtin_nan(""), __builtin_nan(""));
    const double nv = hypot(vx, vy);
    if (nv == 0.0) return a;  // no valid corner, or the corners cancel: the model's direction survives
    const double m = hypot(a.x, a.y);
    return make_double2(m * vx / nv, m * vy / nv);
}

#ifndef XSW_STREAKS_LINES
#define XSW_STREAKS_LINES 4
#endif

// grid.x tiles the sample axis (one complex128 pixel per thread: 16-B accesses, 1 KiB per wave instruction), grid.y tiles the
// lines, as k_detrend does.  A thread keeps its column's bracket (first centre, weights) and the four corner directions of
// the current line bracket in registers and streams down its lines: the line bracket is wave-uniform (scalar loads), and
// the corners are fetched again only when it changes.  Per pixel only the a-priori load and the store touch memory.
// li0 / lt (per line) and sj0 / st (per sample): index of the bracket's first centre and the weight t of the second one;
// the second centre is the next one, or the same past the last (where t is 0).
__global__ __launch_bounds__(256) void k_streaks_ancillary(const double2 *__restrict__ anc, double2 *__restrict__ out, long long lines,
                                                           long long samples, const double2 *__restrict__ dirs, int nl, int ns,
                                                           const int *__restrict__ li0, const double *__restrict__ lt,
                                                           const int *__restrict__ sj0, const double *__restrict__ st, long long lines_per_block)
{
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= samples) return;
    const long long l0 = (long long)blockIdx.y * lines_per_block;
    const long long l1 = l0 + lines_per_block < lines ? l0 + lines_per_block : lines;
    const int j0 = min(max(sj0[col], 0), ns - 1), j1 = min(j0 + 1, ns - 1);
    const double ts = st[col], ws0 = 1.0 - ts, ws1 = ts;
    const double2 *in = anc + l0 * samples + col;
    double2 *o = out + l0 * samples + col;
    int cur = -1;
    Corners q;
    for (long long l = l0; l < l1; l += XSW_STREAKS_LINES) {  // several lines in flight per lane
        double2 a[XSW_STREAKS_LINES];
#pragma unroll
        for (int u = 0; u < XSW_STREAKS_LINES; ++u)
            if (l + u < l1) a[u] = in[u * samples];
#pragma unroll
        for (int u = 0; u < XSW_STREAKS_LINES; ++u) {
            if (l + u >= l1) break;
            const int i0 = min(max(li0[l + u], 0), nl - 1);
            const double tl = lt[l + u];
            if (i0 != cur) {
                const int i1 = min(i0 + 1, nl - 1);
                q.c00 = corner(dirs, i0, j0, ns);
                q.c01 = corner(dirs, i0, j1, ns);
                q.c10 = corner(dirs, i1, j0, ns);
                q.c11 = corner(dirs, i1, j1, ns);
                cur = i0;
            }
            o[u * samples] = blend(a[u], q, 1.0 - tl, tl, ws0, ws1);
        }
        in += XSW_STREAKS_LINES * samples;
        o += XSW_STREAKS_LINES * samples;
    }
}

}  // namespace

extern "C" int xsw_streaks_peak(xsw_ctx *c, int64_t n_lead, int64_t n_windows, int32_t n_angles, int32_t mem, int32_t smooth,
                                const double *weight, const double *used_ratio, int32_t *index, double *weight_out, double *used_ratio_out)
{
    if (!c) return XSW_EINVAL;
    if (!weight || !used_ratio || !index || !weight_out || !used_ratio_out || n_lead < 1 || n_windows < 1)
        return fail(c, XSW_EINVAL, "streaks_peak: bad argument");
    if (n_angles < PEAK_MIN_ANGLES || n_angles > PEAK_MAX_ANGLES)
        return fail(c, XSW_EINVAL, "streaks_peak: n_angles must be %d .. %d, not %d", PEAK_MIN_ANGLES, PEAK_MAX_ANGLES, (int)n_angles);
    if (!fits_int(n_windows, n_lead)) return fail(c, XSW_EINVAL, "streaks_peak: too many windows");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const size_t nw = (size_t)n_windows, C = (size_t)n_lead;
    Buf b[5] = {{weight, nullptr, C * nw * n_angles * 8}, {used_ratio, nullptr, C * nw * 8}, {nullptr, index, nw * 4}, {nullptr, weight_out, nw * 8},
                {nullptr, used_ratio_out, nw * 8}};
    const unsigned grid = (unsigned)((nw + PEAK_WAVES - 1) / PEAK_WAVES);
    return run(c, mem, b, [&](Buf (&x)[5]) {
        hipLaunchKernelGGL(k_streaks_peak, dim3(grid), dim3(64 * PEAK_WAVES), 0, c->stream, (const double *)x[0].dev, (const double *)x[1].dev,
                           (long long)n_lead, (long long)n_windows, (int)n_angles, (int)(smooth != 0), (int *)x[2].dev, (double *)x[3].dev,
                           (double *)x[4].dev);
    }, "streaks_peak");
}

extern "C" int xsw_streaks_resolve(xsw_ctx *c, int64_t n_windows, int32_t mem, const double *dirs, const double *weight, const double *used_ratio,
                                   const double *ancillary, double min_weight, double min_used_ratio, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!dirs || !weight || !used_ratio || !ancillary || !out || n_windows < 1) return fail(c, XSW_EINVAL, "streaks_resolve: bad argument");
    if (!fits_int(n_windows)) return fail(c, XSW_EINVAL, "streaks_resolve: too many windows");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const size_t nw = (size_t)n_windows;
    Buf b[5] = {{dirs, nullptr, nw * 16}, {weight, nullptr, nw * 8}, {used_ratio, nullptr, nw * 8}, {ancillary, nullptr, nw * 16}, {nullptr, out, nw * 16}};
    return run(c, mem, b, [&](Buf (&x)[5]) {
        hipLaunchKernelGGL(k_streaks_resolve, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, c->stream, (const double2 *)x[0].dev,
                           (const double *)x[1].dev, (const double *)x[2].dev, (const double2 *)x[3].dev, (long long)n_windows, min_weight,
                           min_used_ratio, (double2 *)x[4].dev);
    }, "streaks_resolve");
}

extern "C" int xsw_streaks_ancillary(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *ancillary, int32_t n_rows,
                                     int32_t n_cols, const double *dirs, const int32_t *line_first, const double *line_t,
                                     const int32_t *sample_first, const double *sample_t, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!ancillary || !dirs || !line_first || !line_t || !sample_first || !sample_t || !out || lines < 1 || samples < 1 || n_rows < 1 || n_cols < 1)
        return fail(c, XSW_EINVAL, "streaks_ancillary: bad argument");
    if (int rc = check_dims(c, "streaks_ancillary", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const size_t npx = (size_t)lines * samples;
    Buf b[7] = {{ancillary, nullptr, npx * 16}, {dirs, nullptr, (size_t)n_rows * n_cols * 16}, {line_first, nullptr, (size_t)lines * 4},
                {line_t, nullptr, (size_t)lines * 8}, {sample_first, nullptr, (size_t)samples * 4}, {sample_t, nullptr, (size_t)samples * 8},
                {nullptr, out, npx * 16}};
    const Strips g = strip_grid(lines, samples);
    const long long lpb = g.rows_per_block;
    return run(c, mem, b, [&](Buf (&x)[7]) {
        hipLaunchKernelGGL(k_streaks_ancillary, dim3((unsigned)g.gx, (unsigned)g.gy), dim3(256), 0, c->stream, (const double2 *)x[0].dev,
                           (double2 *)x[6].dev, (long long)lines, (long long)samples, (const double2 *)x[1].dev, (int)n_rows, (int)n_cols,
                           (const int *)x[2].dev, (const double *)x[3].dev, (const int *)x[4].dev, (const double *)x[5].dev, lpb);
    }, "streaks_ancillary");
}
