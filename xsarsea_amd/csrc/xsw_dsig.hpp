// dsig_cr on the device (reference: windspeed/utils.py:47-91 `get_dsig`, :18-44 `get_dsig_wspd`): the weight of the cross-pol
// term of the dual-pol cost from the cross-pol signal-to-noise ratio r = sigma0_cr / nesz_cr.
//
//   XSW_DSIG_S1_V2       1 / sqrt(r ** c),  c = d0 + d1 / (1 + exp(-c0 (inc - c1)))   float64 whatever the rasters are
//   XSW_DSIG_RS2_V2      1 / sqrt(r ** 8)                                            in the dtype of r
//   XSW_DSIG_CMODMS1AHW  (1.25 / r) ** 4                                             in the dtype of r
//
// Three HBM-bound streaming kernels:
//   k_dsig       elementwise, r = one IEEE division in the common dtype of sigma0_cr and nesz_cr (numpy's promotion)
//   k_dsig_flat  the same rules on the FLATTENED noise of xsw_nesz_flatten without that raster: the pixel's noise is formed in
//                a register from the line's fit and the column abscissa with k_nesz_eval's own expression (bit-equal to what
//                k_nesz_eval stores), so per pixel only sigma0 (and inc for S1_V2) are read and dsig_cr is written
//   k_dsig_wspd  get_dsig_wspd's product of two logistics, float64.
// Special values follow from IEEE arithmetic as in numpy: r < 0 is NaN under S1_V2 (pow of a negative base) and finite under
// the even powers, r == 0 gives inf, r == inf gives 0, NaN stays NaN; an exp that overflows gives inf and its factor 1/inf = 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xsw.h"
#include "xsw_nesz.hpp"

namespace xsw {

// The rule on a float64 ratio.  Even powers by squaring: three (two) roundings against pow's one, < 2 ulp.
template <int RULE>
__device__ __forceinline__ double dsig_rule(double r, double inc)
{
    if (RULE == XSW_DSIG_S1_V2) {
        const double c = 1.46852088 + 1.4058646 / (1.0 + exp(-1.57952257 * (inc - 25.61843791)));
        return 1.0 / sqrt(pow(r, c));
    }
    if (RULE == XSW_DSIG_RS2_V2) {
        const double r2 = r * r, r4 = r2 * r2;
        return 1.0 / sqrt(r4 * r4);
    }
    const double q = 1.25 / r, q2 = q * q;
    return q2 * q2;
}

// The two float32 rules on a float32 ratio (numpy stays in float32 there: powf, sqrtf, one division).  The power is squared
// in float64 and rounded once -- the correctly rounded float32 power, denormal results included, which float32 squarings are not.
template <int RULE>
__device__ __forceinline__ float dsig_rule_f32(float r)
{
    if (RULE == XSW_DSIG_RS2_V2) {
        const double p = (double)r, p2 = p * p, p4 = p2 * p2;
        return 1.0f / sqrtf((float)(p4 * p4));
    }
    const double q = (double)(1.25f / r), q2 = q * q;
    return (float)(q2 * q2);
}

template <typename T, typename TN, int RULE> struct DsigOut { typedef double type; };
template <> struct DsigOut<float, float, XSW_DSIG_RS2_V2> { typedef float type; };
template <> struct DsigOut<float, float, XSW_DSIG_CMODMS1AHW> { typedef float type; };

template <typename T, typename TN, int RULE>
__device__ __forceinline__ typename DsigOut<T, TN, RULE>::type dsig_pixel(T s, TN nz, T inc)
{
    if constexpr (sizeof(T) == 4 && sizeof(TN) == 4) {
        const float r = s / nz;  // the float32 quotient, also under S1_V2 (which widens it afterwards)
        if constexpr (RULE == XSW_DSIG_S1_V2) return dsig_rule<RULE>((double)r, (double)inc);
        else return dsig_rule_f32<RULE>(r);
    } else {
        return dsig_rule<RULE>((double)s / (double)nz, (double)inc);
    }
}

template <typename T, int N> struct DsigVec { typedef T type __attribute__((ext_vector_type(N))); };

// Elementwise over n pixels, XSW_DSIG_V adjacent pixels per thread (one vector access per raster when every raster is aligned
// to its vector; otherwise -- and for the last, partial group -- element by element).  inc is read by S1_V2 only (else NULL).
#define XSW_DSIG_V 4
template <typename T, typename TN, int RULE>
__global__ __launch_bounds__(256) void k_dsig(const T *__restrict__ sigma0, const TN *__restrict__ nesz, const T *__restrict__ inc,
                                              typename DsigOut<T, TN, RULE>::type *__restrict__ out, long long n)
{
    typedef typename DsigOut<T, TN, RULE>::type TO;
    constexpr int V = XSW_DSIG_V;
    constexpr bool INC = RULE == XSW_DSIG_S1_V2;
    typedef typename DsigVec<T, V>::type vt_t;
    typedef typename DsigVec<TN, V>::type vn_t;
    typedef typename DsigVec<TO, V>::type vo_t;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i >= n) return;
    const bool vec = i + V <= n && (((size_t)sigma0 | (INC ? (size_t)inc : 0)) & (sizeof(vt_t) - 1)) == 0 &&
                     ((size_t)nesz & (sizeof(vn_t) - 1)) == 0 && ((size_t)out & (sizeof(vo_t) - 1)) == 0;
    if (vec) {
        const vt_t s = *(const vt_t *)(sigma0 + i);
        const vn_t z = *(const vn_t *)(nesz + i);
        vt_t a = s;
        if (INC) a = *(const vt_t *)(inc + i);
        vo_t o;
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = dsig_pixel<T, TN, RULE>(s[k], z[k], a[k]);
        *(vo_t *)(out + i) = o;
    } else {
        for (int k = 0; k < V && i + k < n; ++k)
            out[i + k] = dsig_pixel<T, TN, RULE>(sigma0[i + k], nesz[i + k], INC ? inc[i + k] : (T)0);
    }
}

// The fused pass.  Grid and registers as k_nesz_eval: a thread keeps its XSW_NESZ_EV column abscissae and streams down its block
// of lines, the line's (slope, icpt) are wave-uniform.  The flattened noise is k_nesz_eval's expression, copied here letter for
// letter (that kernel is left as it is): for float32 rasters the float32 exp2 widened to float64, for float64 rasters nesz_exp10.
// The rule is then the float64 one -- the flattened noise is float64 in the reference, so r and everything after it is --,
// stored as float64 or rounded once to float32.  XSW_DSIG_FLAT_LINES lines are in flight per lane.
#ifndef XSW_DSIG_FLAT_LINES
#define XSW_DSIG_FLAT_LINES 4
#endif
template <bool F32>
__device__ __forceinline__ double nesz_flat_value(double x, double sl, double ic)
{
    const double t = (x * sl + ic - 1.0) * 0.1;
    return F32 ? (double)__builtin_amdgcn_exp2f((float)(t * 3.321928094887362)) : nesz_exp10(t);
}

template <typename T, typename TO, int RULE>
__global__ __launch_bounds__(256) void k_dsig_flat(const double *__restrict__ col, const double *__restrict__ fit,
                                                   const T *__restrict__ sigma0, const T *__restrict__ inc, TO *__restrict__ out,
                                                   long long lines, long long samples, long long lines_per_block)
{
    constexpr int EV = XSW_NESZ_EV;
    constexpr int U = XSW_DSIG_FLAT_LINES;
    constexpr bool F32 = sizeof(T) == 4;
    constexpr bool INC = RULE == XSW_DSIG_S1_V2;
    static_assert(EV == 2, "the vector accesses below are pairs");
    typedef typename DsigVec<T, EV>::type vt_t;
    typedef typename DsigVec<TO, EV>::type vo_t;
    const long long s = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * EV;
    if (s >= samples) return;
    const long long l0 = (long long)blockIdx.y * lines_per_block;
    const long long l1 = l0 + lines_per_block < lines ? l0 + lines_per_block : lines;
    const double *xs = col + samples;
    double x[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) x[k] = xs[s + k < samples ? s + k : samples - 1];
    const bool vec = s + EV <= samples && (samples & 1) == 0 && (((size_t)sigma0 | (INC ? (size_t)inc : 0)) & (sizeof(vt_t) - 1)) == 0 &&
                     ((size_t)out & (sizeof(vo_t) - 1)) == 0;
    const long long at = l0 * samples + s;
    const T *ps = sigma0 + at, *pi = inc + at;
    TO *o = out + at;
    auto pixel = [&](int k, double sl, double ic, T sv, T iv) {
        const double nz = nesz_flat_value<F32>(x[k], sl, ic);
        return (TO)dsig_rule<RULE>((double)sv / nz, (double)iv);
    };
    if (vec) {
        long long l = l0;
        for (; l + U <= l1; l += U) {
            vt_t a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a[u] = *(const vt_t *)(ps + u * samples);
                b[u] = a[u];
                if (INC) b[u] = *(const vt_t *)(pi + u * samples);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double sl = fit[2 * (l + u)], ic = fit[2 * (l + u) + 1];
                vo_t r;
#pragma unroll
                for (int k = 0; k < EV; ++k) r[k] = pixel(k, sl, ic, a[u][k], b[u][k]);
                *(vo_t *)(o + u * samples) = r;
            }
            ps += U * samples; pi += U * samples; o += U * samples;
        }
        for (; l < l1; ++l, ps += samples, pi += samples, o += samples) {
            const double sl = fit[2 * l], ic = fit[2 * l + 1];
            const vt_t a = *(const vt_t *)ps;
            vt_t b = a;
            if (INC) b = *(const vt_t *)pi;
            vo_t r;
#pragma unroll
            for (int k = 0; k < EV; ++k) r[k] = pixel(k, sl, ic, a[k], b[k]);
            *(vo_t *)o = r;
        }
    } else {
        for (long long l = l0; l < l1; ++l, ps += samples, pi += samples, o += samples) {
            const double sl = fit[2 * l], ic = fit[2 * l + 1];
#pragma unroll
            for (int k = 0; k < EV; ++k)
                if (s + k < samples) o[k] = pixel(k, sl, ic, ps[k], INC ? pi[k] : (T)0);
        }
    }
}

// get_dsig_wspd: clip(1 / (1 + exp(-b (U - (c0 - gamma SNR)))) * 1 / (1 + exp((U - 30) k)), 0, 1); the comparisons of the clip
// are false for NaN, which so passes through as in np.clip.
struct DsigWspdCoef {
    double b, c0, gamma, k;
};
__global__ __launch_bounds__(256) void k_dsig_wspd(const double *__restrict__ U, const double *__restrict__ snr, double *__restrict__ out,
                                                   long long n, DsigWspdCoef q)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double u = U[i];
        const double centre = q.c0 - q.gamma * snr[i];
        const double core = 1.0 / (1.0 + exp(-q.b * (u - centre)));
        const double drop = 1.0 / (1.0 + exp((u - 30.0) * q.k));
        const double v = core * drop;
        out[i] = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    }
}

}  // namespace xsw
