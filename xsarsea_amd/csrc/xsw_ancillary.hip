// The inversion's a-priori wind raster from a coarse model grid: the kernel behind xsarsea_amd.ancillary and its C ABI
// (xsw_ancillary_model, include/xsw.h).  It is what the reference's notebook docs/examples/windspeed_retrieval_L1.ipynb does by
// hand before the inversion -- speed and meteorological direction of (U10, V10), dir_meteo_to_sample against the ground heading,
// speed * exp(1j * angle) -- in its closed form -(u + 1j v) (cos h + 1j sin h), on the model's own nodes and the scene's
// tie-point grid instead of on rasters resampled elsewhere.
//
//   k_ancillary_model<T>  the full-raster pass: per pixel the scene's longitude, latitude and heading vector from the four tie
//                         points around it, the model wind from the four nodes around that position, rotated into the antenna
//                         frame; nothing read per pixel but the eight nodes (in cache), 16 B written
//
// Sums are float64 in a fixed order; -ffp-contract=off (xsarsea_amd/_build.py) keeps them free of contractions, and the kernel
// calls no trigonometric function (the heading's cosine and sine are the caller's tables): tests/ancillary_model_ref.py
// restates it bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "xsw_host.hpp"
#include "xsw_run.hpp"
#include "xsw_tie.hpp"

namespace {

#ifndef XSW_ANC_LINES
#define XSW_ANC_LINES 4
#endif

// The cell of coordinate x on an axis of n nodes (n >= 2): lower node i, upper node i1, weight t of the upper one.  Periodic: x
// is reduced into [0, n) and node n - 1 is followed by node 0.  Otherwise the pixel is inside iff 0 <= x <= n - 1, the last node
// belongs to cell n - 2 with weight 1, and an outside pixel gets indices that are safe to load from.
struct Cell {
    int i, i1;
    double t;
    bool inside;
};

__device__ inline Cell cell_of(double x, int n, bool periodic)
{
    Cell c;
    if (periodic) {
        const double dn = (double)n;
        double r = x - floor(x / dn) * dn;
        if (!(r >= 0.0) || r >= dn) r = 0.0;  // a rounding's width from a whole number of turns: node 0
        const double f = floor(r);
        c.i = min((int)f, n - 1);
        c.i1 = c.i + 1 == n ? 0 : c.i + 1;
        c.t = r - f;
        c.inside = true;
        return c;
    }
    c.inside = x >= 0.0 && x <= (double)(n - 1);
    const double f = fmin(fmax(floor(x), 0.0), (double)(n - 2));  // NaN -> 0
    c.i = (int)f;
    c.i1 = c.i + 1;
    c.t = x - f;
    return c;
}

// grid.x tiles the sample axis (one complex128 pixel per thread: 16-B stores, 1 KiB per wave instruction), grid.y tiles the lines,
// as k_streaks_ancillary does.  A thread keeps its column's sample bracket and, for the current line bracket, the four tie fields
// already blended along the sample axis at the bracket's two tie lines (eight doubles); the line bracket is wave-uniform (scalar
// loads) and the tie corners are fetched again only when it changes.  Per pixel: the blend along the line axis, one hypot and
// two divisions for the heading vector, the model cell, the eight-node gather and the store.  XSW_ANC_LINES lines are in flight
// per lane: their gathers are issued before the first of them is used.
// li0 / lt (per line) and sj0 / st (per sample): index of the bracket's first tie point and the weight t of the next one; the
// next one is the same past the last (where t is 0).  u, v are [n_lat][n_lon].
template <typename T>
__global__ __launch_bounds__(256) void k_ancillary_model(double2 *__restrict__ out, long long lines, long long samples, const T *__restrict__ u,
                                                         const T *__restrict__ v, int n_lat, int n_lon, double lon0, double dlon, int periodic,
                                                         double lat0, double dlat, int nl, int ns, const double *__restrict__ tlon,
                                                         const double *__restrict__ tlat, const double *__restrict__ tcos,
                                                         const double *__restrict__ tsin, const int *__restrict__ li0,
                                                         const double *__restrict__ lt, const int *__restrict__ sj0,
                                                         const double *__restrict__ st, long long lines_per_block)
{
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= samples) return;
    const long long l0 = (long long)blockIdx.y * lines_per_block;
    const long long l1 = l0 + lines_per_block < lines ? l0 + lines_per_block : lines;
    const int j0 = min(max(sj0[col], 0), ns - 1), j1 = min(j0 + 1, ns - 1);
    const double ts = st[col], ws0 = 1.0 - ts, ws1 = ts;
    double2 *o = out + l0 * samples + col;
    const double nan = __builtin_nan("");
    int cur = -1;
    TieRows q;
    for (long long l = l0; l < l1; l += XSW_ANC_LINES) {
        double ch[XSW_ANC_LINES], sh[XSW_ANC_LINES], tx[XSW_ANC_LINES], ty[XSW_ANC_LINES];
        double u00[XSW_ANC_LINES], u01[XSW_ANC_LINES], u10[XSW_ANC_LINES], u11[XSW_ANC_LINES];
        double v00[XSW_ANC_LINES], v01[XSW_ANC_LINES], v10[XSW_ANC_LINES], v11[XSW_ANC_LINES];
        bool inside[XSW_ANC_LINES];
#pragma unroll
        for (int k = 0; k < XSW_ANC_LINES; ++k) {
            if (l + k >= l1) break;
            const int i0 = min(max(li0[l + k], 0), nl - 1);
            const double tl = lt[l + k], wl0 = 1.0 - tl, wl1 = tl;
            if (i0 != cur) {
                q = tie_rows(tlon, tlat, tcos, tsin, i0, min(i0 + 1, nl - 1), j0, j1, ns, ws0, ws1);
                cur = i0;
            }
            const TiePoint g = tie_point(q, wl0, wl1);  // the headings cancel: ch, sh NaN, the pixel is NaN
            ch[k] = g.ch;
            sh[k] = g.sh;
            const Cell cx = cell_of((g.lon - lon0) / dlon, n_lon, periodic != 0), cy = cell_of((g.lat - lat0) / dlat, n_lat, false);
            inside[k] = cx.inside && cy.inside;
            tx[k] = cx.t;
            ty[k] = cy.t;
            const long long r0 = (long long)cy.i * n_lon, r1 = (long long)cy.i1 * n_lon;
            u00[k] = (double)u[r0 + cx.i]; u01[k] = (double)u[r0 + cx.i1]; u10[k] = (double)u[r1 + cx.i]; u11[k] = (double)u[r1 + cx.i1];
            v00[k] = (double)v[r0 + cx.i]; v01[k] = (double)v[r0 + cx.i1]; v10[k] = (double)v[r1 + cx.i]; v11[k] = (double)v[r1 + cx.i1];
        }
#pragma unroll
        for (int k = 0; k < XSW_ANC_LINES; ++k) {
            if (l + k >= l1) break;
            const double wx0 = 1.0 - tx[k], wx1 = tx[k], wy0 = 1.0 - ty[k], wy1 = ty[k];
            const double uu = wy0 * (wx0 * u00[k] + wx1 * u01[k]) + wy1 * (wx0 * u10[k] + wx1 * u11[k]);
            const double vv = wy0 * (wx0 * v00[k] + wx1 * v01[k]) + wy1 * (wx0 * v10[k] + wx1 * v11[k]);
            const double re = -(uu * ch[k] - vv * sh[k]), im = -(uu * sh[k] + vv * ch[k]);
            o[k * samples] = inside[k] ? make_double2(re, im) : make_double2(nan, nan);
        }
        o += XSW_ANC_LINES * samples;
    }
}

}  // namespace

extern "C" int xsw_ancillary_model(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t dtype, const void *u, const void *v,
                                   int32_t n_lat, int32_t n_lon, double lon0, double dlon, int32_t periodic, double lat0, double dlat,
                                   int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                                   const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                                   const double *sample_t, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!u || !v || !tie_lon || !tie_lat || !tie_cos || !tie_sin || !line_first || !line_t || !sample_first || !sample_t || !out || lines < 1 ||
        samples < 1 || n_tie_lines < 1 || n_tie_samples < 1)
        return fail(c, XSW_EINVAL, "ancillary_model: bad argument");
    if (n_lat < 2 || n_lon < 2) return fail(c, XSW_EINVAL, "ancillary_model: the model grid must have two nodes or more on each axis, not %d x %d", (int)n_lat, (int)n_lon);
    if (!std::isfinite(lon0) || !std::isfinite(lat0) || !std::isfinite(dlon) || !std::isfinite(dlat) || dlon == 0.0 || dlat == 0.0)
        return fail(c, XSW_EINVAL, "ancillary_model: the model axes must have finite origins and finite non-zero steps");
    if (periodic != 0 && periodic != 1) return fail(c, XSW_EINVAL, "ancillary_model: periodic must be 0 or 1");
    if (dtype != XSW_F32 && dtype != XSW_F64) return fail(c, XSW_EINVAL, "ancillary_model: dtype must be XSW_F32 or XSW_F64");
    if (int rc = check_dims(c, "ancillary_model", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const size_t npx = (size_t)lines * samples, nodes = (size_t)n_lat * n_lon * (dtype == XSW_F32 ? 4 : 8), ties = (size_t)n_tie_lines * n_tie_samples * 8;
    Buf b[11] = {{u, nullptr, nodes}, {v, nullptr, nodes}, {tie_lon, nullptr, ties}, {tie_lat, nullptr, ties}, {tie_cos, nullptr, ties},
                 {tie_sin, nullptr, ties}, {line_first, nullptr, (size_t)lines * 4}, {line_t, nullptr, (size_t)lines * 8},
                 {sample_first, nullptr, (size_t)samples * 4}, {sample_t, nullptr, (size_t)samples * 8}, {nullptr, out, npx * 16}};
    const Strips g = strip_grid(lines, samples);
    const long long lpb = g.rows_per_block;
    return run(c, mem, b, [&](Buf (&x)[11]) {
        auto go = [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_ancillary_model<T>, dim3((unsigned)g.gx, (unsigned)g.gy), dim3(256), 0, c->stream, (double2 *)x[10].dev,
                               (long long)lines, (long long)samples, (const T *)x[0].dev, (const T *)x[1].dev, (int)n_lat, (int)n_lon, lon0, dlon,
                               (int)periodic, lat0, dlat, (int)n_tie_lines, (int)n_tie_samples, (const double *)x[2].dev, (const double *)x[3].dev,
                               (const double *)x[4].dev, (const double *)x[5].dev, (const int *)x[6].dev, (const double *)x[7].dev,
                               (const int *)x[8].dev, (const double *)x[9].dev, lpb);
        };
        if (dtype == XSW_F32) go(float{});
        else go(double{});
    }, "ancillary_model");
}
