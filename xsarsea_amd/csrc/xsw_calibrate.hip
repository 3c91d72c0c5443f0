// Calibration of a product's digital numbers: the kernel behind xsarsea_amd.calibrate and its C ABI (xsw_calibrate,
// include/xsw.h).  sigma0 = (DN^2 - N) / A^2 and nesz = N / A^2 with A the sigma0 calibration LUT and N the noise LUT, the incidence
// angle from the geolocation grid and a validity mask, all from 2-byte digital numbers and a few kilobytes of annotation.
//
//   k_calibrate<DN, OUT, VEC, TABS>  one streaming pass: a thread owns four consecutive samples of a strip of lines; 2 B (uint16)
//                                    or 4 B (float32) read per pixel, 4 B or 8 B written per float raster, 1 B for the mask;
//                                    the annotation tables and their brackets stay in cache
//
// Every operation is float64 in the order include/xsw.h states; -ffp-contract=off (xsarsea_amd/_build.py) keeps it free of
// contractions, the one division per pixel is IEEE, and no library function is called: tests/calibrate_ref.py restates the
// kernel in numpy bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "xsw_host.hpp"
#include "xsw_run.hpp"

namespace {

#ifndef XSW_CAL_LINES
#define XSW_CAL_LINES 4  // lines in flight per lane: their digital numbers are loaded before the first of them is used
#endif
#ifndef XSW_CAL_MIN_LINES
#define XSW_CAL_MIN_LINES 32  // a workgroup's strip is at least this many lines long: the per-thread table state is set up once per strip
#endif

enum : int { TAB_CAL = 1, TAB_RANGE = 2, TAB_AZIMUTH = 4, TAB_INC = 8 };  // k_calibrate's TABS: dn with the sigma0 LUT, the two noise tables, incidence

// One annotation table on the device: f [nl][ns], li0 / lt per raster line, sj0 / st per raster sample (xsw_table).
struct Tab {
    const double *f;
    const int *li0;
    const double *lt;
    const int *sj0;
    const double *st;
    int nl, ns;
};

struct CalArgs {
    Tab lut, range, azimuth, inc;
    long long lines, samples, lines_per_block;
    int use_fill;
    unsigned fill_u16;
    float fill_f32;
};

// One table at a thread's four columns: their sample brackets and, for the line bracket `cur`, the table blended along the
// sample axis at the bracket's two node lines (TieRows of xsw_tie.hpp, four columns wide).
struct Cols {
    unsigned j0[4];  // (clamped into the table before it is kept)
    double t[4], r0[4], r1[4];
    int cur;
};

// s: the thread's first sample; columns past the raster (the last quad of the element-wise path) read the last sample's bracket.
__device__ inline void cols_init(Cols &c, const Tab &T, long long s, long long samples)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long sk = s + k < samples ? s + k : samples - 1;
        c.j0[k] = (unsigned)min(max(T.sj0[sk], 0), T.ns - 1);
        c.t[k] = T.st[sk];
    }
    c.cur = -1;
}

// x, as a value the compiler knows nothing about: what is derived from it is computed where it is used.  Without it the second
// column index and the first weight of every bracket are hoisted out of the line loop and held in registers for its whole run
// (20 more per table), for a blend that runs only when a line bracket changes.
template <typename V>
__device__ inline V opaque(V x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// The table at raster line l for the four columns.  The line bracket is wave-uniform (scalar loads); the rows are blended again
// only when it changes.
__device__ inline void cols_at(Cols &c, const Tab &T, long long l, double (&out)[4])
{
    const int i0 = min(max(T.li0[l], 0), T.nl - 1);
    const double tl = T.lt[l], wl0 = 1.0 - tl, wl1 = tl;
    if (i0 != c.cur) {
        const double *f0 = T.f + (long long)i0 * T.ns, *f1 = T.f + (long long)min(i0 + 1, T.nl - 1) * T.ns;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned j0 = opaque(c.j0[k]), j1 = min(j0 + 1u, (unsigned)T.ns - 1u);
            const double ws1 = opaque(c.t[k]), ws0 = 1.0 - ws1;
            c.r0[k] = ws0 * f0[j0] + ws1 * f0[j1];
            c.r1[k] = ws0 * f1[j0] + ws1 * f1[j1];
            __builtin_amdgcn_sched_barrier(0);  // one column's four nodes at a time: a bracket changes rarely, its registers are needed always
        }
        c.cur = i0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = wl0 * c.r0[k] + wl1 * c.r1[k];
}

// Four consecutive digital numbers from p: one 8-byte (uint16) or 16-byte (float32) load, or, element-wise, the n <= 4 that exist.
template <typename DN, bool VEC>
__device__ inline void load4(DN (&d)[4], const DN *__restrict__ p, long long n)
{
    if constexpr (VEC) {
        using V = std::conditional_t<std::is_same_v<DN, float>, float4, ushort4>;
        const V v = *reinterpret_cast<const V *>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = k < n ? p[k] : DN(0);
    }
}

// Four consecutive values, rounded once to OUT: 16-byte stores (one for float32, two for float64), or element-wise.
template <typename OUT, bool VEC>
__device__ inline void store4(OUT *__restrict__ p, const double (&x)[4], long long n)
{
    if constexpr (VEC && std::is_same_v<OUT, float>) {
        *reinterpret_cast<float4 *>(p) = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
    } else if constexpr (VEC) {
        reinterpret_cast<double2 *>(p)[0] = make_double2(x[0], x[1]);
        reinterpret_cast<double2 *>(p)[1] = make_double2(x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = (OUT)x[k];
    }
}

// grid.x tiles the quads of samples (256 threads: 1024 samples per workgroup), grid.y the strips of lines.  A thread keeps, per
// table that is there (TABS: an absent table is no code and no register), the state of `Cols`; XSW_CAL_LINES lines are in flight:
// their digital numbers are loaded before the first of them is used.  VEC: samples is a multiple of four and every raster is
// aligned to its access, so a thread's four samples are one load and one store per raster; otherwise every access is
// element-wise and the row's last quad may be partial.  Output pointers that are null are skipped (uniform branches).
template <typename DN, typename OUT, bool VEC, int TABS>
__global__ __launch_bounds__(256) void k_calibrate(const DN *__restrict__ dn, OUT *__restrict__ o_s0, OUT *__restrict__ o_nz, OUT *__restrict__ o_inc,
                                                   unsigned char *__restrict__ o_valid, const CalArgs a)
{
    constexpr bool CAL = TABS & TAB_CAL, NR = TABS & TAB_RANGE, NA = TABS & TAB_AZIMUTH, INC = TABS & TAB_INC;
    const long long s = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (s >= a.samples) return;
    const long long n = a.samples - s;  // samples from s to the end of the row (>= 4 on the vector path)
    const long long l0 = (long long)blockIdx.y * a.lines_per_block;
    const long long l1 = l0 + a.lines_per_block < a.lines ? l0 + a.lines_per_block : a.lines;
    Cols cA, cR, cZ, cI;
    if constexpr (CAL) cols_init(cA, a.lut, s, a.samples);
    if constexpr (NR) cols_init(cR, a.range, s, a.samples);
    if constexpr (NA) cols_init(cZ, a.azimuth, s, a.samples);
    if constexpr (INC) cols_init(cI, a.inc, s, a.samples);
    const double nan = __builtin_nan("");
    for (long long l = l0; l < l1; l += XSW_CAL_LINES) {
        DN d[XSW_CAL_LINES][4];
        if constexpr (CAL) {
#pragma unroll
            for (int k = 0; k < XSW_CAL_LINES; ++k) {
                if (l + k >= l1) break;
                load4<DN, VEC>(d[k], dn + (l + k) * a.samples + s, n);
            }
        }
#pragma unroll
        for (int k = 0; k < XSW_CAL_LINES; ++k) {
            if (l + k >= l1) break;
            const long long at = (l + k) * a.samples + s;
            if constexpr (INC) {
                double inc[4];
                cols_at(cI, a.inc, l + k, inc);
                store4<OUT, VEC>(o_inc + at, inc, n);
            }
            if constexpr (CAL) {
                double A[4], N[4], s0[4], nz[4];
                cols_at(cA, a.lut, l + k, A);
                if constexpr (NR) cols_at(cR, a.range, l + k, N);
                if constexpr (NA) {
                    double na[4];
                    cols_at(cZ, a.azimuth, l + k, na);
#pragma unroll
                    for (int j = 0; j < 4; ++j) N[j] = NR ? N[j] * na[j] : na[j];
                }
                unsigned ok = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (!NR && !NA) N[j] = 0.0;
                    const double dd = (double)d[k][j], q = dd * dd, g = 1.0 / (A[j] * A[j]);
                    nz[j] = N[j] * g;
                    s0[j] = (q - N[j]) * g;
                    bool fill;
                    if constexpr (std::is_same_v<DN, float>) fill = a.use_fill && d[k][j] == a.fill_f32;
                    else fill = a.use_fill && (unsigned)d[k][j] == a.fill_u16;
                    if (fill) s0[j] = nan;
                    ok |= (unsigned)(s0[j] > 0.0) << (8 * j);  // (NaN > 0 is false: a fill pixel is never valid)
                }
                if (o_s0) store4<OUT, VEC>(o_s0 + at, s0, n);
                if (o_nz) store4<OUT, VEC>(o_nz + at, nz, n);
                if (o_valid) {
                    if constexpr (VEC) {
                        *reinterpret_cast<unsigned *>(o_valid + at) = ok;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < n) o_valid[at + j] = (unsigned char)(ok >> (8 * j));
                    }
                }
            }
        }
    }
}

bool present(const xsw_table *t) { return t && t->values; }

// nullptr, or what is wrong with a table that is there.
const char *table_fault(const xsw_table *t)
{
    if (!present(t)) return nullptr;
    if (t->n_lines < 1 || t->n_samples < 1) return "has an empty axis";
    if (!t->line_first || !t->line_t || !t->sample_first || !t->sample_t) return "lacks a bracket";
    return nullptr;
}

bool aligned(const void *p, size_t to) { return ((uintptr_t)p % to) == 0; }

}  // namespace

extern "C" int xsw_calibrate(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t dn_dtype, int32_t out_dtype, const void *dn,
                             const xsw_table *sigma0_lut, const xsw_table *noise_range, const xsw_table *noise_azimuth,
                             const xsw_table *incidence, int32_t use_fill, double fill, void *out_sigma0, void *out_nesz, void *out_incidence,
                             uint8_t *out_valid)
{
    if (!c) return XSW_EINVAL;
    if (lines < 1 || samples < 1) return fail(c, XSW_EINVAL, "calibrate: bad argument");
    const xsw_table *tabs[4] = {sigma0_lut, noise_range, noise_azimuth, incidence};
    static const char *const names[4] = {"sigma0_lut", "noise_range", "noise_azimuth", "incidence"};
    for (int k = 0; k < 4; ++k)
        if (const char *why = table_fault(tabs[k])) return fail(c, XSW_EINVAL, "calibrate: table %s %s", names[k], why);
    if (out_dtype != XSW_F32 && out_dtype != XSW_F64) return fail(c, XSW_EINVAL, "calibrate: out_dtype must be XSW_F32 or XSW_F64");
    if (!dn) {
        if (!present(incidence) || present(sigma0_lut) || present(noise_range) || present(noise_azimuth) || !out_incidence || out_sigma0 ||
            out_nesz || out_valid)
            return fail(c, XSW_EINVAL, "calibrate: without dn only the incidence table and out_incidence may be given");
    } else {
        if (dn_dtype != XSW_DN_U16 && dn_dtype != XSW_DN_F32) return fail(c, XSW_EINVAL, "calibrate: dn_dtype must be XSW_DN_U16 or XSW_DN_F32");
        if (!present(sigma0_lut)) return fail(c, XSW_EINVAL, "calibrate: dn needs the sigma0_lut table");
        if (out_incidence && !present(incidence)) return fail(c, XSW_EINVAL, "calibrate: out_incidence needs the incidence table");
        if (!out_sigma0 && !out_nesz && !out_incidence && !out_valid) return fail(c, XSW_EINVAL, "calibrate: no output");
        if (use_fill != 0 && use_fill != 1) return fail(c, XSW_EINVAL, "calibrate: use_fill must be 0 or 1");
        if (use_fill && dn_dtype == XSW_DN_U16 && !(fill >= 0.0 && fill <= 65535.0 && fill == std::floor(fill)))
            return fail(c, XSW_EINVAL, "calibrate: a uint16 fill must be a whole number in 0 .. 65535");
    }
    if (int rc = check_dims(c, "calibrate", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const bool f32_dn = dn && dn_dtype == XSW_DN_F32, f64_out = out_dtype == XSW_F64;
    const size_t npx = (size_t)lines * samples, es = f32_dn ? 4 : 2, os = f64_out ? 8 : 4;
    int mask = dn ? TAB_CAL : 0;
    if (dn && present(noise_range)) mask |= TAB_RANGE;
    if (dn && present(noise_azimuth)) mask |= TAB_AZIMUTH;
    if (out_incidence) mask |= TAB_INC;
    // [0] dn, [1 + 5 k ..] table k: values and its four brackets (a table the pass does not read travels nowhere), [21..24] outputs
    Buf b[25] = {in_buf(dn, npx * es)};
    for (int k = 0; k < 4; ++k) {
        const xsw_table *t = (mask & (1 << k)) ? tabs[k] : nullptr;
        b[1 + 5 * k] = in_buf(t ? t->values : nullptr, t ? (size_t)t->n_lines * t->n_samples * 8 : 0);
        b[2 + 5 * k] = in_buf(t ? t->line_first : nullptr, (size_t)lines * 4);
        b[3 + 5 * k] = in_buf(t ? t->line_t : nullptr, (size_t)lines * 8);
        b[4 + 5 * k] = in_buf(t ? t->sample_first : nullptr, (size_t)samples * 4);
        b[5 + 5 * k] = in_buf(t ? t->sample_t : nullptr, (size_t)samples * 8);
    }
    b[21] = out_buf(out_sigma0, npx * os);
    b[22] = out_buf(out_nesz, npx * os);
    b[23] = out_buf(out_incidence, npx * os);
    b[24] = out_buf(out_valid, npx);
    const long long quads = ((long long)samples + 3) / 4;
    const Strips g = strip_grid(lines, quads);
    const long long lpb = std::max<long long>(g.rows_per_block, XSW_CAL_MIN_LINES);
    const dim3 grid((unsigned)g.gx, (unsigned)((lines + lpb - 1) / lpb));
    return run(c, mem, b, [&](Buf (&x)[25]) {
        CalArgs a{};
        Tab *dst[4] = {&a.lut, &a.range, &a.azimuth, &a.inc};
        for (int k = 0; k < 4; ++k)
            if (mask & (1 << k))
                *dst[k] = Tab{(const double *)x[1 + 5 * k].dev, (const int *)x[2 + 5 * k].dev, (const double *)x[3 + 5 * k].dev,
                              (const int *)x[4 + 5 * k].dev, (const double *)x[5 + 5 * k].dev, (int)tabs[k]->n_lines, (int)tabs[k]->n_samples};
        a.lines = lines; a.samples = samples; a.lines_per_block = lpb;
        a.use_fill = dn ? use_fill : 0;
        a.fill_u16 = (use_fill && !f32_dn) ? (unsigned)fill : 0u;
        a.fill_f32 = (float)fill;
        const bool vec = samples % 4 == 0 && aligned(x[0].dev, 4 * es) && aligned(x[21].dev, 16) && aligned(x[22].dev, 16) && aligned(x[23].dev, 16) &&
                         aligned(x[24].dev, 4);
        auto go = [&](auto dn_t, auto out_t, auto vec_t, auto tabs_t) {
            using DN = decltype(dn_t);
            using OUT = decltype(out_t);
            hipLaunchKernelGGL((k_calibrate<DN, OUT, decltype(vec_t)::value, decltype(tabs_t)::value>), grid, dim3(256), 0, c->stream,
                               (const DN *)x[0].dev, (OUT *)x[21].dev, (OUT *)x[22].dev, (OUT *)x[23].dev, (unsigned char *)x[24].dev, a);
        };
        auto by_tabs = [&](auto dn_t, auto out_t, auto vec_t) {
            switch (mask) {  // the nine combinations the checks above let through
            case 1: go(dn_t, out_t, vec_t, std::integral_constant<int, 1>{}); break;
            case 3: go(dn_t, out_t, vec_t, std::integral_constant<int, 3>{}); break;
            case 5: go(dn_t, out_t, vec_t, std::integral_constant<int, 5>{}); break;
            case 7: go(dn_t, out_t, vec_t, std::integral_constant<int, 7>{}); break;
            case 9: go(dn_t, out_t, vec_t, std::integral_constant<int, 9>{}); break;
            case 11: go(dn_t, out_t, vec_t, std::integral_constant<int, 11>{}); break;
            case 13: go(dn_t, out_t, vec_t, std::integral_constant<int, 13>{}); break;
            case 15: go(dn_t, out_t, vec_t, std::integral_constant<int, 15>{}); break;
            default:
                if constexpr (std::is_same_v<decltype(dn_t), unsigned short>) go(dn_t, out_t, vec_t, std::integral_constant<int, TAB_INC>{});
            }
        };
        auto by_vec = [&](auto dn_t, auto out_t) {
            if (vec) by_tabs(dn_t, out_t, std::true_type{});
            else by_tabs(dn_t, out_t, std::false_type{});
        };
        auto by_out = [&](auto dn_t) {
            if (f64_out) by_vec(dn_t, double{});
            else by_vec(dn_t, float{});
        };
        if (f32_dn) by_out(float{});
        else by_out((unsigned short)0);
    }, "calibrate");
}
