// Sea / land keep mask from coastline edges: the kernels behind xsarsea_amd.landmask and its C ABI (xsw_land_mask,
// include/xsw.h).  A pixel's position comes from the scene's tie points (xsw_tie.hpp: tie_lonlat, the arithmetic of
// xsw_ancillary_model's step 1), its byte from the even-odd rule over the edges, in the half-open form the header states: no
// division, no library call, every operation float64 and rounded once (-ffp-contract=off, xsarsea_amd/_build.py), so that
// tests/landmask_ref.py can ask for equal bytes.
//
//   k_land_mask         a thread owns four consecutive samples of XSW_LAND_LINES lines; the edges are sorted into latitude bands
//                       on the host (xsarsea_amd/landmask.py), a workgroup stages the lists of the bands its pixels fall into
//                       into LDS, chunk by chunk, and every thread walks a chunk with broadcast reads, testing only those of its
//                       pixels whose own band is the staged one
//   k_land_mask_direct  every pixel against every edge, the same staging without bands: what the tests compare the banded
//                       kernel with, and the baseline of profiles/bench_landmask.py
//
// One thread owns its bytes: no atomics.  A band decides which edges a pixel meets, never what an edge answers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "xsw_host.hpp"
#include "xsw_run.hpp"
#include "xsw_tie.hpp"

namespace {

// Edges of one staging chunk: 32 B each, 32 KiB, so that four workgroups (128 KiB) fit a CU's 160 KiB of LDS.  k_land_mask_direct
// runs that many and more; k_land_mask, with the positions of 16 pixels per lane in registers (about 190 VGPRs), runs two
// workgroups per CU: it is the registers, not the chunk, that bound it (profiles/landmask_kernel_resources.tsv).
#ifndef XSW_LAND_CHUNK
#define XSW_LAND_CHUNK 1024
#endif
#ifndef XSW_LAND_LINES
#define XSW_LAND_LINES 4  // lines of a line group
#endif

struct alignas(32) Edge {
    double x1, y1, x2, y2;
};

struct LandArgs {
    uint8_t *out;
    const uint8_t *and_with;
    long long lines, samples, lines_per_block;
    const double *tlon, *tlat;
    int nl, ns;
    const int *li0;
    const double *lt;
    const int *sj0;
    const double *st;
    const double *edges;  // [n_edges][4] = x1, y1, x2, y2
    int n_edges;
    const int *band_start, *band_edges;
    int n_bands, n_list;
    double lat0, h;
    int invert, vec;  // vec: rows and bases are 4-byte aligned (samples % 4 == 0): one 4-byte load and store per thread and line
};

// The statement of include/xsw.h (xsw_land_mask), per edge.  The straddle test comes first; the products are formed only inside
// the edge's own longitude range.
__device__ inline bool edge_hit(double px, double py, double x1, double y1, double x2, double y2)
{
    if ((y1 > py) == (y2 > py)) return false;
    const double xmin = fmin(x1, x2), xmax = fmax(x1, x2);
    if (px < xmin) return true;
    if (!(px <= xmax)) return false;
    const double a = (px - x1) * (y2 - y1), b = (py - y1) * (x2 - x1);
    return y2 > y1 ? a < b : a > b;
}

// The sample brackets of a thread's four columns (a column past the raster reads the last one's and is never stored).
struct Columns {
    int j0[4], j1[4];
    double ws1[4];
};

__device__ inline Columns columns_of(const LandArgs &A, long long col0)
{
    Columns c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long s = col0 + q < A.samples ? col0 + q : A.samples - 1;
        c.j0[q] = min(max(A.sj0[s], 0), A.ns - 1);
        c.j1[q] = min(c.j0[q] + 1, A.ns - 1);
        c.ws1[q] = A.st[s];
    }
    return c;
}

__device__ inline TieLonLat pixel_at(const LandArgs &A, const Columns &c, int q, long long line)
{
    const int i0 = min(max(A.li0[line], 0), A.nl - 1);
    const double tl = A.lt[line];
    return tie_lonlat(A.tlon, A.tlat, i0, min(i0 + 1, A.nl - 1), c.j0[q], c.j1[q], A.ns, 1.0 - c.ws1[q], c.ws1[q], 1.0 - tl, tl);
}

// The four bytes of a thread on one line: land[q] from the parity, 1 = water unless inverted, and_with folded in after that.
template <bool AND>
__device__ inline void store_line(const LandArgs &A, long long line, long long col0, unsigned land4)
{
    const long long at = line * A.samples + col0;
    const unsigned flip = A.invert ? 0u : 1u;
    if (A.vec) {  // col0 + 3 < samples: samples is a multiple of four
        unsigned w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) w |= (((land4 >> q) & 1u) ^ flip) << (8 * q);
        if (AND) {
            const unsigned m = *reinterpret_cast<const unsigned *>(A.and_with + at);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (!((m >> (8 * q)) & 0xffu)) w &= ~(0xffu << (8 * q));
        }
        *reinterpret_cast<unsigned *>(A.out + at) = w;
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (col0 + q >= A.samples) break;
        unsigned v = ((land4 >> q) & 1u) ^ flip;
        if (AND && !A.and_with[at + q]) v = 0;
        A.out[at + q] = (uint8_t)v;
    }
}

__device__ inline void stage_edge(Edge *dst, const double *__restrict__ edges, int e)
{
    const double *p = edges + 4 * (long long)e;
    dst->x1 = p[0]; dst->y1 = p[1]; dst->x2 = p[2]; dst->y2 = p[3];
}

// grid.x tiles the sample axis in blocks of 1024 (256 threads of four samples), grid.y the lines (strip_grid on the raster of
// sample quads).  Per line group of XSW_LAND_LINES lines: the positions and band indices of the thread's pixels; the workgroup's
// band range and westernmost pixel by a wave shuffle and four LDS words; then, band by band, the band's list staged in chunks.
// A band's list is ordered by descending xmax (the host plan's rule): a thread stops at the first edge wholly west of its pixels
// of that band, the workgroup at the first chunk that begins with an edge wholly west of all its pixels.  Both skips are exact:
// such an edge is neither east nor mid.  Indices (brackets, band_start, band_edges) are clamped, never trusted.
template <bool AND>
__global__ __launch_bounds__(256) void k_land_mask(LandArgs A)
{
    constexpr int NL = XSW_LAND_LINES, NP = 4 * NL;
    static_assert(NP <= 32, "the parity bits of a line group live in one word");
    __shared__ Edge s_edge[XSW_LAND_CHUNK];
    __shared__ int s_lo[4], s_hi[4];
    __shared__ double s_west[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const long long col0 = ((long long)blockIdx.x * 256 + tid) * 4;
    const long long l0 = (long long)blockIdx.y * A.lines_per_block;
    const long long l1 = l0 + A.lines_per_block < A.lines ? l0 + A.lines_per_block : A.lines;
    const Columns cols = columns_of(A, col0);
    const int last_band = A.n_bands - 1;
    for (long long l = l0; l < l1; l += NL) {
        double px[NP], py[NP];
        int band[NP];
        int lo = INT_MAX, hi = -1;
        double west = INFINITY;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const long long line = l + k < l1 ? l + k : l1 - 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = 4 * k + q;
                const TieLonLat g = pixel_at(A, cols, q, line);
                px[p] = g.lon;
                py[p] = g.lat;
                const bool live = l + k < l1 && col0 + q < A.samples;
                // clamp(floor((lat - lat0) / h), 0, n_bands - 1); a NaN goes to band 0
                const int b = (int)fmin(fmax(floor((g.lat - A.lat0) / A.h), 0.0), (double)last_band);
                band[p] = live ? b : -1;
                if (live) {
                    lo = min(lo, b);
                    hi = max(hi, b);
                    west = fmin(west, g.lon);
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo = min(lo, __shfl_xor(lo, off));
            hi = max(hi, __shfl_xor(hi, off));
            west = fmin(west, __shfl_xor(west, off));
        }
        if ((tid & 63) == 0) {
            s_lo[wave] = lo;
            s_hi[wave] = hi;
            s_west[wave] = west;
        }
        __syncthreads();
        lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
        west = fmin(fmin(s_west[0], s_west[1]), fmin(s_west[2], s_west[3]));
        unsigned land = 0;
        for (int b = lo; b <= hi; ++b) {  // (no live pixel: lo > hi)
            const int e0 = min(max(A.band_start[b], 0), A.n_list), e1 = min(max(A.band_start[b + 1], e0), A.n_list);
            unsigned mine = 0;
            double my_west = INFINITY;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (band[p] == b) {
                    mine |= 1u << p;
                    my_west = fmin(my_west, px[p]);
                }
            for (int c0 = e0; c0 < e1; c0 += XSW_LAND_CHUNK) {
                const double *f = A.edges + 4 * (long long)min(max(A.band_edges[c0], 0), A.n_edges - 1);
                if (fmax(f[0], f[2]) < west) break;  // workgroup-uniform: this edge and every later one lie west of all its pixels
                const int n = min(XSW_LAND_CHUNK, e1 - c0);
                __syncthreads();  // the chunk before has been walked
                for (int i = tid; i < n; i += 256) stage_edge(&s_edge[i], A.edges, min(max(A.band_edges[c0 + i], 0), A.n_edges - 1));
                __syncthreads();
                if (!mine) continue;
                for (int i = 0; i < n; ++i) {
                    const Edge e = s_edge[i];  // one address per wave: a broadcast read
                    if (fmax(e.x1, e.x2) < my_west) {
                        mine = 0;  // ... and so are the chunks that follow
                        break;
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        if ((mine >> p) & 1u) land ^= (unsigned)edge_hit(px[p], py[p], e.x1, e.y1, e.x2, e.y2) << p;
                }
            }
        }
        __syncthreads();  // s_lo / s_hi / s_west and the last chunk are free for the next line group
#pragma unroll
        for (int k = 0; k < NL; ++k)
            if (l + k < l1 && col0 < A.samples) store_line<AND>(A, l + k, col0, (land >> (4 * k)) & 0xfu);
    }
}

// The same grid; one line at a time, every edge in the order given, no bands and no early stop.
template <bool AND>
__global__ __launch_bounds__(256) void k_land_mask_direct(LandArgs A)
{
    __shared__ Edge s_edge[XSW_LAND_CHUNK];
    const int tid = threadIdx.x;
    const long long col0 = ((long long)blockIdx.x * 256 + tid) * 4;
    const long long l0 = (long long)blockIdx.y * A.lines_per_block;
    const long long l1 = l0 + A.lines_per_block < A.lines ? l0 + A.lines_per_block : A.lines;
    const Columns cols = columns_of(A, col0);
    for (long long l = l0; l < l1; ++l) {
        double px[4], py[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const TieLonLat g = pixel_at(A, cols, q, l);
            px[q] = g.lon;
            py[q] = g.lat;
        }
        unsigned land = 0;
        for (int c0 = 0; c0 < A.n_edges; c0 += XSW_LAND_CHUNK) {
            const int n = min(XSW_LAND_CHUNK, A.n_edges - c0);
            __syncthreads();
            for (int i = tid; i < n; i += 256) stage_edge(&s_edge[i], A.edges, c0 + i);
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const Edge e = s_edge[i];
#pragma unroll
                for (int q = 0; q < 4; ++q) land ^= (unsigned)edge_hit(px[q], py[q], e.x1, e.y1, e.x2, e.y2) << q;
            }
        }
        if (col0 < A.samples) store_line<AND>(A, l, col0, land);
    }
}

// XSW_LAND_PATH, read at every call: 0 bands (also when unset), 1 direct, -1 anything else.
int land_path()
{
    const char *v = getenv("XSW_LAND_PATH");
    if (!v || !strcmp(v, "bands")) return 0;
    return strcmp(v, "direct") ? -1 : 1;
}

}  // namespace

extern "C" int32_t xsw_land_chunk_edges(void) { return XSW_LAND_CHUNK; }

extern "C" int xsw_land_mask(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t n_tie_lines, int32_t n_tie_samples,
                             const double *tie_lon, const double *tie_lat, const int32_t *line_first, const double *line_t,
                             const int32_t *sample_first, const double *sample_t, int32_t n_edges, const double *edges, int32_t n_bands,
                             const int32_t *band_start, int32_t n_list, const int32_t *band_edges, double lat0, double h, const uint8_t *and_with,
                             int32_t invert, uint8_t *out)
{
    if (!c) return XSW_EINVAL;
    if (lines < 0 || samples < 0) return fail(c, XSW_EINVAL, "land_mask: negative raster shape");
    if (!tie_lon || !tie_lat || !line_first || !line_t || !sample_first || !sample_t || !out || n_tie_lines < 1 || n_tie_samples < 1)
        return fail(c, XSW_EINVAL, "land_mask: bad argument");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    if (invert != 0 && invert != 1) return fail(c, XSW_EINVAL, "land_mask: invert must be 0 or 1");
    if (n_edges < 0 || (n_edges > 0 && !edges) || n_edges > INT_MAX / 4) return fail(c, XSW_EINVAL, "land_mask: n_edges must be >= 0, with their array");
    if (n_bands < 0 || n_bands > 65536 || n_list < 0) return fail(c, XSW_EINVAL, "land_mask: n_bands must be 0 .. 65536 and n_list >= 0");
    if (n_bands > 0 && (!band_start || (n_list > 0 && !band_edges) || !std::isfinite(lat0) || !std::isfinite(h) || !(h > 0.0)))
        return fail(c, XSW_EINVAL, "land_mask: bands need band_start, band_edges, a finite lat0 and a finite h > 0");
    const int path = land_path();
    if (path < 0) return fail(c, XSW_EINVAL, "XSW_LAND_PATH must be direct or bands, not '%s'", getenv("XSW_LAND_PATH"));
    if (int rc = check_dims(c, "land_mask", lines, samples)) return rc;
    if (n_bands > 0 && mem == XSW_MEM_HOST) {  // host tables can be read here; device tables are clamped by the kernel
        for (int32_t b = 0; b < n_bands; ++b)
            if (band_start[b] < 0 || band_start[b + 1] < band_start[b] || band_start[b + 1] > n_list)
                return fail(c, XSW_EINVAL, "land_mask: band_start must ascend from >= 0 to <= n_list (band %d)", (int)b);
        for (int32_t k = 0; k < n_list; ++k)
            if (band_edges[k] < 0 || band_edges[k] >= n_edges)
                return fail(c, XSW_EINVAL, "land_mask: band_edges[%d] = %d is outside [0, %d)", (int)k, (int)band_edges[k], (int)n_edges);
    }
    if (!lines || !samples) return XSW_OK;
    const bool banded = path == 0 && n_bands > 0 && n_edges > 0 && n_list > 0;  // no edges: all water, by the direct kernel's empty loop
    const size_t npx = (size_t)lines * samples, ties = (size_t)n_tie_lines * n_tie_samples * 8;
    Buf b[11] = {{tie_lon, nullptr, ties}, {tie_lat, nullptr, ties}, {line_first, nullptr, (size_t)lines * 4}, {line_t, nullptr, (size_t)lines * 8},
                 {sample_first, nullptr, (size_t)samples * 4}, {sample_t, nullptr, (size_t)samples * 8}, in_buf(edges, (size_t)n_edges * 32),
                 in_buf(banded ? band_start : nullptr, ((size_t)n_bands + 1) * 4), in_buf(banded ? band_edges : nullptr, (size_t)n_list * 4),
                 in_buf(and_with, npx), {nullptr, out, npx}};
    const Strips g = strip_grid(lines, (samples + 3) / 4);
    return run(c, mem, b, [&](Buf (&x)[11]) {
        LandArgs A;
        A.out = (uint8_t *)x[10].dev;
        A.and_with = (const uint8_t *)x[9].dev;
        A.lines = lines; A.samples = samples; A.lines_per_block = g.rows_per_block;
        A.tlon = (const double *)x[0].dev; A.tlat = (const double *)x[1].dev;
        A.nl = n_tie_lines; A.ns = n_tie_samples;
        A.li0 = (const int *)x[2].dev; A.lt = (const double *)x[3].dev; A.sj0 = (const int *)x[4].dev; A.st = (const double *)x[5].dev;
        A.edges = (const double *)x[6].dev; A.n_edges = n_edges;
        A.band_start = (const int *)x[7].dev; A.band_edges = (const int *)x[8].dev;
        A.n_bands = n_bands; A.n_list = n_list;
        A.lat0 = lat0; A.h = h;
        A.invert = invert;
        A.vec = samples % 4 == 0 && (uintptr_t)A.out % 4 == 0 && (uintptr_t)A.and_with % 4 == 0;
        const dim3 grid((unsigned)g.gx, (unsigned)g.gy), block(256);
        if (banded) {
            if (A.and_with) hipLaunchKernelGGL(k_land_mask<true>, grid, block, 0, c->stream, A);
            else hipLaunchKernelGGL(k_land_mask<false>, grid, block, 0, c->stream, A);
        } else {
            if (A.and_with) hipLaunchKernelGGL(k_land_mask_direct<true>, grid, block, 0, c->stream, A);
            else hipLaunchKernelGGL(k_land_mask_direct<false>, grid, block, 0, c->stream, A);
        }
    }, "land_mask");
}
