// Block statistics of a raster on a product grid: the kernels behind xsarsea_amd.cells and its C ABI (xsw_wind_cells,
// xsw_raster_cells; include/xsw.h has the statement).  The raster is tiled from pixel (0, 0) by cells of cell_lines x cell_samples
// pixels, the last cell of an axis clipped; every cell gets its valid count, its float64 sums in ONE stated order and what
// follows from them -- vector and scalar mean wind, its scatter and steadiness, with tie points the centre's position and the
// east / north components; or mean and scatter of a real raster.
//
//   k_cells<Src, MAP>   Src: complex128 / complex64 winds, co-pol grid codes (read through `sol`, as k_expand reads them: 4 B per
//                       pixel, nothing expanded), float32 / float64 rasters.  MAP: one wave per cell, or one 256-thread
//                       workgroup per cell.  A cell has exactly one owner and there is no atomic: the result does not depend
//                       on the launch.
//   k_wind_grid<Src, DIRECT>  the same wind sources binned on a regular longitude / latitude grid (xsw_wind_grid,
//                       xsarsea_amd.grid): every pixel geolocated from the tie points, its terms added to its bin as 64-bit
//                       integers in fixed point, which have no order; stated and described further down.
//   k_wind_polar<Src, DIRECT> the same binned in rings and sectors around a given centre (xsw_wind_polar, xsarsea_amd.polar),
//                       with the radial and tangential components and the bin's largest speed; after k_wind_grid.
//   k_wind_centre<Src, DIRECT> the annulus sums of k_wind_polar around every node of a lattice of candidate centres
//                       (xsw_wind_centre, xsarsea_amd.centre): every pixel meets every candidate; after k_wind_polar.
//
// The order of every sum: pixel p = r * w + c of a cell (w its clipped width) goes to accumulator p mod 256; each accumulator
// starts at +0.0 and adds its pixels in ascending p, an invalid pixel adding +0.0 (which changes no accumulator: none is ever
// -0.0); then a[i] += a[i + h] for i < h, h = 128 .. 1.  A wave owns the 256 accumulators four per lane (t, t + 64, t + 128,
// t + 192): the folds at 128 and 64 are lane-local, the rest is an xor butterfly (IEEE addition commutes, so both partners of
// an exchange hold the same bits).  A workgroup owns them one per thread: the folds at 128 and 64 go through LDS, wave 0 does
// the butterfly.  Both give the bits of tests/cells_ref.py.  -ffp-contract=off (xsarsea_amd/_build.py) keeps q = re * re +
// im * im free of contractions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "xsw_codes.hpp"
#include "xsw_host.hpp"
#include "xsw_run.hpp"
#include "xsw_tie.hpp"

namespace {

#ifndef XSW_CELLS_WG_AREA
#define XSW_CELLS_WG_AREA 4096  // cells of at least this many pixels (cell_lines * cell_samples) get a workgroup each, smaller ones a wave.
                                // Measured on 20000 x 20000 (profiles/cells_bench.json; ms wave / workgroup, complex128 | codes | float32), cells of
                                // 20 x 20: 1.81 / 2.76 | 1.81 / 2.74 | 0.85 / 1.65, 32 x 32: 1.32 / 1.38 | 1.34 / 1.32 | 0.61 / 0.84,
                                // 50 x 50: 1.25 / 1.23 | 1.26 / 1.20 | 0.56 / 0.69, 70 x 70: 1.23 / 1.08 | 1.26 / 1.11 | 0.55 / 0.59,
                                // 100 x 100: 1.23 / 1.06 | 1.34 / 1.19 | 0.55 / 0.56, 300 x 300: 1.36 / 1.14 | 1.64 / 1.32 | 0.87 / 0.63,
                                // 1000 x 1000: 8.92 / 2.59 | 10.1 / 2.85 | 7.74 / 2.07.  The wind sources cross near 50 x 50, float32 near 100 x 100.
#endif
// The mapping of a call: a function of the cell's nominal area alone.  Environment XSW_CELLS_MAPPING = wave | workgroup forces
// one (tests, measurements); it is read on the host at every call, so that one process can compare the two.
enum { MAP_WAVE = 0, MAP_WORKGROUP = 1 };
static int cells_mapping(long long area, bool &bad_env)
{
    bad_env = false;
    if (const char *v = getenv("XSW_CELLS_MAPPING")) {
        if (!strcmp(v, "wave")) return MAP_WAVE;
        if (!strcmp(v, "workgroup")) return MAP_WORKGROUP;
        bad_env = true;
    }
    return area >= XSW_CELLS_WG_AREA ? MAP_WORKGROUP : MAP_WAVE;
}

struct CellGrid {
    long long lines, samples, n_sc, ncells;  // the raster, cells per cell row, cells in all
    int cl, cs;
};

// One pixel as fetched: a wind's two parts or a real value in `a`, and whether the source itself calls it valid.
struct Px {
    double a, b;
    bool ok;
};

// ---- sources.  fetch(i): pixel i of the raster.  NS sums per cell; terms(): what a valid pixel adds to them.
struct WindSums {
    static constexpr int NS = 4;  // re, im, s, q
    __device__ static void terms(const Px &x, double (&v)[NS])
    {
        const double q = x.a * x.a + x.b * x.b;
        v[0] = x.a; v[1] = x.b; v[2] = sqrt(q); v[3] = q;
    }
};
struct RealSums {
    static constexpr int NS = 2;  // x, x * x
    __device__ static void terms(const Px &x, double (&v)[NS]) { v[0] = x.a; v[1] = x.a * x.a; }
};

struct SrcC128 : WindSums {
    const double2 *p;
    __device__ Px fetch(long long i) const { const double2 z = p[i]; return Px{z.x, z.y, !(z.x != z.x) && !(z.y != z.y)}; }
};
struct SrcC64 : WindSums {
    const float2 *p;
    __device__ Px fetch(long long i) const { const float2 z = p[i]; return Px{(double)z.x, (double)z.y, !(z.x != z.x) && !(z.y != z.y)}; }
};
struct SrcCodes : WindSums {
    const unsigned *p;
    const double *sol;
    long long plane;
    __device__ Px fetch(long long i) const
    {
        const auto read = [](const double *table, long long k) { const double2 z = ((const double2 *)table)[k]; return xsw::Wind{z.x, z.y}; };
        xsw::Wind co;
        const xsw::CoPoint g = xsw::expand_co(p[i], plane, sol, read, co);  // valid iff co_decode(code, plane).grid()
        return Px{co.re, co.im, g.have};
    }
};
template <typename T>
struct SrcReal : RealSums {
    const T *p;
    __device__ Px fetch(long long i) const { const T x = p[i]; return Px{(double)x, 0.0, !(x != x)}; }
};

// ---- what is written per cell, by the one lane that holds the folded sums.  Every pointer may be null: not computed, not written.
__device__ inline double scatter(double sq, double s, double nd, int n)
{
    const double var = (sq - (s * s) / nd) / (nd - 1.0);
    return n < 2 ? __builtin_nan("") : sqrt(var < 0.0 ? 0.0 : var);  // not fmax: n == 1 must stay NaN
}

struct WindOuts {
    int *count;
    double2 *wind;
    double *wspd, *wspd_std, *steadiness, *lon, *lat, *u, *v;
    const double *tlon, *tlat, *tcos, *tsin;  // tlon null: no geolocation
    const int *li0, *sj0;                     // per cell row / cell column: the bracket of the centre between tie points
    const double *lt, *st;
    int nl, ns;
    __device__ void write(long long cell, long long ci, long long cj, int n, const double (&s)[4]) const
    {
        const double nd = (double)n;
        const double mre = s[0] / nd, mim = s[1] / nd, ws = s[2] / nd;
        if (count) count[cell] = n;
        if (wind) wind[cell] = make_double2(mre, mim);
        if (wspd) wspd[cell] = ws;
        if (wspd_std) wspd_std[cell] = scatter(s[3], s[2], nd, n);
        if (steadiness) steadiness[cell] = sqrt(mre * mre + mim * mim) / ws;
        if (!tlon) return;
        const int i0 = min(max(li0[ci], 0), nl - 1), j0 = min(max(sj0[cj], 0), ns - 1);
        const double tl = lt[ci], ts = st[cj];
        const TieRows q = tie_rows(tlon, tlat, tcos, tsin, i0, min(i0 + 1, nl - 1), j0, min(j0 + 1, ns - 1), ns, 1.0 - ts, ts);
        const TiePoint g = tie_point(q, 1.0 - tl, tl);
        if (lon) lon[cell] = g.lon;
        if (lat) lat[cell] = g.lat;
        if (u) u[cell] = -(mre * g.ch + mim * g.sh);
        if (v) v[cell] = -(mim * g.ch - mre * g.sh);
    }
};

struct RealOuts {
    int *count;
    double *mean, *std;
    __device__ void write(long long cell, long long, long long, int n, const double (&s)[2]) const
    {
        const double nd = (double)n;
        if (count) count[cell] = n;
        if (mean) mean[cell] = s[0] / nd;
        if (std) std[cell] = scatter(s[1], s[0], nd, n);
    }
};

// A thread walks its cell in steps of STRIDE pixels (64: a wave's lane, 256: a workgroup's thread), STEPS = 4 steps per trip,
// whose four loads (and keep bytes) are issued before the first is used.  Wave: step j of a trip feeds accumulator t + 64 j.
// Workgroup: the four steps feed the thread's one accumulator in ascending p (eight steps per trip measured no better: 2.71
// against 2.59 ms at 1000 x 1000, 1.15 against 1.05 ms at 100 x 100).  (r, c) follow p without a division per pixel.
template <typename Src, int MAP, typename Outs>
__global__ __launch_bounds__(256) void k_cells(const Src src, const unsigned char *__restrict__ keep, const CellGrid g, const Outs o)
{
    constexpr int NS = Src::NS, STRIDE = MAP == MAP_WAVE ? 64 : 256, NACC = MAP == MAP_WAVE ? 4 : 1, STEPS = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = MAP == MAP_WAVE ? lane : (int)threadIdx.x;
    const long long cell = MAP == MAP_WAVE ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
    if (cell >= g.ncells) return;  // whole waves of the last workgroup (wave mapping only: no barrier follows there)
    const long long ci = cell / g.n_sc, cj = cell - ci * g.n_sc;
    const long long row0 = ci * g.cl, col0 = cj * g.cs;
    const long long h = min((long long)g.cl, g.lines - row0);
    const int w = (int)min((long long)g.cs, g.samples - col0);
    const long long N = h * w, first = row0 * g.samples + col0;
    const int dq = STRIDE / w, dr = STRIDE % w;
    long long r = t / w;
    int c = t % w;

    double acc[NACC][NS];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int k = 0; k < NS; ++k) acc[j][k] = 0.0;
    int n = 0;
    for (long long b = t; b - t < N; b += STEPS * STRIDE) {
        Px x[STEPS];
#pragma unroll
        for (int j = 0; j < STEPS; ++j) {
            x[j] = Px{0.0, 0.0, false};
            if (b + j * STRIDE < N) {
                const long long i = first + r * g.samples + c;
                x[j] = src.fetch(i);
                if (keep) x[j].ok = x[j].ok && keep[i] != 0;
            }
            c += dr;
            r += dq;
            if (c >= w) { c -= w; ++r; }
        }
#pragma unroll
        for (int j = 0; j < STEPS; ++j) {
            double v[NS];
            Src::terms(x[j], v);
            n += x[j].ok ? 1 : 0;
#pragma unroll
            for (int k = 0; k < NS; ++k) acc[MAP == MAP_WAVE ? j : 0][k] += x[j].ok ? v[k] : 0.0;
        }
    }

    double s[NS];
    if constexpr (MAP == MAP_WAVE) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            acc[0][k] += acc[2][k];  // h = 128
            acc[1][k] += acc[3][k];
            s[k] = acc[0][k] + acc[1][k];  // h = 64
        }
    } else {
        __shared__ double part[NS][256];
        __shared__ int part_n[4];
#pragma unroll
        for (int k = 0; k < NS; ++k) part[k][t] = acc[0][k];
        __syncthreads();
        if (t < 128)  // h = 128
#pragma unroll
            for (int k = 0; k < NS; ++k) part[k][t] += part[k][t + 128];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = t < 64 ? part[k][t] + part[k][t + 64] : 0.0;  // h = 64
#pragma unroll
        for (int hh = 32; hh >= 1; hh >>= 1) n += __shfl_xor(n, hh);
        if (lane == 0) part_n[wave] = n;
        __syncthreads();
        if (wave != 0) return;
        n = part_n[0] + part_n[1] + part_n[2] + part_n[3];
    }
#pragma unroll
    for (int hh = 32; hh >= 1; hh >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += __shfl_xor(s[k], hh);
        if constexpr (MAP == MAP_WAVE) n += __shfl_xor(n, hh);
    }
    if (lane == 0) o.write(cell, ci, cj, n, s);
}

template <typename Src, typename Outs>
static void launch_cells(hipStream_t stream, int map, const Src &src, const void *keep, const CellGrid &g, const Outs &o)
{
    if (map == MAP_WAVE)
        hipLaunchKernelGGL((k_cells<Src, MAP_WAVE, Outs>), dim3((unsigned)((g.ncells + 3) / 4)), dim3(256), 0, stream, src, (const unsigned char *)keep, g, o);
    else
        hipLaunchKernelGGL((k_cells<Src, MAP_WORKGROUP, Outs>), dim3((unsigned)g.ncells), dim3(256), 0, stream, src, (const unsigned char *)keep, g, o);
}

// The refusals the two entries share, the cell grid and the mapping.
static int plan_cells(xsw_ctx *c, const char *who, int64_t lines, int64_t samples, int32_t mem, int32_t cell_lines, int32_t cell_samples, CellGrid &g,
                      int &map)
{
    if (lines < 1 || samples < 1) return fail(c, XSW_EINVAL, "%s: the raster must have one line and one sample or more", who);
    if (cell_lines < 1 || cell_samples < 1) return fail(c, XSW_EINVAL, "%s: cells must be 1 x 1 pixels or more, not %d x %d", who, (int)cell_lines, (int)cell_samples);
    if (int rc = check_dims(c, who, lines, samples + 256)) return rc;  // the kernel's column index runs up to 256 past a cell's width
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    g.lines = lines; g.samples = samples;
    g.cl = (int)std::min<int64_t>(cell_lines, lines);  // a larger cell is clipped to the raster anyway
    g.cs = (int)std::min<int64_t>(cell_samples, samples);
    const long long n_lc = (lines + g.cl - 1) / g.cl;
    g.n_sc = (samples + g.cs - 1) / g.cs;
    g.ncells = n_lc * g.n_sc;
    bool bad_env;
    map = cells_mapping((long long)cell_lines * cell_samples, bad_env);
    if (bad_env) return fail(c, XSW_EINVAL, "%s: XSW_CELLS_MAPPING must be wave or workgroup", who);
    if ((map == MAP_WAVE ? (g.ncells + 3) / 4 : g.ncells) > 0x7fffffffLL) return fail(c, XSW_EINVAL, "%s: too many cells for one launch", who);
    return XSW_OK;
}

// ---- wind on a regular longitude / latitude grid: order-free binning in fixed point (xsw_wind_grid; include/xsw.h has the
// statement).  Every valid pixel adds five 64-bit integers to its bin, so the sums depend on no order: the launch geometry, the
// pre-aggregation below and the path switch change no bit.
#ifndef XSW_GRID_LINES
#define XSW_GRID_LINES 4  // lines in flight per lane: their loads are issued before the first is used, as k_ancillary_model does
#endif
#ifndef XSW_GRID_MIN_LINES
#define XSW_GRID_MIN_LINES 32  // a workgroup's strip is at least this many lines long (strip_grid alone gives small rasters one line per workgroup: no run)
#endif
#ifndef XSW_GRID_SLOTS
#define XSW_GRID_SLOTS 256  // slots of the workgroup's LDS table, a power of two: 4 B of tag and 40 B of sums each, 11 KiB
#endif
static_assert((XSW_GRID_SLOTS & (XSW_GRID_SLOTS - 1)) == 0 && XSW_GRID_SLOTS >= 2, "the slot of a bin is a masked hash");

// The path of a call.  Environment XSW_GRID_PATH = direct | lds forces one (tests, measurements); read on the host at every call.
enum { GRID_LDS = 0, GRID_DIRECT = 1 };
static int grid_path(bool &bad_env)
{
    bad_env = false;
    if (const char *v = getenv("XSW_GRID_PATH")) {
        if (!strcmp(v, "direct")) return GRID_DIRECT;
        if (!strcmp(v, "lds")) return GRID_LDS;
        bad_env = true;
    }
    return GRID_LDS;
}

struct LonLat {
    double lon0, dlon, lat0, dlat;
    int n_lon, n_lat, periodic;
};

struct GridTies {
    const double *tlon, *tlat, *tcos, *tsin;
    const int *li0, *sj0;  // per line / per sample: the pixel's bracket between tie points
    const double *lt, *st;
    int nl, ns;
};

// llrint(a * scale), halves to even; |a * scale| < 2**33 for every pixel that is added.
__device__ inline unsigned long long fixed_point(double a, double scale) { return (unsigned long long)(long long)__builtin_rint(a * scale); }

// The geometry of k_ancillary_model: grid.x tiles the sample axis, one column per thread; grid.y tiles the lines into strips.  A
// thread keeps its sample bracket and the eight tie values blended along the sample axis; the line bracket is wave-uniform.
// DIRECT: every valid pixel's five adds go to global memory.  Otherwise three stages:
//   (a) while a thread walking down its column stays in one bin it keeps (bin, n, Su, Sv, Ss, Sq) in registers;
//   (b) on a bin change the run goes to the workgroup's direct-mapped LDS table: the slot's tag is claimed with a compare-and-swap,
//       the sums are added with LDS 64-bit adds; a slot held by another bin sends the run straight to global memory;
//   (c) at the end every occupied slot is added to global memory.
// Global adds are device-scope and return nothing; two's-complement addition makes the signed sums right.
// Measured on 20000 x 20000 complex128 (profiles/grid_bench.json; ms staged / DIRECT): bins of 0.1 degree 3.35 / 429, of 0.01 degree
// 3.73 / 131 (k_ancillary_model in the same run: 3.30); bins smaller than a pixel, 4000 x 4000: 2.40 / 2.30, where every pixel's five
// adds reach global memory either way: 3.4e10 64-bit adds per second.
template <typename Src, bool DIRECT>
__global__ __launch_bounds__(256) void k_wind_grid(const Src src, const unsigned char *__restrict__ keep, long long lines, long long samples,
                                                   const LonLat g, const GridTies tp, long long lines_per_block,
                                                   unsigned long long *__restrict__ sums)
{
    constexpr int SLOTS = DIRECT ? 1 : XSW_GRID_SLOTS;
    __shared__ int tag[SLOTS];
    __shared__ unsigned long long tab[5][SLOTS];
    const long long plane = (long long)g.n_lat * g.n_lon;
    if constexpr (!DIRECT) {
        for (int t = threadIdx.x; t < SLOTS; t += 256) {
            tag[t] = -1;
#pragma unroll
            for (int k = 0; k < 5; ++k) tab[k][t] = 0;
        }
        __syncthreads();
    }
    const auto to_global = [&](int bin, const unsigned long long (&s)[5]) {
#pragma unroll
        for (int k = 0; k < 5; ++k) atomicAdd(sums + k * plane + bin, s[k]);
    };
    const auto to_table = [&](int bin, const unsigned long long (&s)[5]) {
        const unsigned slot = (((unsigned)bin * 2654435761u) >> 16) & (SLOTS - 1);
        const int old = atomicCAS(&tag[slot], -1, bin);
        if (old == -1 || old == bin) {
#pragma unroll
            for (int k = 0; k < 5; ++k) atomicAdd(&tab[k][slot], s[k]);
        } else {
            to_global(bin, s);
        }
    };

    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col < samples) {  // (no return: the barriers around the table are the whole workgroup's)
        const long long l0 = (long long)blockIdx.y * lines_per_block;
        const long long l1 = l0 + lines_per_block < lines ? l0 + lines_per_block : lines;
        const int j0 = min(max(tp.sj0[col], 0), tp.ns - 1), j1 = min(j0 + 1, tp.ns - 1);
        const double ts = tp.st[col], ws0 = 1.0 - ts, ws1 = ts;
        const double dn_lon = (double)g.n_lon, dn_lat = (double)g.n_lat;
        int tie_cur = -1;
        TieRows q;
        int cur = -1;  // (a): the run's bin, none yet
        unsigned long long acc[5] = {0, 0, 0, 0, 0};
        for (long long l = l0; l < l1; l += XSW_GRID_LINES) {
            Px x[XSW_GRID_LINES];
#pragma unroll
            for (int k = 0; k < XSW_GRID_LINES; ++k) {
                x[k] = Px{0.0, 0.0, false};
                if (l + k < l1) {
                    const long long i = (l + k) * samples + col;
                    x[k] = src.fetch(i);
                    if (keep) x[k].ok = x[k].ok && keep[i] != 0;
                }
            }
#pragma unroll
            for (int k = 0; k < XSW_GRID_LINES; ++k) {
                if (l + k >= l1) break;
                const int i0 = min(max(tp.li0[l + k], 0), tp.nl - 1);
                const double tl = tp.lt[l + k];
                if (i0 != tie_cur) {
                    q = tie_rows(tp.tlon, tp.tlat, tp.tcos, tp.tsin, i0, min(i0 + 1, tp.nl - 1), j0, j1, tp.ns, ws0, ws1);
                    tie_cur = i0;
                }
                const TiePoint p = tie_point(q, 1.0 - tl, tl);
                const double re = x[k].a, im = x[k].b;
                const double qq = re * re + im * im, sp = sqrt(qq);
                const double u = -(re * p.ch + im * p.sh), v = -(im * p.ch - re * p.sh);
                double gx = (p.lon - g.lon0) / g.dlon;
                const double gy = (p.lat - g.lat0) / g.dlat;
                bool inside = gy >= 0.0 && gy < dn_lat;
                if (g.periodic) {
                    gx = gx - floor(gx / dn_lon) * dn_lon;
                    if (!(gx >= 0.0) || gx >= dn_lon) gx = 0.0;  // a rounding's width from a whole number of turns: bin 0
                } else {
                    inside = inside && gx >= 0.0 && gx < dn_lon;
                }
                if (!(x[k].ok && inside && !(u != u) && !(v != v) && qq < 65536.0)) continue;
                const int bi = min((int)floor(gx), g.n_lon - 1), bj = min((int)floor(gy), g.n_lat - 1);  // inside [0, n) already: never trusted
                const int bin = bj * g.n_lon + bi;
                const unsigned long long a[5] = {1ull, fixed_point(u, 16777216.0), fixed_point(v, 16777216.0), fixed_point(sp, 16777216.0),
                                                 fixed_point(qq, 65536.0)};
                if constexpr (DIRECT) {
                    to_global(bin, a);
                } else {
                    if (bin != cur) {
                        if (cur >= 0) to_table(cur, acc);
                        cur = bin;
#pragma unroll
                        for (int m = 0; m < 5; ++m) acc[m] = 0;
                    }
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[m] += a[m];
                }
            }
        }
        if constexpr (!DIRECT)
            if (cur >= 0) to_table(cur, acc);
    }
    if constexpr (!DIRECT) {
        __syncthreads();
        for (int t = threadIdx.x; t < SLOTS; t += 256) {  // (c)
            const int bin = tag[t];
            if (bin < 0) continue;
            const unsigned long long s[5] = {tab[0][t], tab[1][t], tab[2][t], tab[3][t], tab[4][t]};
            to_global(bin, s);
        }
    }
}

template <typename Src>
static void launch_grid(hipStream_t stream, int path, const Src &src, const void *keep, long long lines, long long samples, const LonLat &g,
                        const GridTies &tp, int64_t *sums)
{
    const Strips s = strip_grid(lines, samples);
    const long long lpb = std::max<long long>(s.rows_per_block, XSW_GRID_MIN_LINES);
    const dim3 grid((unsigned)s.gx, (unsigned)((lines + lpb - 1) / lpb));  // no more strips than strip_grid's: at most 65535
    if (path == GRID_DIRECT)
        hipLaunchKernelGGL((k_wind_grid<Src, true>), grid, dim3(256), 0, stream, src, (const unsigned char *)keep, lines, samples, g, tp, lpb,
                           (unsigned long long *)sums);
    else
        hipLaunchKernelGGL((k_wind_grid<Src, false>), grid, dim3(256), 0, stream, src, (const unsigned char *)keep, lines, samples, g, tp, lpb,
                           (unsigned long long *)sums);
}

// ---- wind around a given centre: rings and sectors on a local chart (xsw_wind_polar; include/xsw.h has the statement).  The
// sources, the geolocation, the walk down a column and the three stages are k_wind_grid's; a pixel adds five integers to its bin
// and raises a sixth, the bin's largest speed, by an unsigned 64-bit maximum (the value is never negative), which has no order
// either.  No trigonometric call: the sector is found by comparing against a host table of sin / cos of the sector borders of
// one quadrant, kept in LDS.
#ifndef XSW_POLAR_MAX_SECTORS
#define XSW_POLAR_MAX_SECTORS 360  // the LDS table holds sin and cos of XSW_POLAR_MAX_SECTORS / 4 + 1 borders
#endif
static_assert(XSW_POLAR_MAX_SECTORS % 4 == 0 && XSW_POLAR_MAX_SECTORS >= 4, "quadrant borders are sector borders");

struct Polar {
    double lon_c, lat_c, cos_c, sin_c, dr_km;
    int n_r, n_theta;
};

template <typename Src, bool DIRECT>
__global__ __launch_bounds__(256) void k_wind_polar(const Src src, const unsigned char *__restrict__ keep, long long lines, long long samples,
                                                    const Polar g, const double *__restrict__ sector_sin, const double *__restrict__ sector_cos,
                                                    const GridTies tp, long long lines_per_block, unsigned long long *__restrict__ sums)
{
    constexpr int SLOTS = DIRECT ? 1 : XSW_GRID_SLOTS, BORDERS = XSW_POLAR_MAX_SECTORS / 4 + 1;
    constexpr double D2R = 0.017453292519943295, R_KM = 6371.0088, KX = R_KM * D2R;
    __shared__ int tag[SLOTS];
    __shared__ unsigned long long tab[6][SLOTS];
    __shared__ double bsin[BORDERS], bcos[BORDERS];
    const long long plane = (long long)g.n_r * g.n_theta;
    const int mq = min(g.n_theta / 4, BORDERS - 1);  // (the entry refuses more sectors: never trusted)
    for (int t = threadIdx.x; t <= mq; t += 256) {
        bsin[t] = sector_sin[t];
        bcos[t] = sector_cos[t];
    }
    if constexpr (!DIRECT) {
        for (int t = threadIdx.x; t < SLOTS; t += 256) {
            tag[t] = -1;
#pragma unroll
            for (int k = 0; k < 6; ++k) tab[k][t] = 0;
        }
    }
    __syncthreads();
    const auto to_global = [&](int bin, const unsigned long long (&s)[6]) {
#pragma unroll
        for (int k = 0; k < 5; ++k) atomicAdd(sums + k * plane + bin, s[k]);
        atomicMax(sums + 5 * plane + bin, s[5]);
    };
    const auto to_table = [&](int bin, const unsigned long long (&s)[6]) {
        const unsigned slot = (((unsigned)bin * 2654435761u) >> 16) & (SLOTS - 1);
        const int old = atomicCAS(&tag[slot], -1, bin);
        if (old == -1 || old == bin) {
#pragma unroll
            for (int k = 0; k < 5; ++k) atomicAdd(&tab[k][slot], s[k]);
            atomicMax(&tab[5][slot], s[5]);
        } else {
            to_global(bin, s);
        }
    };

    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col < samples) {  // (no return: the barriers around the table are the whole workgroup's)
        const long long l0 = (long long)blockIdx.y * lines_per_block;
        const long long l1 = l0 + lines_per_block < lines ? l0 + lines_per_block : lines;
        const int j0 = min(max(tp.sj0[col], 0), tp.ns - 1), j1 = min(j0 + 1, tp.ns - 1);
        const double ts = tp.st[col], ws0 = 1.0 - ts, ws1 = ts;
        const double dn_r = (double)g.n_r, half_c = 0.5 * g.cos_c;
        int tie_cur = -1;
        TieRows q;
        int cur = -1;  // (a): the run's bin, none yet
        unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
        for (long long l = l0; l < l1; l += XSW_GRID_LINES) {
            Px px[XSW_GRID_LINES];
#pragma unroll
            for (int k = 0; k < XSW_GRID_LINES; ++k) {
                px[k] = Px{0.0, 0.0, false};
                if (l + k < l1) {
                    const long long i = (l + k) * samples + col;
                    px[k] = src.fetch(i);
                    if (keep) px[k].ok = px[k].ok && keep[i] != 0;
                }
            }
#pragma unroll
            for (int k = 0; k < XSW_GRID_LINES; ++k) {
                if (l + k >= l1) break;
                const int i0 = min(max(tp.li0[l + k], 0), tp.nl - 1);
                const double tl = tp.lt[l + k];
                if (i0 != tie_cur) {
                    q = tie_rows(tp.tlon, tp.tlat, tp.tcos, tp.tsin, i0, min(i0 + 1, tp.nl - 1), j0, j1, tp.ns, ws0, ws1);
                    tie_cur = i0;
                }
                const TiePoint p = tie_point(q, 1.0 - tl, tl);
                const double re = px[k].a, im = px[k].b;
                const double qq = re * re + im * im, sp = sqrt(qq);
                const double u = -(re * p.ch + im * p.sh), v = -(im * p.ch - re * p.sh);
                double dl = p.lon - g.lon_c;
                dl = dl - 360.0 * __builtin_rint(dl / 360.0);
                const double dy = (p.lat - g.lat_c) * D2R, h = 0.5 * dy;
                const double m = (g.cos_c - g.sin_c * h) - half_c * (h * h);
                const double x = (KX * dl) * m, y = R_KM * dy;
                const double rr = x * x + y * y, r = sqrt(rr);
                const double fr = floor(r / g.dr_km);
                if (!(px[k].ok && fr < dn_r && !(u != u) && !(v != v) && qq < 65536.0)) continue;  // (a NaN radius fails fr < n_r)
                int quadrant = 0;
                double a = 0.0, b = 1.0;  // x = y = 0: sector 0
                if (x >= 0.0 && y > 0.0) { a = x; b = y; }
                else if (x > 0.0 && y <= 0.0) { quadrant = 1; a = -y; b = x; }
                else if (x <= 0.0 && y < 0.0) { quadrant = 2; a = -x; b = -y; }
                else if (x < 0.0 && y >= 0.0) { quadrant = 3; a = y; b = -x; }
                int lo = 0, hi = mq;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (a * bcos[mid] >= b * bsin[mid]) lo = mid;
                    else hi = mid;
                }
                const bool centre = r == 0.0;
                const double vr = centre ? 0.0 : (u * x + v * y) / r, vt = centre ? 0.0 : (v * x - u * y) / r;
                const int bin = min((int)fr, g.n_r - 1) * g.n_theta + quadrant * mq + lo;  // fr inside [0, n_r) already: never trusted
                const unsigned long long s24 = fixed_point(sp, 16777216.0);
                const unsigned long long t[6] = {1ull, s24, fixed_point(qq, 65536.0), fixed_point(vr, 16777216.0), fixed_point(vt, 16777216.0), s24};
                if constexpr (DIRECT) {
                    to_global(bin, t);
                } else {
                    if (bin != cur) {
                        if (cur >= 0) to_table(cur, acc);
                        cur = bin;
#pragma unroll
                        for (int n = 0; n < 6; ++n) acc[n] = 0;
                    }
#pragma unroll
                    for (int n = 0; n < 5; ++n) acc[n] += t[n];
                    acc[5] = acc[5] > t[5] ? acc[5] : t[5];
                }
            }
        }
        if constexpr (!DIRECT)
            if (cur >= 0) to_table(cur, acc);
    }
    if constexpr (!DIRECT) {
        __syncthreads();
        for (int t = threadIdx.x; t < SLOTS; t += 256) {  // (c)
            const int bin = tag[t];
            if (bin < 0) continue;
            const unsigned long long s[6] = {tab[0][t], tab[1][t], tab[2][t], tab[3][t], tab[4][t], tab[5][t]};
            to_global(bin, s);
        }
    }
}

template <typename Src>
static void launch_polar(hipStream_t stream, int path, const Src &src, const void *keep, long long lines, long long samples, const Polar &g,
                         const double *sector_sin, const double *sector_cos, const GridTies &tp, int64_t *sums)
{
    const Strips s = strip_grid(lines, samples);
    const long long lpb = std::max<long long>(s.rows_per_block, XSW_GRID_MIN_LINES);
    const dim3 grid((unsigned)s.gx, (unsigned)((lines + lpb - 1) / lpb));  // as launch_grid
    if (path == GRID_DIRECT)
        hipLaunchKernelGGL((k_wind_polar<Src, true>), grid, dim3(256), 0, stream, src, (const unsigned char *)keep, lines, samples, g, sector_sin,
                           sector_cos, tp, lpb, (unsigned long long *)sums);
    else
        hipLaunchKernelGGL((k_wind_polar<Src, false>), grid, dim3(256), 0, stream, src, (const unsigned char *)keep, lines, samples, g, sector_sin,
                           sector_cos, tp, lpb, (unsigned long long *)sums);
}

// ---- the cyclone centre from the wind field: annulus sums on a lattice of candidate centres (xsw_wind_centre; include/xsw.h has
// the statement).  The sources, the geolocation, the chart and the walk down a column are k_wind_polar's; here a pixel meets EVERY
// candidate and adds its five integers to each one whose annulus it lies in: many bins per pixel, so the stages are the other way
// round -- the pixels are staged, the bins live in registers.
//   DIRECT  a thread owns a pixel, loops over all candidates and sends each hit's five adds to global memory.
//   staged  (a) the walk: a thread computes its pixel's candidate-independent terms (x, y, u, v, Q24(sp), Q16(q)) once; pixels
//               that the drop rule drops, or that lie outside the square |x|, |y| < bound around the lattice, go no further; the
//               survivors of a line are compacted into the workgroup's LDS tile of 48 B entries (a ballot, the lane's rank among
//               the wave's survivors, one LDS add per wave for the wave's base);
//           (b) the sweep, when the tile cannot take another line of 256 entries and at the end of the strip: thread t owns the
//               candidates t, t + 256, ... (at most four: 31 * 31 <= 1024), keeps their five sums in registers across the whole
//               strip and reads the entries one after the other, every lane the same address: broadcast reads, as k_land_mask
//               walks its edges.  A lattice below 256 candidates is owned by 256 / candidates thread groups, group s taking
//               the entries s, s + groups, ...; their partial sums meet by 64-bit LDS adds in the idle tile before (c);
//           (c) the flush: every candidate with n > 0 adds its five words to global memory.
// The cull.  A hit has fl(sqrt(fl(dx * dx + dy * dy))) < r_out, so |dx| < r_out * (1 + 4 ulp); dx = fl(x - cx) and |cx| <=
// fl(h * step_km) for every candidate, so |x| < (fl(h * step_km) + r_out) * (1 + 8 ulp).  bound is that sum, rounded, times
// (1 + 2**-40): a margin of 2**13 ulp where 10 are needed, the same for y.  A NaN coordinate fails the comparison, as it fails the
// annulus test.  The pre-test on rr = dx * dx + dy * dy is conservative in the same way: sqrt is monotone and rounds once, so
// r_in <= sqrt(rr) < r_out needs r_in * r_in * (1 - 2**-50) <= rr <= r_out * r_out * (1 + 2**-50); only then is the root taken.
// tests/centre_ref.py has neither the cull nor the pre-test: equal sums show that they lose nothing.
#ifndef XSW_CENTRE_TILE
#define XSW_CENTRE_TILE 512  // entries of the LDS tile, 48 B each: 24 KiB, two full lines between sweeps
#endif
#ifndef XSW_CENTRE_MAX_LINES
#define XSW_CENTRE_MAX_LINES 64  // a strip is at most this many lines long where the grid allows: the workgroups inside the square do all
                                 // the pair work, and shorter strips spread it over more of them
#endif
#define XSW_CENTRE_MAX_N 31
static_assert(XSW_CENTRE_TILE >= 512 && XSW_CENTRE_TILE * 48 >= 5 * 256 * 8, "a line must fit twice, and the partial sums of a small lattice meet in the tile");
static_assert(XSW_CENTRE_MAX_N * XSW_CENTRE_MAX_N <= 4 * 256, "a thread owns at most four candidates");

// The path of a call.  Environment XSW_CENTRE_PATH = direct forces the direct kernel (tests, measurements); read on the host at every call.
enum { CENTRE_STAGED = 0, CENTRE_DIRECT = 1 };
static int centre_path(bool &bad_env)
{
    bad_env = false;
    if (const char *v = getenv("XSW_CENTRE_PATH")) {
        if (!strcmp(v, "direct")) return CENTRE_DIRECT;
        bad_env = true;
    }
    return CENTRE_STAGED;
}

struct Centre {
    double lon_g, lat_g, cos_g, sin_g, step_km, r_in, r_out;
    double rr_lo, rr_hi, bound;  // the staged path's pre-test on rr and its cull square (launch_centre)
    int n_c;
};

struct alignas(16) CentreEntry {
    double x, y, u, v;
    unsigned long long s24, q16;
};
static_assert(sizeof(CentreEntry) == 48, "the tile's entries are 48 B");

template <typename Src, bool DIRECT>
__global__ __launch_bounds__(256) void k_wind_centre(const Src src, const unsigned char *__restrict__ keep, long long lines, long long samples,
                                                     const Centre g, const GridTies tp, long long lines_per_block,
                                                     unsigned long long *__restrict__ sums)
{
    constexpr int TILE = DIRECT ? 1 : XSW_CENTRE_TILE;
    constexpr double D2R = 0.017453292519943295, R_KM = 6371.0088, KX = R_KM * D2R;
    __shared__ CentreEntry tile[TILE];
    __shared__ int line_count[3];  // the survivors of line n of the strip are counted in word n % 3
    const int tid = threadIdx.x, lane = tid & 63;
    const int nc = min(max(g.n_c, 1), XSW_CENTRE_MAX_N), nc2 = nc * nc, half = (nc - 1) / 2;  // (the entry refuses other sizes: never trusted)
    // (b)'s ownership: `own` candidates first, first + 256, ...; group `slice` of `slices` takes the entries slice, slice + slices, ...
    int own, first = tid, slice = 0, slices = 1;
    if (nc2 < 256) {
        slices = 256 / nc2;
        slice = tid / nc2;
        first = tid - slice * nc2;
        own = slice < slices ? 1 : 0;
    } else {
        own = (nc2 - 1 - tid) / 256 + 1;
    }
    double cx[4], cy[4];
    unsigned long long acc[4][5];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = first + 256 * m, i = c / nc, j = c - i * nc;
        cy[m] = (double)(i - half) * g.step_km;
        cx[m] = (double)(j - half) * g.step_km;
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[m][k] = 0;
    }
    const auto sweep = [&](int count) {
        for (int e = slice; e < count; e += slices) {
            const CentreEntry p = tile[e];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (m >= own) continue;
                const double dx = p.x - cx[m], dy = p.y - cy[m];
                const double rr = dx * dx + dy * dy;
                if (!(rr >= g.rr_lo && rr <= g.rr_hi)) continue;
                const double r = sqrt(rr);
                if (!(g.r_in <= r && r < g.r_out)) continue;
                const bool centre = r == 0.0;
                const double vr = centre ? 0.0 : (p.u * dx + p.v * dy) / r, vt = centre ? 0.0 : (p.v * dx - p.u * dy) / r;
                acc[m][0] += 1ull;
                acc[m][1] += p.s24;
                acc[m][2] += p.q16;
                acc[m][3] += fixed_point(vr, 16777216.0);
                acc[m][4] += fixed_point(vt, 16777216.0);
            }
        }
    };

    const long long col = (long long)blockIdx.x * blockDim.x + tid;
    const bool live = col < samples;  // (no return: the barriers are the whole workgroup's, and so is every loop bound below)
    const long long cc = live ? col : samples - 1;
    const long long l0 = (long long)blockIdx.y * lines_per_block;
    const long long l1 = l0 + lines_per_block < lines ? l0 + lines_per_block : lines;
    const int j0 = min(max(tp.sj0[cc], 0), tp.ns - 1), j1 = min(j0 + 1, tp.ns - 1);
    const double ts = tp.st[cc], ws0 = 1.0 - ts, ws1 = ts;
    const double half_c = 0.5 * g.cos_g;
    int tie_cur = -1;
    TieRows q;
    int fill = 0, word = 0;  // entries in the tile; the word that counts the line at hand
    if constexpr (!DIRECT) {
        if (tid < 3) line_count[tid] = 0;
        __syncthreads();
    }
    for (long long l = l0; l < l1; l += XSW_GRID_LINES) {
        Px px[XSW_GRID_LINES];
#pragma unroll
        for (int k = 0; k < XSW_GRID_LINES; ++k) {
            px[k] = Px{0.0, 0.0, false};
            if (live && l + k < l1) {
                const long long i = (l + k) * samples + col;
                px[k] = src.fetch(i);
                if (keep) px[k].ok = px[k].ok && keep[i] != 0;
            }
        }
#pragma unroll
        for (int k = 0; k < XSW_GRID_LINES; ++k) {
            if (l + k >= l1) break;
            const int i0 = min(max(tp.li0[l + k], 0), tp.nl - 1);
            const double tl = tp.lt[l + k];
            if (i0 != tie_cur) {
                q = tie_rows(tp.tlon, tp.tlat, tp.tcos, tp.tsin, i0, min(i0 + 1, tp.nl - 1), j0, j1, tp.ns, ws0, ws1);
                tie_cur = i0;
            }
            const TiePoint p = tie_point(q, 1.0 - tl, tl);
            const double re = px[k].a, im = px[k].b;
            const double qq = re * re + im * im, sp = sqrt(qq);
            const double u = -(re * p.ch + im * p.sh), v = -(im * p.ch - re * p.sh);
            double dl = p.lon - g.lon_g;
            dl = dl - 360.0 * __builtin_rint(dl / 360.0);
            const double dy = (p.lat - g.lat_g) * D2R, h = 0.5 * dy;
            const double m = (g.cos_g - g.sin_g * h) - half_c * (h * h);
            const double x = (KX * dl) * m, y = R_KM * dy;
            const bool ok = px[k].ok && !(u != u) && !(v != v) && qq < 65536.0;
            if constexpr (DIRECT) {
                if (!ok) continue;
                const unsigned long long s24 = fixed_point(sp, 16777216.0), q16 = fixed_point(qq, 65536.0);
                for (int i = 0; i < nc; ++i) {
                    const double ddy = y - (double)(i - half) * g.step_km;
                    for (int j = 0; j < nc; ++j) {
                        const double ddx = x - (double)(j - half) * g.step_km;
                        const double r = sqrt(ddx * ddx + ddy * ddy);
                        if (!(g.r_in <= r && r < g.r_out)) continue;  // (a NaN radius fails)
                        const bool centre = r == 0.0;
                        const double vr = centre ? 0.0 : (u * ddx + v * ddy) / r, vt = centre ? 0.0 : (v * ddx - u * ddy) / r;
                        unsigned long long *out = sums + i * nc + j;
                        atomicAdd(out, 1ull);
                        atomicAdd(out + nc2, s24);
                        atomicAdd(out + 2 * nc2, q16);
                        atomicAdd(out + 3 * nc2, fixed_point(vr, 16777216.0));
                        atomicAdd(out + 4 * nc2, fixed_point(vt, 16777216.0));
                    }
                }
            } else {
                // (a): fill <= TILE - 256 here and a line has at most 256 survivors, so every index below is inside the tile
                const bool survives = ok && fabs(x) < g.bound && fabs(y) < g.bound;
                const unsigned long long mask = __ballot(survives);
                int base = 0;
                if (lane == 0 && mask) base = atomicAdd(&line_count[word], __popcll(mask));
                base = __shfl(base, 0);
                if (survives) {
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    tile[fill + base + rank] = CentreEntry{x, y, u, v, fixed_point(sp, 16777216.0), fixed_point(qq, 65536.0)};
                }
                __syncthreads();
                fill += min(max(line_count[word], 0), 256);
                // the word of the line after the next: read for the last time before this barrier, added to after the next one
                if (tid == 0) line_count[(word + 2) % 3] = 0;
                word = (word + 1) % 3;
                if (fill > TILE - 256) {  // (b); workgroup-uniform
                    sweep(fill);
                    __syncthreads();  // the tile has been read
                    fill = 0;
                }
            }
        }
    }
    if constexpr (!DIRECT) {
        sweep(fill);
        if (slices > 1) {  // workgroup-uniform: the groups' partial sums meet in the tile, [5][256] words
            unsigned long long *meet = (unsigned long long *)tile;
            __syncthreads();  // the tile has been read
#pragma unroll
            for (int k = 0; k < 5; ++k) meet[k * 256 + tid] = 0;
            __syncthreads();
            if (own && acc[0][0]) {
#pragma unroll
                for (int k = 0; k < 5; ++k) atomicAdd(&meet[k * 256 + first], acc[0][k]);
            }
            __syncthreads();
            if (tid < nc2 && meet[tid]) {  // (c)
#pragma unroll
                for (int k = 0; k < 5; ++k) atomicAdd(sums + k * nc2 + tid, meet[k * 256 + tid]);
            }
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {  // (c)
                if (m >= own || !acc[m][0]) continue;
#pragma unroll
                for (int k = 0; k < 5; ++k) atomicAdd(sums + k * nc2 + first + 256 * m, acc[m][k]);
            }
        }
    }
}

template <typename Src>
static void launch_centre(hipStream_t stream, int path, const Src &src, const void *keep, long long lines, long long samples, const Centre &g,
                          const GridTies &tp, int64_t *sums)
{
    const Strips s = strip_grid(lines, samples);
    const long long cap = std::max<long long>(XSW_CENTRE_MAX_LINES, (lines + 65534) / 65535);  // grid.y stays within 65535
    const long long lpb = std::max<long long>(std::min<long long>(s.rows_per_block, cap), XSW_GRID_MIN_LINES);
    const dim3 grid((unsigned)s.gx, (unsigned)((lines + lpb - 1) / lpb));
    if (path == CENTRE_DIRECT)
        hipLaunchKernelGGL((k_wind_centre<Src, true>), grid, dim3(256), 0, stream, src, (const unsigned char *)keep, lines, samples, g, tp, lpb,
                           (unsigned long long *)sums);
    else
        hipLaunchKernelGGL((k_wind_centre<Src, false>), grid, dim3(256), 0, stream, src, (const unsigned char *)keep, lines, samples, g, tp, lpb,
                           (unsigned long long *)sums);
}

}  // namespace

extern "C" int xsw_wind_grid(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                             int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                             const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                             const double *sample_t, double lon0, double dlon, int32_t n_lon, int32_t periodic, double lat0, double dlat,
                             int32_t n_lat, int64_t *sums)
{
    if (!c) return XSW_EINVAL;
    if (!src) return fail(c, XSW_EINVAL, "wind_grid: no source");
    if (!sums) return fail(c, XSW_EINVAL, "wind_grid: no sums");
    if (src_kind != XSW_CELLS_C128 && src_kind != XSW_CELLS_C64 && src_kind != XSW_CELLS_CODES)
        return fail(c, XSW_EINVAL, "wind_grid: src_kind must be XSW_CELLS_C128, XSW_CELLS_C64 or XSW_CELLS_CODES");
    if (src_kind == XSW_CELLS_CODES && !c->have_co) return fail(c, XSW_ENOLUT, "wind_grid: co-pol codes given but no co-pol LUT on this context");
    if (!tie_lon || !tie_lat || !tie_cos || !tie_sin || !line_first || !line_t || !sample_first || !sample_t || n_tie_lines < 1 || n_tie_samples < 1)
        return fail(c, XSW_EINVAL, "wind_grid: tie points are required: their four grids, both brackets and one point or more per axis");
    if (lines < 1 || samples < 1) return fail(c, XSW_EINVAL, "wind_grid: the raster must have one line and one sample or more");
    if (int rc = check_dims(c, "wind_grid", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    if (!std::isfinite(lon0) || !std::isfinite(lat0) || !std::isfinite(dlon) || !std::isfinite(dlat) || !(dlon > 0.0) || dlat == 0.0)
        return fail(c, XSW_EINVAL, "wind_grid: the grid needs finite edges, dlon > 0 and a finite non-zero dlat");
    if (n_lon < 1 || n_lat < 1 || (int64_t)n_lon * n_lat > 0x7fffffffLL)
        return fail(c, XSW_EINVAL, "wind_grid: n_lon and n_lat must be 1 or more and n_lon * n_lat must fit int32, not %d x %d", (int)n_lon, (int)n_lat);
    if (periodic != 0 && periodic != 1) return fail(c, XSW_EINVAL, "wind_grid: periodic must be 0 or 1");
    bool bad_env;
    const int path = grid_path(bad_env);
    if (bad_env) return fail(c, XSW_EINVAL, "wind_grid: XSW_GRID_PATH must be direct or lds");
    const size_t npx = (size_t)lines * samples, ties = (size_t)n_tie_lines * n_tie_samples * 8;
    const size_t elem = src_kind == XSW_CELLS_C128 ? 16 : src_kind == XSW_CELLS_C64 ? 8 : 4;
    Buf b[11] = {{src, nullptr, npx * elem}, in_buf(keep, npx), {tie_lon, nullptr, ties}, {tie_lat, nullptr, ties}, {tie_cos, nullptr, ties},
                 {tie_sin, nullptr, ties}, {line_first, nullptr, (size_t)lines * 4}, {line_t, nullptr, (size_t)lines * 8},
                 {sample_first, nullptr, (size_t)samples * 4}, {sample_t, nullptr, (size_t)samples * 8},
                 {sums, sums, (size_t)n_lon * n_lat * 40}};  // copied up, added to, copied down
    const LonLat g{lon0, dlon, lat0, dlat, (int)n_lon, (int)n_lat, (int)periodic};
    return run(c, mem, b, [&](Buf (&x)[11]) {
        GridTies tp;
        tp.tlon = (const double *)x[2].dev; tp.tlat = (const double *)x[3].dev; tp.tcos = (const double *)x[4].dev; tp.tsin = (const double *)x[5].dev;
        tp.li0 = (const int *)x[6].dev; tp.lt = (const double *)x[7].dev; tp.sj0 = (const int *)x[8].dev; tp.st = (const double *)x[9].dev;
        tp.nl = n_tie_lines; tp.ns = n_tie_samples;
        int64_t *out = (int64_t *)x[10].dev;
        if (src_kind == XSW_CELLS_C128) { SrcC128 s; s.p = (const double2 *)x[0].dev; launch_grid(c->stream, path, s, x[1].dev, lines, samples, g, tp, out); }
        else if (src_kind == XSW_CELLS_C64) { SrcC64 s; s.p = (const float2 *)x[0].dev; launch_grid(c->stream, path, s, x[1].dev, lines, samples, g, tp, out); }
        else {
            SrcCodes s;
            s.p = (const unsigned *)x[0].dev; s.sol = c->T.sol; s.plane = (long long)c->T.n_w * c->T.n_phi;
            launch_grid(c->stream, path, s, x[1].dev, lines, samples, g, tp, out);
        }
    }, "wind_grid");
}

extern "C" int xsw_wind_polar(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                              int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                              const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                              const double *sample_t, double lon_c, double lat_c, double cos_lat_c, double sin_lat_c, double dr_km, int32_t n_r,
                              int32_t n_theta, const double *sector_sin, const double *sector_cos, int64_t *sums)
{
    if (!c) return XSW_EINVAL;
    if (!src) return fail(c, XSW_EINVAL, "wind_polar: no source");
    if (!sums) return fail(c, XSW_EINVAL, "wind_polar: no sums");
    if (src_kind != XSW_CELLS_C128 && src_kind != XSW_CELLS_C64 && src_kind != XSW_CELLS_CODES)
        return fail(c, XSW_EINVAL, "wind_polar: src_kind must be XSW_CELLS_C128, XSW_CELLS_C64 or XSW_CELLS_CODES");
    if (src_kind == XSW_CELLS_CODES && !c->have_co) return fail(c, XSW_ENOLUT, "wind_polar: co-pol codes given but no co-pol LUT on this context");
    if (!tie_lon || !tie_lat || !tie_cos || !tie_sin || !line_first || !line_t || !sample_first || !sample_t || n_tie_lines < 1 || n_tie_samples < 1)
        return fail(c, XSW_EINVAL, "wind_polar: tie points are required: their four grids, both brackets and one point or more per axis");
    if (lines < 1 || samples < 1) return fail(c, XSW_EINVAL, "wind_polar: the raster must have one line and one sample or more");
    if (int rc = check_dims(c, "wind_polar", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    if (!std::isfinite(lon_c) || !std::isfinite(lat_c) || !(std::fabs(lat_c) <= 89.0))
        return fail(c, XSW_EINVAL, "wind_polar: the centre needs a finite longitude and a latitude within 89 degrees of the equator");
    if (!std::isfinite(cos_lat_c) || !std::isfinite(sin_lat_c)) return fail(c, XSW_EINVAL, "wind_polar: cos and sin of the centre's latitude must be finite");
    if (!std::isfinite(dr_km) || !(dr_km > 0.0)) return fail(c, XSW_EINVAL, "wind_polar: dr_km must be finite and positive");
    if (n_r < 1 || n_theta < 4 || n_theta % 4 != 0 || n_theta > XSW_POLAR_MAX_SECTORS || (int64_t)n_r * n_theta > 0x7fffffffLL)
        return fail(c, XSW_EINVAL, "wind_polar: n_r must be 1 or more, n_theta a multiple of 4 from 4 to %d and n_r * n_theta must fit int32, not %d x %d",
                    XSW_POLAR_MAX_SECTORS, (int)n_r, (int)n_theta);
    if (!sector_sin || !sector_cos) return fail(c, XSW_EINVAL, "wind_polar: the table of sector borders is required");
    bool bad_env;
    const int path = grid_path(bad_env);
    if (bad_env) return fail(c, XSW_EINVAL, "wind_polar: XSW_GRID_PATH must be direct or lds");
    const size_t npx = (size_t)lines * samples, ties = (size_t)n_tie_lines * n_tie_samples * 8, borders = (size_t)(n_theta / 4 + 1) * 8;
    const size_t elem = src_kind == XSW_CELLS_C128 ? 16 : src_kind == XSW_CELLS_C64 ? 8 : 4;
    Buf b[13] = {{src, nullptr, npx * elem}, in_buf(keep, npx), {tie_lon, nullptr, ties}, {tie_lat, nullptr, ties}, {tie_cos, nullptr, ties},
                 {tie_sin, nullptr, ties}, {line_first, nullptr, (size_t)lines * 4}, {line_t, nullptr, (size_t)lines * 8},
                 {sample_first, nullptr, (size_t)samples * 4}, {sample_t, nullptr, (size_t)samples * 8}, {sector_sin, nullptr, borders},
                 {sector_cos, nullptr, borders}, {sums, sums, (size_t)n_r * n_theta * 48}};  // copied up, accumulated into, copied down
    const Polar g{lon_c - 360.0 * std::rint(lon_c / 360.0), lat_c, cos_lat_c, sin_lat_c, dr_km, (int)n_r, (int)n_theta};  // step 0
    return run(c, mem, b, [&](Buf (&x)[13]) {
        GridTies tp;
        tp.tlon = (const double *)x[2].dev; tp.tlat = (const double *)x[3].dev; tp.tcos = (const double *)x[4].dev; tp.tsin = (const double *)x[5].dev;
        tp.li0 = (const int *)x[6].dev; tp.lt = (const double *)x[7].dev; tp.sj0 = (const int *)x[8].dev; tp.st = (const double *)x[9].dev;
        tp.nl = n_tie_lines; tp.ns = n_tie_samples;
        const double *ss = (const double *)x[10].dev, *sc = (const double *)x[11].dev;
        int64_t *out = (int64_t *)x[12].dev;
        if (src_kind == XSW_CELLS_C128) { SrcC128 s; s.p = (const double2 *)x[0].dev; launch_polar(c->stream, path, s, x[1].dev, lines, samples, g, ss, sc, tp, out); }
        else if (src_kind == XSW_CELLS_C64) { SrcC64 s; s.p = (const float2 *)x[0].dev; launch_polar(c->stream, path, s, x[1].dev, lines, samples, g, ss, sc, tp, out); }
        else {
            SrcCodes s;
            s.p = (const unsigned *)x[0].dev; s.sol = c->T.sol; s.plane = (long long)c->T.n_w * c->T.n_phi;
            launch_polar(c->stream, path, s, x[1].dev, lines, samples, g, ss, sc, tp, out);
        }
    }, "wind_polar");
}

extern "C" int xsw_wind_centre(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                               int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                               const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                               const double *sample_t, double lon_g, double lat_g, double cos_lat_g, double sin_lat_g, double step_km, int32_t n_c,
                               double r_in_km, double r_out_km, int64_t *sums)
{
    if (!c) return XSW_EINVAL;
    if (!src) return fail(c, XSW_EINVAL, "wind_centre: no source");
    if (!sums) return fail(c, XSW_EINVAL, "wind_centre: no sums");
    if (src_kind != XSW_CELLS_C128 && src_kind != XSW_CELLS_C64 && src_kind != XSW_CELLS_CODES)
        return fail(c, XSW_EINVAL, "wind_centre: src_kind must be XSW_CELLS_C128, XSW_CELLS_C64 or XSW_CELLS_CODES");
    if (src_kind == XSW_CELLS_CODES && !c->have_co) return fail(c, XSW_ENOLUT, "wind_centre: co-pol codes given but no co-pol LUT on this context");
    if (!tie_lon || !tie_lat || !tie_cos || !tie_sin || !line_first || !line_t || !sample_first || !sample_t || n_tie_lines < 1 || n_tie_samples < 1)
        return fail(c, XSW_EINVAL, "wind_centre: tie points are required: their four grids, both brackets and one point or more per axis");
    if (lines < 1 || samples < 1) return fail(c, XSW_EINVAL, "wind_centre: the raster must have one line and one sample or more");
    if (int rc = check_dims(c, "wind_centre", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    if (!std::isfinite(lon_g) || !std::isfinite(lat_g) || !(std::fabs(lat_g) <= 89.0))
        return fail(c, XSW_EINVAL, "wind_centre: the first guess needs a finite longitude and a latitude within 89 degrees of the equator");
    if (!std::isfinite(cos_lat_g) || !std::isfinite(sin_lat_g)) return fail(c, XSW_EINVAL, "wind_centre: cos and sin of the first guess's latitude must be finite");
    if (n_c < 1 || n_c > XSW_CENTRE_MAX_N || n_c % 2 != 1)
        return fail(c, XSW_EINVAL, "wind_centre: n_c must be odd, from 1 to %d, not %d", XSW_CENTRE_MAX_N, (int)n_c);
    if (n_c > 1 && (!std::isfinite(step_km) || !(step_km > 0.0))) return fail(c, XSW_EINVAL, "wind_centre: step_km must be finite and positive");
    if (!std::isfinite(r_in_km) || !std::isfinite(r_out_km) || !(r_in_km >= 0.0) || !(r_in_km < r_out_km))
        return fail(c, XSW_EINVAL, "wind_centre: the annulus needs finite radii with 0 <= r_in_km < r_out_km");
    bool bad_env;
    const int path = centre_path(bad_env);
    if (bad_env) return fail(c, XSW_EINVAL, "wind_centre: XSW_CENTRE_PATH must be direct, or unset");
    const size_t npx = (size_t)lines * samples, ties = (size_t)n_tie_lines * n_tie_samples * 8;
    const size_t elem = src_kind == XSW_CELLS_C128 ? 16 : src_kind == XSW_CELLS_C64 ? 8 : 4;
    Buf b[11] = {{src, nullptr, npx * elem}, in_buf(keep, npx), {tie_lon, nullptr, ties}, {tie_lat, nullptr, ties}, {tie_cos, nullptr, ties},
                 {tie_sin, nullptr, ties}, {line_first, nullptr, (size_t)lines * 4}, {line_t, nullptr, (size_t)lines * 8},
                 {sample_first, nullptr, (size_t)samples * 4}, {sample_t, nullptr, (size_t)samples * 8},
                 {sums, sums, (size_t)n_c * n_c * 40}};  // copied up, added to, copied down
    Centre g;
    g.lon_g = lon_g - 360.0 * std::rint(lon_g / 360.0);
    g.lat_g = lat_g; g.cos_g = cos_lat_g; g.sin_g = sin_lat_g;
    g.step_km = n_c > 1 ? step_km : 0.0;  // one candidate: the first guess itself, whatever step_km holds
    g.r_in = r_in_km; g.r_out = r_out_km; g.n_c = (int)n_c;
    const double wide = 1.0 + 0x1p-40, up = 1.0 + 0x1p-50, down = 1.0 - 0x1p-50;  // k_wind_centre's comment has the reasons
    g.rr_lo = (r_in_km * r_in_km) * down;
    g.rr_hi = (r_out_km * r_out_km) * up;
    g.bound = ((double)((n_c - 1) / 2) * g.step_km + r_out_km) * wide;
    return run(c, mem, b, [&](Buf (&x)[11]) {
        GridTies tp;
        tp.tlon = (const double *)x[2].dev; tp.tlat = (const double *)x[3].dev; tp.tcos = (const double *)x[4].dev; tp.tsin = (const double *)x[5].dev;
        tp.li0 = (const int *)x[6].dev; tp.lt = (const double *)x[7].dev; tp.sj0 = (const int *)x[8].dev; tp.st = (const double *)x[9].dev;
        tp.nl = n_tie_lines; tp.ns = n_tie_samples;
        int64_t *out = (int64_t *)x[10].dev;
        if (src_kind == XSW_CELLS_C128) { SrcC128 s; s.p = (const double2 *)x[0].dev; launch_centre(c->stream, path, s, x[1].dev, lines, samples, g, tp, out); }
        else if (src_kind == XSW_CELLS_C64) { SrcC64 s; s.p = (const float2 *)x[0].dev; launch_centre(c->stream, path, s, x[1].dev, lines, samples, g, tp, out); }
        else {
            SrcCodes s;
            s.p = (const unsigned *)x[0].dev; s.sol = c->T.sol; s.plane = (long long)c->T.n_w * c->T.n_phi;
            launch_centre(c->stream, path, s, x[1].dev, lines, samples, g, tp, out);
        }
    }, "wind_centre");
}

extern "C" int xsw_wind_cells(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                              int32_t cell_lines, int32_t cell_samples, int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon,
                              const double *tie_lat, const double *tie_cos, const double *tie_sin, const int32_t *line_first, const double *line_t,
                              const int32_t *sample_first, const double *sample_t, int32_t *out_count, double *out_wind, double *out_wspd,
                              double *out_wspd_std, double *out_steadiness, double *out_longitude, double *out_latitude, double *out_u, double *out_v)
{
    if (!c) return XSW_EINVAL;
    if (!src) return fail(c, XSW_EINVAL, "wind_cells: no source");
    if (src_kind != XSW_CELLS_C128 && src_kind != XSW_CELLS_C64 && src_kind != XSW_CELLS_CODES)
        return fail(c, XSW_EINVAL, "wind_cells: src_kind must be XSW_CELLS_C128, XSW_CELLS_C64 or XSW_CELLS_CODES");
    if (src_kind == XSW_CELLS_CODES && !c->have_co) return fail(c, XSW_ENOLUT, "wind_cells: co-pol codes given but no co-pol LUT on this context");
    if (!tie_lon && (out_longitude || out_latitude || out_u || out_v))
        return fail(c, XSW_EINVAL, "wind_cells: longitude, latitude, u and v need tie points");
    if (tie_lon && (!tie_lat || !tie_cos || !tie_sin || !line_first || !line_t || !sample_first || !sample_t || n_tie_lines < 1 || n_tie_samples < 1))
        return fail(c, XSW_EINVAL, "wind_cells: tie points need their four grids, both brackets and one point or more per axis");
    CellGrid g;
    int map;
    if (int rc = plan_cells(c, "wind_cells", lines, samples, mem, cell_lines, cell_samples, g, map)) return rc;
    const size_t npx = (size_t)lines * samples, nc = (size_t)g.ncells, n_lc = nc / (size_t)g.n_sc, n_sc = (size_t)g.n_sc;
    const size_t ties = tie_lon ? (size_t)n_tie_lines * n_tie_samples * 8 : 0;
    const size_t elem = src_kind == XSW_CELLS_C128 ? 16 : src_kind == XSW_CELLS_C64 ? 8 : 4;
    Buf b[19] = {{src, nullptr, npx * elem}, in_buf(keep, npx), in_buf(tie_lon, ties), in_buf(tie_lat, ties), in_buf(tie_cos, ties), in_buf(tie_sin, ties),
                 in_buf(tie_lon ? line_first : nullptr, n_lc * 4), in_buf(tie_lon ? line_t : nullptr, n_lc * 8),
                 in_buf(tie_lon ? sample_first : nullptr, n_sc * 4), in_buf(tie_lon ? sample_t : nullptr, n_sc * 8),
                 out_buf(out_count, nc * 4), out_buf(out_wind, nc * 16), out_buf(out_wspd, nc * 8), out_buf(out_wspd_std, nc * 8),
                 out_buf(out_steadiness, nc * 8), out_buf(out_longitude, nc * 8), out_buf(out_latitude, nc * 8), out_buf(out_u, nc * 8),
                 out_buf(out_v, nc * 8)};
    return run(c, mem, b, [&](Buf (&x)[19]) {
        WindOuts o;
        o.count = (int *)x[10].dev; o.wind = (double2 *)x[11].dev; o.wspd = (double *)x[12].dev; o.wspd_std = (double *)x[13].dev;
        o.steadiness = (double *)x[14].dev; o.lon = (double *)x[15].dev; o.lat = (double *)x[16].dev; o.u = (double *)x[17].dev; o.v = (double *)x[18].dev;
        o.tlon = (const double *)x[2].dev; o.tlat = (const double *)x[3].dev; o.tcos = (const double *)x[4].dev; o.tsin = (const double *)x[5].dev;
        o.li0 = (const int *)x[6].dev; o.lt = (const double *)x[7].dev; o.sj0 = (const int *)x[8].dev; o.st = (const double *)x[9].dev;
        o.nl = n_tie_lines; o.ns = n_tie_samples;
        if (src_kind == XSW_CELLS_C128) { SrcC128 s; s.p = (const double2 *)x[0].dev; launch_cells(c->stream, map, s, x[1].dev, g, o); }
        else if (src_kind == XSW_CELLS_C64) { SrcC64 s; s.p = (const float2 *)x[0].dev; launch_cells(c->stream, map, s, x[1].dev, g, o); }
        else {
            SrcCodes s;
            s.p = (const unsigned *)x[0].dev; s.sol = c->T.sol; s.plane = (long long)c->T.n_w * c->T.n_phi;
            launch_cells(c->stream, map, s, x[1].dev, g, o);
        }
    }, "wind_cells");
}

extern "C" int xsw_raster_cells(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t dtype, const void *x, const uint8_t *keep,
                                int32_t cell_lines, int32_t cell_samples, int32_t *out_count, double *out_mean, double *out_std)
{
    if (!c) return XSW_EINVAL;
    if (!x) return fail(c, XSW_EINVAL, "raster_cells: no source");
    if (dtype != XSW_F32 && dtype != XSW_F64) return fail(c, XSW_EINVAL, "raster_cells: dtype must be XSW_F32 or XSW_F64");
    CellGrid g;
    int map;
    if (int rc = plan_cells(c, "raster_cells", lines, samples, mem, cell_lines, cell_samples, g, map)) return rc;
    const size_t npx = (size_t)lines * samples, nc = (size_t)g.ncells;
    Buf b[5] = {{x, nullptr, npx * (dtype == XSW_F32 ? 4 : 8)}, in_buf(keep, npx), out_buf(out_count, nc * 4), out_buf(out_mean, nc * 8),
                out_buf(out_std, nc * 8)};
    return run(c, mem, b, [&](Buf (&y)[5]) {
        RealOuts o;
        o.count = (int *)y[2].dev; o.mean = (double *)y[3].dev; o.std = (double *)y[4].dev;
        if (dtype == XSW_F32) { SrcReal<float> s; s.p = (const float *)y[0].dev; launch_cells(c->stream, map, s, y[1].dev, g, o); }
        else { SrcReal<double> s; s.p = (const double *)y[0].dev; launch_cells(c->stream, map, s, y[1].dev, g, o); }
    }, "raster_cells");
}
