// Wind-streak direction histograms (Koch 2004; reference: src/xsarsea/gradients.py): the kernels behind
// xsarsea_amd.gradients and their C ABI (the twelve xsw_grad_* entries of include/xsw.h, at the end of this file).
//
//   k_grad_area   f x f box mean (cv2.resize INTER_AREA at an integer factor, Gradients._sigma0_resample :343-367)
//   k_grad_r2     R2 (:689-722): 5x5 B4 "symm" convolution, 2x2 NaN-skipping mean, 3x3 B2 "symm" convolution, optional sqrt;
//                 one 16 x 16 tile of the coarse output per workgroup, the fine input with its halo in LDS
//   k_grad_local  local_gradients (:588-634): Scharr (BORDER_REFLECT_101), grad**2, then R2 of (re, im, |grad**2|) in the
//                 same tiling; writes G2 = sqrt(R2(grad**2)), G3 = R2(|grad**2|) and the quality c
//   k_grad_hist   gradient_histogram (:828-879) of one window per workgroup: exact median of |G2| by radix select on the
//                 float64 bit patterns (integer LDS atomics on counters), then the bin sums in a fixed order (deterministic)
//   k_grad_hist_masked  the same code with a uint8 keep mask on the G2 grid: a pixel whose byte is 0 behaves as a NaN G2
//   k_grad_keep   b x b block reduction of a raster to that keep mask (xsw_grad_keep_f64 / xsw_grad_keep_u8)
//
// and the rain / heterogeneity mask filtering_parameters (:758-825; xsw_grad_r2_sqrt / xsw_grad_local_sqrt / xsw_grad_smooth /
// xsw_grad_mean / xsw_grad_filter):
//   k_grad_r2 / k_grad_local with SQ   the same kernels taking sqrt(sigma0) on load (float32: the float32 root, then widened)
//   k_grad_smooth   smoothing (:675-686, 3x3 B2 "symm"), optionally of the NaN-skipping 2x2 mean of its input (the quarter-
//                   resolution raster smoothing(coarsen(r2)) that filtering_parameters zooms back)
//   k_grad_mean     Mean (:724-755): B4 then B42 (9x9, B4 dilated by 2, its zero taps multiplying), separable, one 32 x 32 tile
//                   with a halo of 6 in LDS per workgroup
//   k_grad_filter   the same Mean on r2, r2**2 and G3 in turn, the bilinear ndimage.zoom(order=1) sample of the quarter
//                   raster, P1..P4 and f1..f4, F; no half-resolution temporary
//
// Every stage reflects at its OWN array's edge, as the reference's chain of separate scipy / xarray calls does.  Sums are
// float64 in a fixed order; -ffp-contract=off (xsarsea_amd/_build.py) keeps them free of contractions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "xsw_host.hpp"
#include "xsw_run.hpp"

namespace {

constexpr int TILE = 16;               // coarse outputs per tile side (k_grad_r2, k_grad_local)
constexpr int FR = 2 * TILE + 8;       // fine rows / columns of a tile: coarse halo +-1, then the 5x5 reach +-2
constexpr int FRP = FR + 1;
constexpr int CH = TILE + 2;           // coarse halo side
constexpr int CHP = CH + 1;
constexpr int AR = FR + 2;             // ampl rows / columns of a k_grad_local tile (the Scharr reach +-1)
constexpr int ARP = AR + 1;
constexpr int HIST_THREADS = 512;
constexpr int HIST_WAVES = HIST_THREADS / 64;
constexpr int HIST_CHUNK = 72;         // bins accumulated per sweep (registers per thread)
constexpr int RADIX_BITS = 11;
constexpr int RADIX = 1 << RADIX_BITS;

// scipy.signal.convolve2d(boundary="symm"): d c b a | a b c d | d c b a  (any overshoot: period 2n)
__host__ __device__ inline long long refl_symm(long long i, long long n)
{
    if (i >= 0 && i < n) return i;  // the common case: no 64-bit remainder
    const long long p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// cv2 BORDER_REFLECT_101: d c b | a b c d | c b a  (period 2n - 2)
__host__ __device__ inline long long refl_101(long long i, long long n)
{
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const long long p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

__device__ inline int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// B4 = B2 * B2 = outer([1,4,6,4,1], [1,4,6,4,1]) / 256 and B2 = outer([1,2,1], [1,2,1]) / 16: dyadic, exact in float64
__device__ inline double b4(int i, int j)
{
    const double w[5] = {1.0, 4.0, 6.0, 4.0, 1.0};
    return w[i] * w[j] * (1.0 / 256.0);
}
__device__ inline double b2(int i, int j)
{
    const double w[3] = {1.0, 2.0, 1.0};
    return w[i] * w[j] * (1.0 / 16.0);
}

// 5x5 B4 at the fine pixel whose window starts at F[y][x]
__device__ inline double conv5(const double (*F)[FRP], int y, int x)
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) s += b4(i, j) * F[y + i][x + j];
    return s;
}

__device__ inline double conv3(const double (*C)[CHP], int y, int x)
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s += b2(i, j) * C[y + i][x + j];
    return s;
}

// coarse halo cell (cy, cx) of the tile at (Y0, X0) holds the coarse pixel symm(Y0 - 1 + cy, L2): its local row in the tile
// (clamped for the cells past a partial tile, whose values are never used)
__device__ inline int halo_src(int c, long long org, long long n) { return clampi(refl_symm(org - 1 + c, n) - (org - 1), 0, CH - 1); }

// ---------------------------------------------------------------------------------------------------------- k_grad_area
template <typename T>
__global__ void k_grad_area(const T *__restrict__ in, T *__restrict__ out, long long S, int f, long long Lo, long long So)
{
    const long long n = Lo * So;
    const double scale = 1.0 / ((double)f * f);
    for (long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x; o < n; o += (long long)gridDim.x * blockDim.x) {
        const long long Y = o / So, X = o - Y * So;
        const T *p = in + Y * f * S + X * f;
        double s = 0.0;
        for (int i = 0; i < f; ++i)
            for (int j = 0; j < f; ++j) s += (double)p[i * S + j];
        out[o] = (T)(s * scale);
    }
}

// square root on load (filtering_parameters: image = np.sqrt(image_ori) in the input's dtype, widened afterwards).  sqrtf is the
// correctly rounded IEEE root here (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt); negative input gives NaN
template <bool SQ>
__device__ inline double load_px(float v) { return SQ ? (double)sqrtf(v) : (double)v; }
template <bool SQ>
__device__ inline double load_px(double v) { return SQ ? sqrt(v) : v; }

// ------------------------------------------------------------------------------------------------------------ k_grad_r2
template <typename T, bool SQ = false>
__global__ __launch_bounds__(256) void k_grad_r2(const T *__restrict__ in, double *__restrict__ out, int L1, int S1, int L2, int S2,
                                                 int take_sqrt)
{
    __shared__ double F[FR][FRP];
    __shared__ double C[CH][CHP];
    const int Y0 = blockIdx.y * TILE, X0 = blockIdx.x * TILE, tid = threadIdx.x;
    const long long fy0 = 2LL * Y0 - 4, fx0 = 2LL * X0 - 4;
    for (int k = tid; k < FR * FR; k += 256) {
        const int ly = k / FR, lx = k - ly * FR;
        F[ly][lx] = load_px<SQ>(in[refl_symm(fy0 + ly, L1) * S1 + refl_symm(fx0 + lx, S1)]);
    }
    __syncthreads();
    for (int k = tid; k < CH * CH; k += 256) {
        const int cy = k / CH, cx = k - cy * CH;
        const int sy = 2 * halo_src(cy, Y0, L2), sx = 2 * halo_src(cx, X0, S2);
        const double v00 = conv5(F, sy, sx), v01 = conv5(F, sy, sx + 1), v10 = conv5(F, sy + 1, sx), v11 = conv5(F, sy + 1, sx + 1);
        // xarray coarsen(...).mean() skips NaN (nanmean): sum of the finite ones / their count; all NaN -> NaN
        int cnt = 0;
        double s = 0.0;
        if (!isnan(v00)) { s += v00; ++cnt; }
        if (!isnan(v01)) { s += v01; ++cnt; }
        if (!isnan(v10)) { s += v10; ++cnt; }
        if (!isnan(v11)) { s += v11; ++cnt; }
        C[cy][cx] = cnt ? s / (double)cnt : __builtin_nan("");
    }
    __syncthreads();
    const int ty = tid / TILE, tx = tid - ty * TILE, Y = Y0 + ty, X = X0 + tx;
    if (Y < L2 && X < S2) {
        const double v = conv3(C, ty, tx);
        out[(long long)Y * S2 + X] = take_sqrt ? sqrt(v) : v;
    }
}

// --------------------------------------------------------------------------------------------------------- k_grad_local
// principal square root, the formula of C99 csqrt (numpy's np.sqrt on complex128)
__device__ inline double2 csqrt_principal(double x, double y)
{
    if (isnan(x) || isnan(y)) return make_double2(__builtin_nan(""), __builtin_nan(""));
    if (x == 0.0 && y == 0.0) return make_double2(0.0, y);
    const double d = hypot(x, y);
    if (x >= 0.0) {
        const double r = sqrt(0.5 * (d + x));
        return make_double2(r, 0.5 * (y / r));
    }
    const double s = sqrt(0.5 * (d - x));
    return make_double2(fabs(0.5 * (y / s)), copysign(s, y));
}

template <typename T = double, bool SQ = false>
__global__ __launch_bounds__(256) void k_grad_local(const T *__restrict__ ampl, double2 *__restrict__ g2, double *__restrict__ g3,
                                                    double *__restrict__ cq, int L1, int S1, int L2, int S2)
{
    // A (ampl with its Scharr halo) is dead once grad**2 is formed: the coarse halo planes reuse its storage
    constexpr int A_DOUBLES = AR * ARP, C_DOUBLES = 3 * CH * CHP;
    static_assert(C_DOUBLES <= A_DOUBLES, "coarse planes must fit in the ampl tile");
    __shared__ double U[A_DOUBLES];
    __shared__ double G[3][FR][FRP];
    double (*A)[ARP] = (double (*)[ARP])U;
    double (*Cr)[CHP] = (double (*)[CHP])U;
    double (*Ci)[CHP] = (double (*)[CHP])(U + CH * CHP);
    double (*Ca)[CHP] = (double (*)[CHP])(U + 2 * CH * CHP);
    const int Y0 = blockIdx.y * TILE, X0 = blockIdx.x * TILE, tid = threadIdx.x;
    const long long ay0 = 2LL * Y0 - 5, ax0 = 2LL * X0 - 5;
    for (int k = tid; k < AR * AR; k += 256) {
        const int ly = k / AR, lx = k - ly * AR;
        A[ly][lx] = load_px<SQ>(ampl[refl_101(ay0 + ly, L1) * S1 + refl_101(ax0 + lx, S1)]);
    }
    __syncthreads();
    // grad**2 at the fine pixel symm(2*Y0 - 4 + ly, L1): A holds ampl at reflect101(q) for the raw rows q = r - 1 .. r + 1
    for (int k = tid; k < FR * FR; k += 256) {
        const int ly = k / FR, lx = k - ly * FR;
        const int r = clampi(refl_symm(2LL * Y0 - 4 + ly, L1) - ay0, 1, AR - 2);
        const int q = clampi(refl_symm(2LL * X0 - 4 + lx, S1) - ax0, 1, AR - 2);
        // cv2.Scharr(CV_64F) as the separable row-then-column filter; every tap multiplies (NaN covers the 3x3 footprint)
        double hx[3], hy[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double *row = &A[r - 1 + d][q - 1];
            hx[d] = -1.0 * row[0] + 0.0 * row[1] + 1.0 * row[2];
            hy[d] = 3.0 * row[0] + 10.0 * row[1] + 3.0 * row[2];
        }
        double dx = 3.0 * hx[0] + 10.0 * hx[1] + 3.0 * hx[2];
        double dy = -1.0 * hy[0] + 0.0 * hy[1] + 1.0 * hy[2];
        if (isnan(dx) || isnan(dy)) dx = dy = __builtin_nan("");  // grad = dx + 1j*dy: one NaN part makes both NaN
        const double re = dx * dx - dy * dy, im = dx * dy + dy * dx;
        G[0][ly][lx] = re;
        G[1][ly][lx] = im;
        G[2][ly][lx] = hypot(re, im);
    }
    __syncthreads();
    for (int k = tid; k < CH * CH; k += 256) {
        const int cy = k / CH, cx = k - cy * CH;
        const int sy = 2 * halo_src(cy, Y0, L2), sx = 2 * halo_src(cx, X0, S2);
        double vr[4], vi[4], va[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            vr[a] = conv5(G[0], sy + (a >> 1), sx + (a & 1));
            vi[a] = conv5(G[1], sy + (a >> 1), sx + (a & 1));
            va[a] = conv5(G[2], sy + (a >> 1), sx + (a & 1));
        }
        // nanmean: complex values are skipped when either part is NaN
        int nc = 0, na = 0;
        double sr = 0.0, si = 0.0, sa = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (!isnan(vr[a]) && !isnan(vi[a])) { sr += vr[a]; si += vi[a]; ++nc; }
            if (!isnan(va[a])) { sa += va[a]; ++na; }
        }
        Cr[cy][cx] = nc ? sr / (double)nc : __builtin_nan("");
        Ci[cy][cx] = nc ? si / (double)nc : __builtin_nan("");
        Ca[cy][cx] = na ? sa / (double)na : __builtin_nan("");
    }
    __syncthreads();
    const int ty = tid / TILE, tx = tid - ty * TILE, Y = Y0 + ty, X = X0 + tx;
    if (Y < L2 && X < S2) {
        const double zr = conv3(Cr, ty, tx), zi = conv3(Ci, ty, tx), za = conv3(Ca, ty, tx);
        const long long o = (long long)Y * S2 + X;
        if (g2) g2[o] = csqrt_principal(zr, zi);
        g3[o] = za;
        const double c = hypot(zr, zi) / (za + 0.00001);
        cq[o] = c <= 1.0 ? c : 0.0;  // c.where(c <= 1).fillna(0): above 1 or NaN -> 0
    }
}

// ---------------------------------------------------------------------------------------------------------- k_grad_hist
struct HistWin {
    long long r0, c0;  // first raster row / column of the window inside the raster
    int nr, nc;        // window rows / columns inside the raster (the rest is NaN padding: never kept)
};

// MASKED: the keep byte is read before the 16-byte G2 load, so a masked-out pixel costs 1 B
template <bool MASKED>
__device__ inline bool kept(const double2 *g2, const uint8_t *keep, const HistWin &h, long long S, int p, double &a)
{
    const int i = p / h.nc, j = p - i * h.nc;
    const long long o = (h.r0 + i) * S + h.c0 + j;
    if (MASKED && !keep[o]) return false;
    const double2 z = g2[o];
    a = hypot(z.x, z.y);
    return !isnan(a) && a > 0.0;
}

__device__ inline unsigned long long bits_of(double a)
{
    return (unsigned long long)__double_as_longlong(a);
}

// One window per workgroup.  Rows / columns outside the raster are the NaN padding of xarray's rolling(center=True): they
// count in the window's size (wl*ws) and are never kept, so only the clipped rectangle is read.  weight receives the bin sums
// (gradient_histogram's `grads`), divided by the window's pixel count when `normalise` (Gradients2D.histogram :118-120).
// MASKED: `keep` (L x S bytes) removes the pixels whose byte is 0 exactly as a NaN G2 would: not kept, so outside the median,
// the bins and used_ratio's numerator.  The thread -> pixel assignment and every summation order are the same in both forms.
template <bool MASKED>
__device__ __forceinline__ void hist_window(const double2 *__restrict__ g2, const double *__restrict__ cq, const uint8_t *__restrict__ keep, int L,
                                            int S, int wl, int ws, const int *__restrict__ rows, int n_rows, const int *__restrict__ cols, int n_cols,
                                            int n_angles, double start, double step, int normalise, double *__restrict__ weight,
                                            double *__restrict__ used_ratio)
{
    __shared__ unsigned hist[2][RADIX];
    __shared__ unsigned long long s_prefix[2];
    __shared__ long long s_rank[2];
    __shared__ long long s_n;
    __shared__ double s_wave[HIST_WAVES][HIST_CHUNK];
    const int win = blockIdx.x, wr = win / n_cols, wc = win - wr * n_cols, tid = threadIdx.x;
    HistWin h;
    {
        const long long r0 = (long long)rows[wr] - wl / 2, c0 = (long long)cols[wc] - ws / 2;
        const long long ra = r0 < 0 ? 0 : r0, rb = r0 + wl > L ? L : r0 + wl;
        const long long ca = c0 < 0 ? 0 : c0, cb = c0 + ws > S ? S : c0 + ws;
        h.r0 = ra;
        h.c0 = ca;
        h.nr = rb > ra ? (int)(rb - ra) : 0;
        h.nc = cb > ca ? (int)(cb - ca) : 0;
    }
    const int np = h.nr * h.nc;  // < 2^31: the window side is bounded by the raster's (checked on the host)
    const double wpix = (double)wl * (double)ws;

    // ---- exact median of the kept |G2|: radix select of ranks (n-1)/2 and n/2 over the bit patterns (non-negative doubles
    // order as their bits), 11-bit digits from the top
    if (tid == 0) { s_prefix[0] = s_prefix[1] = 0; s_rank[0] = s_rank[1] = -1; s_n = 0; }
    for (int shift = 64 - RADIX_BITS, pass = 0; shift > -RADIX_BITS; shift -= RADIX_BITS, ++pass) {
        const int sh = shift < 0 ? 0 : shift;
        const int width = shift < 0 ? RADIX_BITS + shift : RADIX_BITS;
        const unsigned dmask = (1u << width) - 1;
        for (int k = tid; k < 2 * RADIX; k += HIST_THREADS) (&hist[0][0])[k] = 0;
        __syncthreads();
        const unsigned long long pmask = (shift + RADIX_BITS >= 64) ? 0ull : ~0ull << (sh + width);
        const unsigned long long p0 = s_prefix[0], p1 = s_prefix[1];
        const bool same = p0 == p1;
        for (int p = tid; p < np; p += HIST_THREADS) {
            double a;
            if (!kept<MASKED>(g2, keep, h, S, p, a)) continue;
            const unsigned long long key = bits_of(a);
            const unsigned d = (unsigned)(key >> sh) & dmask;
            if ((key & pmask) == p0) atomicAdd(&hist[0][d], 1u);
            if (!same && (key & pmask) == p1) atomicAdd(&hist[1][d], 1u);
        }
        __syncthreads();
        if (tid < 128) {  // wave 0 resolves rank (n-1)/2, wave 1 rank n/2: a wave-wide scan of 32 counters per lane
            const int sel = tid >> 6, lane = tid & 63;
            const unsigned *hh = hist[same ? 0 : sel];
            long long mine = 0;
            for (int k = 0; k < RADIX / 64; ++k) mine += hh[lane * (RADIX / 64) + k];
            long long incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                const long long o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            long long rank;
            if (pass == 0) {
                const long long n = __shfl(incl, 63, 64);
                rank = sel == 0 ? (n - 1) / 2 : n / 2;
                if (lane == 0 && sel == 0) s_n = n;
            } else {
                rank = s_rank[sel];
            }
            const long long excl = incl - mine;
            const bool here = rank >= excl && rank < incl;
            const unsigned long long ball = __ballot(here);
            if (ball && lane == __ffsll((long long)ball) - 1) {
                long long r = rank - excl;
                int d = lane * (RADIX / 64);
                while (r >= (long long)hh[d]) r -= hh[d++];
                s_rank[sel] = r;
                s_prefix[sel] |= (unsigned long long)d << sh;
            }
        }
        __syncthreads();
        if (s_n == 0) break;  // nothing kept: the bin sums are all zero
    }
    const long long n = s_n;
    double m = 0.0;
    if (n > 0) {
        const double lo = __longlong_as_double((long long)s_prefix[0]), hi = __longlong_as_double((long long)s_prefix[1]);
        m = (n & 1) ? lo : (lo + hi) / 2.0;  // numpy's median of an even count: the mean of the two middle values
    }

    // ---- bin sums: every kept pixel adds |g2| / (|g2| + m) * c into bin rint((angle - start) / step) (round half to even,
    // numpy's round); bin n_angles (angle = +pi/2) folds onto bin 0, bins -n_angles .. -1 are numpy's negative indices, and a
    // pixel whose bin lies outside -n_angles .. n_angles (a non-principal g2 only) is skipped, never written.  Each
    // thread sums its own pixels in order, the waves reduce by a fixed butterfly, then the 8 wave sums add in wave order:
    // the result does not depend on scheduling.
    const int lane = tid & 63, wave = tid >> 6;
    for (int b0 = 0; b0 < n_angles; b0 += HIST_CHUNK) {
        double acc[HIST_CHUNK];
#pragma unroll
        for (int b = 0; b < HIST_CHUNK; ++b) acc[b] = 0.0;
        if (n > 0) {
            for (int p = tid; p < np; p += HIST_THREADS) {
                double a;
                if (!kept<MASKED>(g2, keep, h, S, p, a)) continue;
                const int i = p / h.nc, j = p - i * h.nc;
                const long long o = (h.r0 + i) * S + h.c0 + j;
                const double2 z = g2[o];
                const double v = a / (a + m) * cq[o];
                if (isnan(v)) continue;
                long long k = (long long)rint((atan2(z.y, z.x) - start) / step);
                if (k == n_angles) k = 0;        // angle +pi/2 == -pi/2 (mod pi): the one deliberate deviation
                else if (k < 0) k += n_angles;   // numpy's negative index, -n_angles .. -1
                if (k < 0 || k >= n_angles) continue;  // outside numpy's range: the reference raises IndexError (only a
                                                       // non-principal g2 gets here; gradient_histogram checks on the host)
                const int kb = (int)k - b0;
#pragma unroll
                for (int b = 0; b < HIST_CHUNK; ++b) acc[b] += kb == b ? v : 0.0;
            }
        }
#pragma unroll
        for (int b = 0; b < HIST_CHUNK; ++b) {
            double s = acc[b];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) s_wave[wave][b] = s;
        }
        __syncthreads();
        if (tid < HIST_CHUNK && b0 + tid < n_angles) {
            double s = 0.0;
            for (int v = 0; v < HIST_WAVES; ++v) s += s_wave[v][tid];
            weight[(long long)win * n_angles + b0 + tid] = normalise ? s / wpix : s;
        }
        __syncthreads();
    }
    if (tid == 0) used_ratio[win] = (double)n / wpix;
}

__global__ __launch_bounds__(HIST_THREADS) void k_grad_hist(const double2 *__restrict__ g2, const double *__restrict__ cq, int L, int S,
                                                            int wl, int ws, const int *__restrict__ rows, int n_rows, const int *__restrict__ cols,
                                                            int n_cols, int n_angles, double start, double step, int normalise,
                                                            double *__restrict__ weight, double *__restrict__ used_ratio)
{
    hist_window<false>(g2, cq, nullptr, L, S, wl, ws, rows, n_rows, cols, n_cols, n_angles, start, step, normalise, weight, used_ratio);
}

__global__ __launch_bounds__(HIST_THREADS) void k_grad_hist_masked(const double2 *__restrict__ g2, const double *__restrict__ cq,
                                                                   const uint8_t *__restrict__ keep, int L, int S, int wl, int ws,
                                                                   const int *__restrict__ rows, int n_rows, const int *__restrict__ cols, int n_cols,
                                                                   int n_angles, double start, double step, int normalise,
                                                                   double *__restrict__ weight, double *__restrict__ used_ratio)
{
    hist_window<true>(g2, cq, keep, L, S, wl, ws, rows, n_rows, cols, n_cols, n_angles, start, step, normalise, weight, used_ratio);
}

// ---------------------------------------------------------------------------------------------------------- k_grad_keep
// out[Y][X] = 1 iff every input of the b x b block (Y, X) is usable (and and_with[Y][X] != 0 when given), the remainder of the
// raster trimmed.  Usable: x >= threshold for double (an IEEE comparison: NaN is not usable), non-zero for uint8.
// A pure streaming pass shaped as k_detrend: grid.x tiles the output columns (one per thread), grid.y tiles blocks of output
// rows, and a thread streams down its rows.  Each row of a block is read in vectors of W bytes (the host picks the widest W
// that divides the block's row bytes and the raster's row bytes and to which the base is aligned: 16 for the even-width F
// raster at b = 2); the loads of one output are independent of each other and of the next output's.
template <int W> struct KeepVec;
template <> struct KeepVec<16> { typedef uint4 type; };
template <> struct KeepVec<8> { typedef uint2 type; };
template <> struct KeepVec<4> { typedef unsigned type; };
template <> struct KeepVec<1> { typedef uint8_t type; };

__device__ inline bool word_nonzero_bytes(unsigned w) { return ((w - 0x01010101u) & ~w & 0x80808080u) == 0; }  // no zero byte

template <typename T>
struct KeepTest;
template <>
struct KeepTest<double> {
    double thr;
    __device__ bool ok(uint4 v) const
    {
        const double a = __hiloint2double((int)v.y, (int)v.x), b = __hiloint2double((int)v.w, (int)v.z);
        return (a >= thr) & (b >= thr);
    }
    __device__ bool ok(uint2 v) const { return __hiloint2double((int)v.y, (int)v.x) >= thr; }
};
template <>
struct KeepTest<uint8_t> {
    __device__ bool ok(uint4 v) const
    {
        return word_nonzero_bytes(v.x) & word_nonzero_bytes(v.y) & word_nonzero_bytes(v.z) & word_nonzero_bytes(v.w);
    }
    __device__ bool ok(uint2 v) const { return word_nonzero_bytes(v.x) & word_nonzero_bytes(v.y); }
    __device__ bool ok(unsigned v) const { return word_nonzero_bytes(v); }
    __device__ bool ok(uint8_t v) const { return v != 0; }
};

// S: input row length in elements; nv = b * sizeof(T) / W vectors per block row.  B != 0 fixes b = B and nv = 1 at compile time
// (the F raster's 2 x 2 blocks of doubles, 16 B per block row): four output rows, eight loads, in flight per lane.
template <typename T, int W, int B>
__global__ __launch_bounds__(256) void k_grad_keep(const T *__restrict__ in, const uint8_t *__restrict__ and_with, uint8_t *__restrict__ out,
                                                   long long S, int b, int nv, long long Lo, long long So, long long rows_per_block,
                                                   KeepTest<T> test)
{
    typedef typename KeepVec<W>::type vec_t;
    const long long X = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= So) return;
    const long long y0 = (long long)blockIdx.y * rows_per_block;
    const long long y1 = y0 + rows_per_block < Lo ? y0 + rows_per_block : Lo;
    const int bb = B ? B : b, nvv = B ? 1 : nv;
    const long long row_vecs = S * (long long)sizeof(T) / W;  // W divides the row bytes
    const vec_t *col = (const vec_t *)in + X * nvv;
#pragma unroll B ? 4 : 1
    for (long long Y = y0; Y < y1; ++Y) {
        const vec_t *p = col + Y * bb * row_vecs;
        bool ok = and_with ? and_with[Y * So + X] != 0 : true;
#pragma unroll B ? B : 2
        for (int i = 0; i < bb; ++i, p += row_vecs)
#pragma unroll B ? 1 : 2
            for (int k = 0; k < nvv; ++k) ok &= test.ok(p[k]);
        out[Y * So + X] = ok ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------- k_grad_smooth / mean / filter
// NaN-skipping 2x2 mean of `in` (row length S) at the coarse pixel (y, x): xarray coarsen(trim).mean()
__device__ inline double coarsen_at(const double *__restrict__ in, long long S, long long y, long long x)
{
    const double *p = in + 2 * y * S + 2 * x;
    const double v[4] = {p[0], p[1], p[S], p[S + 1]};
    int cnt = 0;
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (!isnan(v[a])) { s += v[a]; ++cnt; }
    return cnt ? s / (double)cnt : __builtin_nan("");
}

// smoothing (:675-686): out = convolve2d(x, B2, "symm") on the Lo x So raster x, which is `in` itself or, with COARSEN, the
// NaN-skipping 2x2 mean of `in` (rows of S pixels, remainder trimmed).  One output per thread, the 3x3 taps from the cache.
template <bool COARSEN>
__global__ __launch_bounds__(256) void k_grad_smooth(const double *__restrict__ in, double *__restrict__ out, int S, int Lo, int So)
{
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (Y >= Lo || X >= So) return;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const long long y = refl_symm((long long)Y - 1 + i, Lo);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long x = refl_symm((long long)X - 1 + j, So);
            s += b2(i, j) * (COARSEN ? coarsen_at(in, S, y, x) : in[y * S + x]);
        }
    }
    out[(long long)Y * So + X] = s;
}

// Mean (:724-755) of one channel on a 32 x 32 tile: convolve2d(B4, "symm") then convolve2d(B42, "symm"), each reflecting at
// the raster's own edge, both separable (B4 = w5 x w5, B42 = w9 x w9 with w9 = w5 dilated by 2).  The zero taps of w9 multiply,
// as scipy's direct sum does: a NaN or Inf anywhere in the 9 x 9 footprint gives NaN.
constexpr int MT = 32;            // outputs per tile side
constexpr int MX = MT + 12;       // staged side: halo 2 (B4) + 4 (B42)
constexpr int MM = MT + 8;        // side after B4: halo 4
constexpr int MXP = MX + 1, MMP = MM + 1;

struct MeanLds {
    double A[MX * MXP];  // the staged channel, then (stride MMP) the B4 result
    double B[MX * MMP];  // row pass of B4, then row pass of B42
    int sy[MM], sx[MM];  // first staged row / column of the B4 taps of each cell of the B4 result
};

__device__ inline double w5(int i)
{
    const double w[5] = {1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16};
    return w[i];
}
__device__ inline double w9(int i)
{
    const double w[9] = {1.0 / 16, 0.0, 4.0 / 16, 0.0, 6.0 / 16, 0.0, 4.0 / 16, 0.0, 1.0 / 16};
    return w[i];
}

// Cell m of the B4 result holds Mean-stage-1 at the raster index symm(org - 4 + m, n): the taps of that index start at its
// staged cell - 2 (the staged cell l holds the input at symm(org - 6 + l, n), so the taps reflect at the input's edge).  Cells
// past a partial tile are clamped; their values are never used.
__device__ inline void mean_setup(MeanLds &t, int Y0, int X0, int L, int S)
{
    for (int m = threadIdx.x; m < 2 * MM; m += 256) {
        const int k = m < MM ? m : m - MM;
        const long long org = m < MM ? Y0 : X0, n = m < MM ? L : S;
        const int v = clampi(refl_symm(org - 4 + k, n) - (org - 6), 2, MX - 3) - 2;
        if (m < MM) t.sy[k] = v; else t.sx[k] = v;
    }
}

// Mean of the channel load(y, x) at the thread's four outputs (rows threadIdx.x / 32 + 8 * o, column threadIdx.x % 32)
template <typename Load>
__device__ inline void mean_tile(MeanLds &t, Load load, int Y0, int X0, int L, int S, double (&out)[4])
{
    const int tid = threadIdx.x;
    for (int k = tid; k < MX * MX; k += 256) {
        const int ly = k / MX, lx = k - ly * MX;
        t.A[ly * MXP + lx] = load(refl_symm((long long)Y0 - 6 + ly, L), refl_symm((long long)X0 - 6 + lx, S));
    }
    __syncthreads();  // also orders mean_setup's writes and the previous channel's reads of B
    for (int k = tid; k < MX * MM; k += 256) {
        const int r = k / MM, mx = k - r * MM;
        const double *a = &t.A[r * MXP + t.sx[mx]];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 5; ++j) s += w5(j) * a[j];
        t.B[r * MMP + mx] = s;
    }
    __syncthreads();
    for (int k = tid; k < MM * MM; k += 256) {
        const int my = k / MM, mx = k - my * MM;
        const double *b = &t.B[t.sy[my] * MMP + mx];
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) s += w5(i) * b[i * MMP];
        t.A[my * MMP + mx] = s;
    }
    __syncthreads();
    for (int k = tid; k < MM * MT; k += 256) {
        const int my = k / MT, tx = k - my * MT;
        const double *a = &t.A[my * MMP + tx];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) s += w9(j) * a[j];
        t.B[my * MMP + tx] = s;
    }
    __syncthreads();
    const int ty = tid >> 5, tx = tid & 31;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const double *b = &t.B[(ty + 8 * o) * MMP + tx];
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) s += w9(i) * b[i * MMP];
        out[o] = s;
    }
}

__global__ __launch_bounds__(256) void k_grad_mean(const double *__restrict__ in, double *__restrict__ out, int L, int S)
{
    __shared__ MeanLds t;
    const int Y0 = blockIdx.y * MT, X0 = blockIdx.x * MT;
    double m[4];
    mean_setup(t, Y0, X0, L, S);
    mean_tile(t, [&](long long y, long long x) { return in[y * S + x]; }, Y0, X0, L, S, m);
    const int X = X0 + (threadIdx.x & 31);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int Y = Y0 + (threadIdx.x >> 5) + 8 * o;
        if (Y < L && X < S) out[(long long)Y * S + X] = m[o];
    }
}

// One axis of scipy.ndimage.zoom(order=1, mode="constant", grid_mode=False): output index o reads the input coordinate
// o * z, z = (n_in - 1) / (n_out - 1); taps floor and floor + 1 with weights 1 - t and 1 - (1 - t).  A tap past the last
// element (the last output, where its weight is 0) is mirrored to n - 2 (index 0 for a one-element axis) and still
// multiplies.  A coordinate beyond n - 1 would be outside (cval 0): it does not occur for n_out in {2 n, 2 n + 1}, n <= 20000.
struct ZoomTap {
    int i0, i1;
    double w0, w1;
    bool inside;
};
__device__ inline ZoomTap zoom_tap(int o, double z, int n)
{
    ZoomTap t;
    const double cc = (double)o * z, fl = floor(cc);
    t.inside = cc <= (double)(n - 1);
    t.i0 = t.inside ? (int)fl : 0;
    t.i1 = t.i0 + 1 < n ? t.i0 + 1 : (n > 1 ? n - 2 : 0);
    t.w0 = 1.0 - (cc - fl);
    t.w1 = 1.0 - t.w0;
    return t;
}

__device__ inline double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }  // np.clip: NaN passes

// filtering_parameters (:780-819) from r2 = R2(ampl), G3 and c of local_gradients(ampl) (L x S) and the quarter-resolution
// q4 = smoothing(coarsen(r2)) (L4 x S4): out is [5][L][S] = f1, f2, f3, f4, F.
__global__ __launch_bounds__(256) void k_grad_filter(const double *__restrict__ r2, const double *__restrict__ g3, const double *__restrict__ cq,
                                                     const double *__restrict__ q4, double *__restrict__ out, int L, int S, int L4, int S4,
                                                     double zy, double zx)
{
    __shared__ MeanLds t;
    const int Y0 = blockIdx.y * MT, X0 = blockIdx.x * MT;
    double J[4], J1[4], G4[4];
    mean_setup(t, Y0, X0, L, S);
    // the three channels r2, r2**2, G3 in turn through one copy of the tile code (unrolled, it costs 230 VGPRs)
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        const double *src = ch == 2 ? g3 : r2;
        double m[4];
        mean_tile(t, [&](long long y, long long x) { const double v = src[y * S + x]; return ch == 1 ? v * v : v; }, Y0, X0, L, S, m);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (ch == 0) J[o] = m[o];
            else if (ch == 1) J1[o] = m[o];
            else G4[o] = m[o];
        }
    }
    const int X = X0 + (threadIdx.x & 31);
    const long long plane = (long long)L * S;
    const ZoomTap tx = zoom_tap(X, zx, S4);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int Y = Y0 + (threadIdx.x >> 5) + 8 * o;
        if (Y >= L || X >= S) continue;
        const long long p = (long long)Y * S + X;
        const double r = r2[p];
        // P1 = sqrt(Mean(r2**2) - Mean(r2)**2) / (Mean(r2) + 1e-5): a negative difference is NaN, as numpy's
        const double P1 = sqrt(J1[o] - J[o] * J[o]) / (J[o] + 0.00001);
        // P2 = (r2 - zoom(q4))**2 / (J**2 + 1e-5); scipy's tap order: ((a00 wy0) wx0 + (a01 wy0) wx1) + (a10 wy1) wx0 + (a11 wy1) wx1
        const ZoomTap ty = zoom_tap(Y, zy, L4);
        double z = 0.0;
        if (ty.inside && tx.inside) {
            const double *q0 = q4 + (long long)ty.i0 * S4, *q1 = q4 + (long long)ty.i1 * S4;
            z += q0[tx.i0] * ty.w0 * tx.w0;
            z += q0[tx.i1] * ty.w0 * tx.w1;
            z += q1[tx.i0] * ty.w1 * tx.w0;
            z += q1[tx.i1] * ty.w1 * tx.w1;
        }
        const double K = r - z;
        const double P2 = K * K / (J[o] * J[o] + 0.00001);
        const double P3 = g3[p] / (G4[o] + 0.00001);
        const double P4 = sqrt(cq[p]);
        const double f1 = clip01(-50.0 * P1 + 2.75), f2 = clip01(-5000.0 * P2 + 3.0);
        const double f3 = clip01(-2.5 * P3 + 4.0), f4 = clip01(-10.0 * P4 + 6.3);
        out[p] = f1;
        out[plane + p] = f2;
        out[2 * plane + p] = f3;
        out[3 * plane + p] = f4;
        out[4 * plane + p] = sqrt(1.0 / 4.0 * (f1 * f1 + f2 * f2 + f3 * f3 + f4 * f4));
    }
}

}  // namespace

extern "C" int xsw_grad_area(xsw_ctx *c, int64_t lines, int64_t samples, int32_t factor, int32_t dtype, int32_t mem, const void *in,
                             void *out)
{
    if (!c) return XSW_EINVAL;
    if (!in || !out || factor < 1 || lines < factor || samples < factor) return fail(c, XSW_EINVAL, "grad_area: bad argument");
    if (dtype != XSW_F32 && dtype != XSW_F64) return fail(c, XSW_EINVAL, "dtype must be XSW_F32 or XSW_F64");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const long long Lo = lines / factor, So = samples / factor, es = dtype == XSW_F32 ? 4 : 8;
    Buf b[2] = {{in, nullptr, (size_t)(lines * samples * es)}, {nullptr, out, (size_t)(Lo * So * es)}};
    const long long nblk = std::min<long long>((Lo * So + 255) / 256, 65536);
    return run(c, mem, b, [&](Buf (&x)[2]) {
        if (dtype == XSW_F32)
            hipLaunchKernelGGL(k_grad_area<float>, dim3((unsigned)nblk), dim3(256), 0, c->stream, (const float *)x[0].dev, (float *)x[1].dev,
                               (long long)samples, (int)factor, Lo, So);
        else
            hipLaunchKernelGGL(k_grad_area<double>, dim3((unsigned)nblk), dim3(256), 0, c->stream, (const double *)x[0].dev, (double *)x[1].dev,
                               (long long)samples, (int)factor, Lo, So);
    }, "grad_area");
}

// xsw_grad_r2 (SQ false: take_sqrt roots the result) and xsw_grad_r2_sqrt (SQ true: the kernel roots sigma0 on load).  SQ is a
// template flag so that each entry instantiates its own kernels where it stands, as it did: their order in the code object.
template <bool SQ>
static int grad_r2(xsw_ctx *c, const char *what, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, int32_t take_sqrt,
                   const void *in, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!in || !out || lines < 2 || samples < 2) return fail(c, XSW_EINVAL, "%s: bad argument (the raster needs 2 x 2 pixels)", what);
    if (int rc = check_dims(c, what, lines, samples)) return rc;
    if (dtype != XSW_F32 && dtype != XSW_F64) return fail(c, XSW_EINVAL, "dtype must be XSW_F32 or XSW_F64");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const int L1 = (int)lines, S1 = (int)samples, L2 = L1 / 2, S2 = S1 / 2, root = (int)(take_sqrt != 0);
    const long long es = dtype == XSW_F32 ? 4 : 8;
    Buf b[2] = {{in, nullptr, (size_t)(lines * samples * es)}, {nullptr, out, (size_t)L2 * S2 * 8}};
    const dim3 grid((S2 + TILE - 1) / TILE, (L2 + TILE - 1) / TILE);
    if (int rc = check_grid(c, what, grid)) return rc;
    return run(c, mem, b, [&](Buf (&x)[2]) {
        if (dtype == XSW_F32)
            hipLaunchKernelGGL((k_grad_r2<float, SQ>), grid, dim3(256), 0, c->stream, (const float *)x[0].dev, (double *)x[1].dev, L1, S1, L2, S2,
                               root);
        else
            hipLaunchKernelGGL((k_grad_r2<double, SQ>), grid, dim3(256), 0, c->stream, (const double *)x[0].dev, (double *)x[1].dev, L1, S1, L2, S2,
                               root);
    }, what);
}

extern "C" int xsw_grad_r2(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, int32_t take_sqrt, const void *in,
                           double *out)
{
    return grad_r2<false>(c, "grad_r2", lines, samples, dtype, mem, take_sqrt, in, out);
}

// xsw_grad_local (SQ false: float64 ampl, g2 required) and xsw_grad_local_sqrt (SQ true: sqrt(sigma0) on load, g2 optional).
template <bool SQ>
static int grad_local(xsw_ctx *c, const char *what, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *in,
                      double *g2, double *g3, double *quality)
{
    if (!c) return XSW_EINVAL;
    if (!in || (!g2 && !SQ) || !g3 || !quality || lines < 2 || samples < 2)
        return fail(c, XSW_EINVAL, "%s: bad argument (the raster needs 2 x 2 pixels)", what);
    if (int rc = check_dims(c, what, lines, samples)) return rc;
    if (dtype != XSW_F32 && dtype != XSW_F64) return fail(c, XSW_EINVAL, "dtype must be XSW_F32 or XSW_F64");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const int L1 = (int)lines, S1 = (int)samples, L2 = L1 / 2, S2 = S1 / 2;
    const size_t no = (size_t)L2 * S2;
    const long long es = dtype == XSW_F32 ? 4 : 8;
    Buf b[4] = {{in, nullptr, (size_t)(lines * samples * es)}, {nullptr, g3, no * 8}, {nullptr, quality, no * 8}, {nullptr, g2, g2 ? no * 16 : 0}};
    const dim3 grid((S2 + TILE - 1) / TILE, (L2 + TILE - 1) / TILE);
    if (int rc = check_grid(c, what, grid)) return rc;
    return run(c, mem, b, [&](Buf (&x)[4]) {
        double2 *pg2 = g2 ? (double2 *)x[3].dev : nullptr;
        double *pg3 = (double *)x[1].dev, *pq = (double *)x[2].dev;
        if constexpr (SQ) {  // xsw_grad_local takes float64 only: there is no k_grad_local<float, false>
            if (dtype == XSW_F32) {
                hipLaunchKernelGGL((k_grad_local<float, true>), grid, dim3(256), 0, c->stream, (const float *)x[0].dev, pg2, pg3, pq, L1, S1, L2, S2);
                return;
            }
        }
        hipLaunchKernelGGL((k_grad_local<double, SQ>), grid, dim3(256), 0, c->stream, (const double *)x[0].dev, pg2, pg3, pq, L1, S1, L2, S2);
    }, what);
}

extern "C" int xsw_grad_local(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *ampl, double *g2, double *g3,
                              double *quality)
{
    return grad_local<false>(c, "grad_local", lines, samples, XSW_F64, mem, ampl, g2, g3, quality);
}

// xsw_grad_hist (keep nullptr: k_grad_hist) and xsw_grad_hist_masked (k_grad_hist_masked).
static int grad_hist(xsw_ctx *c, const char *what, int64_t lines, int64_t samples, int32_t mem, const double *g2, const double *quality,
                     const uint8_t *keep, int32_t window_lines, int32_t window_samples, int32_t n_rows, const int32_t *rows, int32_t n_cols,
                     const int32_t *cols, int32_t n_angles, double angle_start, double angle_step, int32_t normalise, double *weight,
                     double *used_ratio)
{
    if (!g2 || !quality || !rows || !cols || !weight || !used_ratio || lines < 1 || samples < 1 || window_lines < 1 || window_samples < 1 || n_rows < 1 ||
        n_cols < 1 || n_angles < 1)
        return fail(c, XSW_EINVAL, "%s: bad argument", what);
    if (!fits_int(lines, samples) || !fits_int(std::min<long long>(window_lines, lines) * std::min<long long>(window_samples, samples)))
        return fail(c, XSW_EINVAL, "%s: raster or window too large", what);
    if (!fits_int((long long)n_rows * n_cols)) return fail(c, XSW_EINVAL, "%s: too many windows", what);
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const size_t npx = (size_t)lines * samples, nw = (size_t)n_rows * n_cols;
    Buf b[7] = {{g2, nullptr, npx * 16}, {quality, nullptr, npx * 8}, {rows, nullptr, (size_t)n_rows * 4}, {cols, nullptr, (size_t)n_cols * 4},
                {nullptr, weight, nw * n_angles * 8}, {nullptr, used_ratio, nw * 8}, {keep, nullptr, keep ? npx : 0}};
    return run(c, mem, b, [&](Buf (&x)[7]) {
        if (keep)
            hipLaunchKernelGGL(k_grad_hist_masked, dim3((unsigned)nw), dim3(HIST_THREADS), 0, c->stream, (const double2 *)x[0].dev, (const double *)x[1].dev,
                               (const uint8_t *)x[6].dev, (int)lines, (int)samples, (int)window_lines, (int)window_samples, (const int *)x[2].dev, (int)n_rows,
                               (const int *)x[3].dev, (int)n_cols, (int)n_angles, angle_start, angle_step, (int)(normalise != 0), (double *)x[4].dev,
                               (double *)x[5].dev);
        else
            hipLaunchKernelGGL(k_grad_hist, dim3((unsigned)nw), dim3(HIST_THREADS), 0, c->stream, (const double2 *)x[0].dev, (const double *)x[1].dev,
                               (int)lines, (int)samples, (int)window_lines, (int)window_samples, (const int *)x[2].dev, (int)n_rows, (const int *)x[3].dev,
                               (int)n_cols, (int)n_angles, angle_start, angle_step, (int)(normalise != 0), (double *)x[4].dev, (double *)x[5].dev);
    }, what);
}

extern "C" int xsw_grad_hist(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *g2, const double *quality,
                             int32_t window_lines, int32_t window_samples, int32_t n_rows, const int32_t *rows, int32_t n_cols,
                             const int32_t *cols, int32_t n_angles, double angle_start, double angle_step, int32_t normalise,
                             double *weight, double *used_ratio)
{
    if (!c) return XSW_EINVAL;
    return grad_hist(c, "grad_hist", lines, samples, mem, g2, quality, nullptr, window_lines, window_samples, n_rows, rows, n_cols, cols, n_angles,
                     angle_start, angle_step, normalise, weight, used_ratio);
}

extern "C" int xsw_grad_hist_masked(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *g2, const double *quality,
                                    const uint8_t *keep, int32_t window_lines, int32_t window_samples, int32_t n_rows, const int32_t *rows,
                                    int32_t n_cols, const int32_t *cols, int32_t n_angles, double angle_start, double angle_step,
                                    int32_t normalise, double *weight, double *used_ratio)
{
    if (!c) return XSW_EINVAL;
    if (!keep) return fail(c, XSW_EINVAL, "grad_hist_masked: keep is NULL (the unmasked histogram is xsw_grad_hist)");
    return grad_hist(c, "grad_hist_masked", lines, samples, mem, g2, quality, keep, window_lines, window_samples, n_rows, rows, n_cols, cols,
                     n_angles, angle_start, angle_step, normalise, weight, used_ratio);
}

// One launch of k_grad_keep: the widest vector the block's row bytes, the raster's row bytes and the base address allow.
template <typename T>
static int grad_keep(xsw_ctx *c, const char *what, int64_t lines, int64_t samples, int32_t mem, const T *src, KeepTest<T> test, int32_t block,
                     const uint8_t *and_with, uint8_t *out)
{
    if (!src || !out || block < 1 || lines < block || samples < block) return fail(c, XSW_EINVAL, "%s: bad argument (block < 1 or an empty output)", what);
    if (int rc = check_dims(c, what, lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const long long Lo = lines / block, So = samples / block, es = (long long)sizeof(T);
    const size_t no = (size_t)Lo * So;
    Buf b[3] = {{src, nullptr, (size_t)(lines * samples * es)}, {and_with, nullptr, and_with ? no : 0}, {nullptr, out, no}};
    const Strips g = strip_grid(Lo, So);
    const long long rpb = g.rows_per_block;
    const dim3 grid((unsigned)g.gx, (unsigned)g.gy);
    return run(c, mem, b, [&](Buf (&x)[3]) {
        const T *in = (const T *)x[0].dev;
        const uint8_t *aw = and_with ? (const uint8_t *)x[1].dev : nullptr;
        uint8_t *o = (uint8_t *)x[2].dev;
        int W = (int)es;
        for (int w = 16; w >= 4 && w > es; w >>= 1)
            if ((block * es) % w == 0 && (samples * es) % w == 0 && (uintptr_t)in % w == 0) { W = w; break; }
        const int nv = (int)(block * es / W);
#define XSW_KEEP_LAUNCH(WW, BB)                                                                                                              \
    hipLaunchKernelGGL((k_grad_keep<T, WW, BB>), grid, dim3(256), 0, c->stream, in, aw, o, (long long)samples, (int)block, nv, Lo, So, rpb, test)
        if constexpr (sizeof(T) == 8) {
            if (W == 16 && block == 2) XSW_KEEP_LAUNCH(16, 2);
            else if (W == 16) XSW_KEEP_LAUNCH(16, 0);
            else XSW_KEEP_LAUNCH(8, 0);
        } else {
            if (W == 16) XSW_KEEP_LAUNCH(16, 0);
            else if (W == 8) XSW_KEEP_LAUNCH(8, 0);
            else if (W == 4) XSW_KEEP_LAUNCH(4, 0);
            else XSW_KEEP_LAUNCH(1, 0);
        }
#undef XSW_KEEP_LAUNCH
    }, what);
}

extern "C" int xsw_grad_keep_f64(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *src, double threshold, int32_t block,
                                 const uint8_t *and_with, uint8_t *out)
{
    if (!c) return XSW_EINVAL;
    if (std::isnan(threshold)) return fail(c, XSW_EINVAL, "grad_keep_f64: the threshold is NaN");
    KeepTest<double> test;
    test.thr = threshold;
    return grad_keep<double>(c, "grad_keep_f64", lines, samples, mem, src, test, block, and_with, out);
}

extern "C" int xsw_grad_keep_u8(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const uint8_t *src, int32_t block, const uint8_t *and_with,
                                uint8_t *out)
{
    if (!c) return XSW_EINVAL;
    return grad_keep<uint8_t>(c, "grad_keep_u8", lines, samples, mem, src, KeepTest<uint8_t>(), block, and_with, out);
}

extern "C" int xsw_grad_r2_sqrt(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *sigma0, double *out)
{
    return grad_r2<true>(c, "grad_r2_sqrt", lines, samples, dtype, mem, 0, sigma0, out);
}

extern "C" int xsw_grad_local_sqrt(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *sigma0, double *g2,
                                   double *g3, double *quality)
{
    return grad_local<true>(c, "grad_local_sqrt", lines, samples, dtype, mem, sigma0, g2, g3, quality);
}

extern "C" int xsw_grad_smooth(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, int32_t coarsen, const double *in, double *out)
{
    if (!c) return XSW_EINVAL;
    const int64_t f = coarsen ? 2 : 1;
    if (!in || !out || lines < f || samples < f) return fail(c, XSW_EINVAL, "grad_smooth: bad argument");
    if (int rc = check_dims(c, "grad_smooth", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const int S = (int)samples, Lo = (int)(lines / f), So = (int)(samples / f);
    Buf b[2] = {{in, nullptr, (size_t)(lines * samples * 8)}, {nullptr, out, (size_t)Lo * So * 8}};
    const dim3 grid((So + 63) / 64, (Lo + 3) / 4);
    if (int rc = check_grid(c, "grad_smooth", grid)) return rc;
    return run(c, mem, b, [&](Buf (&x)[2]) {
        if (coarsen)
            hipLaunchKernelGGL(k_grad_smooth<true>, grid, dim3(256), 0, c->stream, (const double *)x[0].dev, (double *)x[1].dev, S, Lo, So);
        else
            hipLaunchKernelGGL(k_grad_smooth<false>, grid, dim3(256), 0, c->stream, (const double *)x[0].dev, (double *)x[1].dev, S, Lo, So);
    }, "grad_smooth");
}

extern "C" int xsw_grad_mean(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *in, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!in || !out || lines < 1 || samples < 1) return fail(c, XSW_EINVAL, "grad_mean: bad argument");
    if (int rc = check_dims(c, "grad_mean", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const int L = (int)lines, S = (int)samples;
    Buf b[2] = {{in, nullptr, (size_t)L * S * 8}, {nullptr, out, (size_t)L * S * 8}};
    const dim3 grid((S + MT - 1) / MT, (L + MT - 1) / MT);
    if (int rc = check_grid(c, "grad_mean", grid)) return rc;
    return run(c, mem, b, [&](Buf (&x)[2]) {
        hipLaunchKernelGGL(k_grad_mean, grid, dim3(256), 0, c->stream, (const double *)x[0].dev, (double *)x[1].dev, L, S);
    }, "grad_mean");
}

extern "C" int xsw_grad_filter(xsw_ctx *c, int64_t lines, int64_t samples, int32_t mem, const double *r2, const double *g3, const double *quality,
                               const double *smooth4, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!r2 || !g3 || !quality || !smooth4 || !out || lines < 2 || samples < 2)
        return fail(c, XSW_EINVAL, "grad_filter: bad argument (the half-resolution raster needs 2 x 2 pixels)");
    if (int rc = check_dims(c, "grad_filter", lines, samples)) return rc;
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    const int L = (int)lines, S = (int)samples, L4 = L / 2, S4 = S / 2;
    const size_t n = (size_t)L * S;
    Buf b[5] = {{r2, nullptr, n * 8}, {g3, nullptr, n * 8}, {quality, nullptr, n * 8}, {smooth4, nullptr, (size_t)L4 * S4 * 8}, {nullptr, out, 5 * n * 8}};
    const dim3 grid((S + MT - 1) / MT, (L + MT - 1) / MT);
    if (int rc = check_grid(c, "grad_filter", grid)) return rc;
    // scipy's zoom factor of each axis, the same IEEE division
    const double zy = (double)(L4 - 1) / (double)(L - 1), zx = (double)(S4 - 1) / (double)(S - 1);
    return run(c, mem, b, [&](Buf (&x)[5]) {
        hipLaunchKernelGGL(k_grad_filter, grid, dim3(256), 0, c->stream, (const double *)x[0].dev, (const double *)x[1].dev, (const double *)x[2].dev,
                           (const double *)x[3].dev, (double *)x[4].dev, L, S, L4, S4, zy, zx);
    }, "grad_filter");
}
