// The LUT side's pure arithmetic: what a LUT install derives on the host from the axes and the table before anything is
// allocated or launched -- axis predicates, table shapes and gates, the scalars and capability flags of DevTables, the
// host-built tables -- and the like of xsw_detrend and xsw_nesz_flatten.  No HIP type or call in here, so a host compiler
// builds it alone (tests/test_host_lutplan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "xsw.h"

// ---- table shapes (kernels and install agree on them through these)
#ifndef XSW_INV_BINS
#define XSW_INV_BINS 2048  // thresholds per slice of the inverse-row table (DevTables::inv_rows)
#endif
#ifndef XSW_TAIL_LEVELS
#define XSW_TAIL_LEVELS 7  // levels of the sparse table of tail minima (DevTables::tail_min): windows of up to 2^7 - 1 directions
#endif
// block pyramid (co_block_search, xsw_device.hpp): blocks of XSW_BLK_R speed rows x XSW_BLK_C directions, one candidate per lane
#ifndef XSW_BLK_R
#define XSW_BLK_R 4
#endif
#ifndef XSW_BLK_C
#define XSW_BLK_C 16
#endif
#ifndef XSW_CELL_R
#define XSW_CELL_R 8  // block rows ...
#endif
#ifndef XSW_CELL_C
#define XSW_CELL_C 2  // ... x block columns of a level-1 cell of k_invert_blocks (32 speed rows x 32 directions: 16 blocks, one bounding step)
#endif
#define XSW_BLK_C4 4  // directions of a sub-block (k_invert_blocks: a kept block is bounded once more per quarter before it is swept)

// ---- axis predicates
static inline bool strictly_ascending(const double *a, int n) { return std::adjacent_find(a, a + n, [](double x, double y) { return !(y > x); }) == a + n; }
// "uniform" to the error budget the pruned kernels' screening assumes: they score with w_i = w0 + i*step (forward
// differences) and re-score only candidates within 1e-9 (1 + |J_min| + m2) of the screening minimum with the real axis
// values, so an axis point may be off its grid position by no more than ~1e-12 relative (dJ/dw is O(10..100)): np.linspace
// axes are within a few ulps and pass; an axis stored in float32, or perturbed by 1e-7 of a step, takes the exact kernel.
static inline bool uniform_axis(const double *a, int n)
{
    if (n < 2) return false;
    const double step = (a[n - 1] - a[0]) / (n - 1);
    if (!(step > 0) || !std::isfinite(step)) return false;
    const double tol = 1e-12 * std::max(std::max(std::fabs(a[0]), std::fabs(a[n - 1])), step);
    for (int i = 0; i < n; ++i)
        if (!(std::fabs(a[i] - (a[0] + i * step)) <= tol)) return false;
    return true;
}
static inline bool all_finite(const double *a, size_t n) { return std::all_of(a, a + n, [](double v) { return std::isfinite(v); }); }
static inline bool same_axis(const double *a, int na, const double *b, int nb) { return na == nb && std::equal(a, a + na, b); }
static inline bool left_neighbours(const double *x_old, int n_old, const double *x_new, int n_new, std::vector<int> &lo)
{
    // scipy interp1d: searchsorted(x_old, x_new) (side='left'), clip(1, n-1), minus one; bounds_error=True
    lo.resize(n_new);
    for (int i = 0; i < n_new; ++i) {
        const double x = x_new[i];
        if (!(x >= x_old[0] && x <= x_old[n_old - 1])) return false;
        const int a = (int)(std::lower_bound(x_old, x_old + n_old, x) - x_old);
        int hi = a < 1 ? 1 : (a > n_old - 1 ? n_old - 1 : a);
        lo[i] = hi - 1;
    }
    return true;
}

// A table the context owns carries this many bytes past its last element (the kernels' unmasked vector loads may reach there).
#define XSW_OWNED_SLACK 64
static inline unsigned blocks_of_256(long long n) { return (unsigned)((n + 255) / 256); }

// ---- co-pol geometry, from the shape alone (CoGeometry g{n_inc, n_w, n_phi}): pads, the element counts install_co allocates,
// zeroes and launches over, the gates of the optional tables, the launch grids
struct CoGeometry {
    int n_inc, n_w, n_phi;
    int ppad = (n_phi + 3) & ~3, wpad = (n_w + 3) & ~3;
    // block pyramid: block rows / columns, sub-block columns, cell rows / columns, block rows per band, bands
    int nbr = (n_w + XSW_BLK_R - 1) / XSW_BLK_R, nbc = (n_phi + XSW_BLK_C - 1) / XSW_BLK_C, nbc4 = (n_phi + XSW_BLK_C4 - 1) / XSW_BLK_C4;
    int ncr = (nbr + XSW_CELL_R - 1) / XSW_CELL_R, ncc = (nbc + XSW_CELL_C - 1) / XSW_CELL_C;
    int blk_g = std::max(1, 64 / nbc), nbands = (nbr + blk_g - 1) / blk_g;
    long long rows = (long long)n_inc * n_w;
    size_t n_dense = (size_t)rows * n_phi;
    // padded table = body + slack rows (the kernels read 4 row groups ahead unmasked)
    size_t n_body = (size_t)rows * ppad, n_slack = (size_t)260 * ppad, n_pad = n_body + n_slack;
    size_t tail_n = (size_t)n_inc * (XSW_TAIL_LEVELS + 1) * ppad;  // tail minima
    size_t inv_n = (size_t)n_inc * XSW_INV_BINS * ppad, inv_grid_n = (size_t)3 * n_inc;  // inverse rows, their grid
    size_t coT_n = (size_t)n_inc * n_phi * wpad + 512;  // transposed slices + 512 doubles of slack, zeroed with them
    long long nblk = (long long)n_inc * nbr * nbc, nband = (long long)n_inc * nbands;
    long long ncell = (long long)n_inc * ncr * ncc, nblk4 = (long long)n_inc * nbr * nbc4;
    // inverse rows: unsigned short rows and slices, byte offsets < 2^32; blocks (with them bands and cells), sub-blocks: counts < 2^31
    bool inv_ok = n_w < 65536 && n_inc < 65536 && inv_n * sizeof(unsigned short) < ((size_t)1 << 32);
    bool blk_ok = nblk < (1LL << 31), blk4_ok = nblk4 < (1LL << 31);
    unsigned pad_grid = (unsigned)std::min<long long>((rows + 3) / 4, 256 * 32);  // k_pad_co: 4 rows per workgroup trip
    unsigned col_grid = blocks_of_256((long long)n_inc * n_phi);                 // k_mono_rows / k_inv_rows: one thread per column
};

// ---- co-pol host tables: the caller's values where given, the host libm's otherwise (xsw.h)
struct CoHostTables {
    std::vector<double> wh, cphi, sphi, csphi;  // w / 2; cos / sin(radians(phi)); the two interleaved
    std::vector<float> wh32, csphi32, sol32;
    std::vector<double> out_dir, abs_co, dual_dir, sol;  // DevTables' members of these names
    bool trig_ok = true;  // cphi / sphi are within 1e-12 of this libm's cos / sin (a condition of DevTables::prunable)

    explicit CoHostTables(const xsw_lut *l)
    {
        const int nW = l->n_wspd, nP = l->n_phi;
        wh.resize(nW); cphi.resize(nP); sphi.resize(nP);
        for (int i = 0; i < nW; ++i) wh[i] = 0.5 * l->wspd[i];
        for (int i = 0; i < nP; ++i) {
            const double r = l->phi[i] * (M_PI / 180.0);
            cphi[i] = l->cos_phi ? l->cos_phi[i] : std::cos(r);
            sphi[i] = l->sin_phi ? l->sin_phi[i] : std::sin(r);
            if (std::fabs(cphi[i] - std::cos(r)) > 1e-12 || std::fabs(sphi[i] - std::sin(r)) > 1e-12) trig_ok = false;
        }
        wh32.assign(wh.begin(), wh.end());
        csphi.resize((size_t)2 * nP);
        for (int i = 0; i < nP; ++i) { csphi[2 * i] = cphi[i]; csphi[2 * i + 1] = sphi[i]; }
        csphi32.assign(csphi.begin(), csphi.end());  // float32 copy: the bound arithmetic of k_invert_band2 (xsw_band2.hpp)
        out_dir.resize((size_t)4 * nP); abs_co.resize((size_t)nW * nP); dual_dir.resize((size_t)4 * nW * nP); sol.resize(dual_dir.size());
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < nP; ++i) {
                const double r = (k ? -l->phi[i] : l->phi[i]) * (M_PI / 180.0);
                out_dir[((size_t)k * nP + i) * 2 + 0] = l->out_dir ? l->out_dir[((size_t)k * nP + i) * 2 + 0] : std::cos(r);
                out_dir[((size_t)k * nP + i) * 2 + 1] = l->out_dir ? l->out_dir[((size_t)k * nP + i) * 2 + 1] : std::sin(r);
            }
        for (int iw = 0; iw < nW; ++iw)
            for (int i = 0; i < nP; ++i) {
                const double w = l->wspd[iw];
                for (int k = 0; k < 2; ++k) {
                    const double er = out_dir[((size_t)k * nP + i) * 2], ei = out_dir[((size_t)k * nP + i) * 2 + 1];
                    const double re = w * er, im = w * ei + 0.0 * er;
                    const size_t o = (((size_t)k * nW + iw) * nP + i) * 2;
                    // the co-pol winds themselves, by the store's own operations (store_pixel: w * e.x, w * e.y + 0.0 * e.x): what
                    // a grid code expands to, on the device (k_expand) and on the host (expand_host)
                    sol[o] = re; sol[o + 1] = im;
                    if (l->dual_dir) { dual_dir[o] = l->dual_dir[o]; dual_dir[o + 1] = l->dual_dir[o + 1]; }
                    else { const double ph = std::atan2(im, re); dual_dir[o] = std::cos(ph); dual_dir[o + 1] = std::sin(ph); }
                    if (k == 0) abs_co[(size_t)iw * nP + i] = l->abs_co ? l->abs_co[(size_t)iw * nP + i] : std::hypot(re, im);
                }
            }
        sol32.assign(sol.begin(), sol.end());
    }
};

// ---- co-pol scalars and capability flags: every non-pointer member of DevTables an install sets but co_absmax (read back from
// the device).  Tab: DevTables, or a plain struct with the same member names (the host test's).
template <class Tab>
static inline void co_scalars(Tab &T, const xsw_lut *l, const CoGeometry &g, bool lut_finite, bool trig_ok)
{
    const int nI = g.n_inc, nW = g.n_w, nP = g.n_phi, ppad = g.ppad, wpad = g.wpad;
    T.nbr = g.nbr; T.nbc = g.nbc; T.nbc4 = g.nbc4; T.ncr = g.ncr; T.ncc = g.ncc; T.blk_g = g.blk_g; T.nbands = g.nbands;
    T.n_inc = nI; T.n_w = nW; T.n_phi = nP; T.phi_pad = ppad; T.w_pad = wpad;
    T.phi_180 = (180.0 - (l->phi[nP - 1] - l->phi[0])) < 2.0 ? 1 : 0;  // windspeed.py:152-156
    T.w0 = l->wspd[0];
    T.phi0 = l->phi[0];
    T.phi_last = l->phi[nP - 1];
    T.inv_wstep = nW > 1 ? (nW - 1) / (l->wspd[nW - 1] - l->wspd[0]) : 0.0;
    T.inv_dphi = nP > 1 ? (nP - 1) / (l->phi[nP - 1] - l->phi[0]) : 0.0;
    T.wstep_half = 0.5 / T.inv_wstep;  // the kernels' (w/2)-per-row step: same IEEE quotient they used to form per wave
    T.inv_nphi = 1.0 / (double)nP;
    T.inc_uniform = uniform_axis(l->inc, nI) && nI >= 2 ? 1 : 0;
    T.inc0 = l->inc[0];
    T.inv_incstep = nI > 1 ? (nI - 1) / (l->inc[nI - 1] - l->inc[0]) : 0.0;
    T.prunable = (nW >= 2 && nP >= 2 && nW < 32768 && nP < 65536 && (int64_t)nW * ppad < ((int64_t)1 << 30) && uniform_axis(l->wspd, nW) && uniform_axis(l->phi, nP) && trig_ok &&
                  (l->phi[nP - 1] - l->phi[0]) <= 360.0 + 1e-9 && lut_finite)
                     ? 1 : 0;
    T.co_off32 = ((uint64_t)nI * nW + 260) * (uint64_t)ppad * 8u < ((uint64_t)1 << 32) ? 1 : 0;
    T.band_mul24 = ((uint64_t)nI * nW <= 0xFFFFFFu && (uint64_t)(nI + 1) * XSW_INV_BINS <= 0xFFFFFFu && (uint64_t)ppad * 8u <= 0xFFFFFFu &&
                    (uint64_t)(nI + 1) * nP <= 0xFFFFFFu && (uint64_t)wpad * 8u <= 0xFFFFFFu && (uint64_t)nI * nP * wpad * 8u < ((uint64_t)1 << 32)) ? 1 : 0;
    T.blk_span_ok = (nP > 1 && (XSW_BLK_C - 1) * (l->phi[nP - 1] - l->phi[0]) / (nP - 1) < 170.0) ? 1 : 0;
    T.cell_span_ok = (nP > 1 && (XSW_CELL_C * XSW_BLK_C - 1) * (l->phi[nP - 1] - l->phi[0]) / (nP - 1) < 170.0) ? 1 : 0;
}

// ---- cross-pol: everything upload_cr derives on the host
struct CrPlan {
    int wpad;
    std::vector<double> pad, wh;  // [n_inc][wpad] rows zero-padded; w / 2
    bool finite, monotone;        // no NaN / inf in the table; that, a uniform speed axis and every row non-decreasing
    // inverse of the monotone rows (search_cr_scan): inv[r][b] = first k with row[k] >= t0 + b * width; grid[r] = t0, width,
    // 1 / width (zeros for a row of no width).  Empty: not monotone, or rows too long for unsigned short.
    std::vector<unsigned short> inv;
    std::vector<double> grid;

    explicit CrPlan(const xsw_lut *l) : wpad((l->n_wspd + 3) & ~3)
    {
        const int nI = l->n_inc, nW = l->n_wspd;
        pad.assign((size_t)nI * wpad, 0.0); wh.resize(nW);
        for (int r = 0; r < nI; ++r) memcpy(&pad[(size_t)r * wpad], l->db + (size_t)r * nW, nW * sizeof(double));
        for (int i = 0; i < nW; ++i) wh[i] = 0.5 * l->wspd[i];
        finite = all_finite(l->db, (size_t)nI * nW);
        monotone = finite && nW >= 2 && uniform_axis(l->wspd, nW);
        for (int r = 0; r < nI && monotone; ++r)
            for (int k = 1; k < nW; ++k)
                if (l->db[(size_t)r * nW + k] < l->db[(size_t)r * nW + k - 1]) { monotone = false; break; }
        if (!(monotone && nW < 65536)) return;
        inv.resize((size_t)nI * XSW_INV_BINS); grid.resize((size_t)3 * nI);
        for (int r = 0; r < nI; ++r) {
            const double *row = l->db + (size_t)r * nW;
            const double t0 = row[0], width = (row[nW - 1] - row[0]) / (double)XSW_INV_BINS;
            const bool ok = width > 0.0 && width < 1e300;
            grid[3 * r] = ok ? t0 : 0.0; grid[3 * r + 1] = ok ? width : 0.0; grid[3 * r + 2] = ok ? 1.0 / width : 0.0;
            for (int b = 0; b < XSW_INV_BINS; ++b)
                inv[(size_t)r * XSW_INV_BINS + b] = (unsigned short)(b == 0 || !ok ? 0 : std::lower_bound(row, row + nW, std::fma((double)b, width, t0)) - row);
        }
    }
};

template <class Tab>
static inline void cr_scalars(Tab &T, const xsw_lut *l, const CrPlan &p)
{
    const int nI = l->n_inc, nW = l->n_wspd;
    T.n_inc_cr = nI; T.n_wcr = nW; T.wcr_pad = p.wpad;
    T.cr_finite = p.finite ? 1 : 0;
    T.cr_monotone = p.monotone ? 1 : 0;
    T.wcr0 = l->wspd[0];
    T.inv_wcrstep = nW > 1 ? (nW - 1) / (l->wspd[nW - 1] - l->wspd[0]) : 0.0;
    T.wcrstep_half = 0.5 / T.inv_wcrstep;
    T.inc_cr_uniform = uniform_axis(l->inc, nI) && nI >= 2 ? 1 : 0;
    T.inc_cr0 = l->inc[0];
    T.inv_inccrstep = nI > 1 ? (nI - 1) / (l->inc[nI - 1] - l->inc[0]) : 0.0;
}

// ---- xsw_detrend: both = [ratio | RN(1/ratio)]; returns whether the fused-multiply quotient of k_detrend is exact for every
// divisor of the row (it is only for "ordinary" ones: not tiny, huge, zero, inf, NaN, nor with a mantissa of all ones)
static inline bool detrend_row(const double *ratio_row, size_t samples, std::vector<double> &both)
{
    both.resize(2 * samples);
    bool fast = true;
    for (size_t k = 0; k < samples; ++k) {
        const double r = ratio_row[k];
        both[k] = r;
        both[samples + k] = 1.0 / r;
        uint64_t bits;
        memcpy(&bits, &r, 8);
        const double ar = std::fabs(r);
        if (!(ar > 0x1p-500 && ar < 0x1p500) || (bits & 0xFFFFFFFFFFFFFull) == 0xFFFFFFFFFFFFFull) fast = false;
    }
    return fast;
}

// ---- xsw_nesz_flatten: line blocks of the column pass -- enough workgroups to fill the chip (~16 per CU), at least 8 lines
// each -- and the bytes of its scratch (column partials of partial_bytes each, means, centring abscissa, per-line fit)
struct NeszBlocks {
    long long nb, lpb;
    size_t scratch_bytes;
};
static inline NeszBlocks nesz_blocks(long long lines, long long samples, size_t partial_bytes)
{
    NeszBlocks b;
    const long long gx = (samples + 255) / 256;
    b.nb = (256LL * 16 + gx - 1) / gx;
    b.nb = std::max<long long>(1, std::min<long long>(std::min<long long>(b.nb, (lines + 7) / 8), 65535));
    b.lpb = (lines + b.nb - 1) / b.nb;
    b.nb = (lines + b.lpb - 1) / b.lpb;
    b.scratch_bytes = (size_t)b.nb * samples * partial_bytes + (2 * (size_t)samples + 8 + 2 * (size_t)lines) * sizeof(double);
    return b;
}
