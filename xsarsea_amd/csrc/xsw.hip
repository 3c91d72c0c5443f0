// libxsw host side: context, LUT upload, launch logic behind the C ABI of include/xsw.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "xsw.h"
#include "xsw_device.hpp"
#include "xsw_misc.hpp"
#include "xsw_gmf.hpp"
#include "xsw_nesz.hpp"
#include "xsw_dsig.hpp"
#include "xsw_lutbuild.hpp"

using namespace xsw;

#include "xsw_run.hpp"

#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), e_ == hipErrorOutOfMemory ? XSW_ENOMEM : XSW_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                       \
    } while (0)

extern "C" int xsw_version(void) { return XSW_VERSION; }

extern "C" int xsw_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *xsw_last_error(const xsw_ctx *ctx) { return ctx ? ctx->err.c_str() : create_err().c_str(); }

extern "C" int xsw_ctx_create(int device, xsw_ctx **out)
{
    if (!out) return fail(nullptr, XSW_EINVAL, "ctx out pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, XSW_EHIP, "no HIP device available (%s)", e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, XSW_EINVAL, "device %d out of range [0,%d)", device, n);
    xsw_ctx *c = new xsw_ctx;
    c->device = device;
    const int rc = [&]() -> int {
        HIPCHK(nullptr, hipSetDevice(device));
        HIPCHK(nullptr, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        c->stream = c->own_stream;
        HIPCHK(nullptr, hipMalloc((void **)&c->d_stats, 8 * sizeof(unsigned long long)));
        HIPCHK(nullptr, hipMemset(c->d_stats, 0, 8 * sizeof(unsigned long long)));
        return XSW_OK;
    }();
    if (rc != XSW_OK) {  // nothing half-built is handed out or leaked
        if (c->d_stats) (void)hipFree(c->d_stats);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        delete c;
        return rc;
    }
    *out = c;
    return XSW_OK;
}

static void worker_release(xsw_ctx::Worker &w)
{
    if (w.s) (void)hipStreamSynchronize(w.s);
    (void)grow(w.pin, w.pin_cap, 0, nullptr, true);
    (void)grow(w.dev, w.dev_cap, 0);
}

extern "C" int xsw_ctx_destroy(xsw_ctx *c)
{
    if (!c) return XSW_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_all(c->co_allocs);
    free_all(c->cr_allocs);
    if (c->d_stats) (void)hipFree(c->d_stats);
    (void)grow(c->d_ratio, c->ratio_cap, 0);
    (void)grow(c->lists.base, c->lists_bytes, 0);
    (void)grow(c->nesz_scratch, c->nesz_cap, 0);
    for (hipEvent_t e : c->timing_events) (void)hipEventDestroy(e);
    (void)grow(c->arena, c->arena_cap, 0);
    for (auto &w : c->workers) {
        worker_release(w);
        if (w.s) (void)hipStreamDestroy(w.s);
    }
    for (void *p : c->host_allocs) (void)hipHostFree(p);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return XSW_OK;
}

extern "C" int xsw_set_stream(xsw_ctx *c, void *s)
{
    if (!c) return XSW_EINVAL;
    if ((hipStream_t)s != c->stream) {
        // context-owned buffers (work list, nesz scratch, ratio row) are reused by the next call: what was queued on the old
        // stream must be through with them before anything queued on the new one touches them -- ordered on the device (an
        // event the new stream waits for), the host does not block
        HIPCHK(c, hipSetDevice(c->device));
        hipEvent_t ev = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)s, ev, 0);
        (void)hipEventDestroy(ev);  // released once the wait has been satisfied
        if (e != hipSuccess) return fail(c, XSW_EHIP, "stream hand-over failed: %s", hipGetErrorString(e));
    }
    c->stream = (hipStream_t)s;  // NULL is a valid handle: the device's default stream
    return XSW_OK;
}

extern "C" int xsw_use_own_stream(xsw_ctx *c)
{
    if (!c) return XSW_EINVAL;
    return xsw_set_stream(c, (void *)c->own_stream);
}

static int host_thread_count(const xsw_ctx *c);

// Staging kept between calls: each worker of the host-memory paths owns a page-locked buffer and a device buffer of one chunk
// (float32 mono: ~40 MB each; float64 dual-pol: ~110 MB each), i.e. up to threads x chunk of pinned host memory per context.
// After every host-memory call the buffers beyond XSW_STAGING_KEEP_MB (default 1536 MB per context -- the default 12 workers at float32 mono chunks hold ~1.1 GB --, counted per worker as the
// larger of its page-locked and its device buffer) are released, largest first -- a later call allocates them again (a few ms each).
static void trim_staging(xsw_ctx *c)
{
    static const size_t keep = (size_t)env_int("XSW_STAGING_KEEP_MB", 1536, 0) << 20;
    // a worker counts with the larger of its two buffers: the pinned-input paths (XSW_MEM_HOST_PINNED, the pinned detrend) hold
    // no page-locked staging at all, and the device side of a worker (inputs + codes + its work lists and records) outgrows
    // the pinned side
    auto held = [](const xsw_ctx::Worker &w) { return std::max(w.pin_cap, w.dev_cap); };
    size_t total = 0;
    for (auto &w : c->workers) total += held(w);
    while (total > keep) {
        xsw_ctx::Worker *big = nullptr;
        for (auto &w : c->workers)
            if (held(w) && (!big || held(w) > held(*big))) big = &w;
        if (!big) break;
        total -= held(*big);
        worker_release(*big);
    }
}

extern "C" int xsw_set_host_threads(xsw_ctx *c, int n)
{
    if (!c || n < 0) return XSW_EINVAL;
    c->host_threads = n > 32 ? 32 : n;
    // workers the new count no longer uses give their staging back now
    const size_t keep_workers = (size_t)host_thread_count(c);
    if (c->workers.size() > keep_workers) {
        (void)hipSetDevice(c->device);
        for (size_t k = keep_workers; k < c->workers.size(); ++k) {
            worker_release(c->workers[k]);
            if (c->workers[k].s) (void)hipStreamDestroy(c->workers[k].s);
        }
        c->workers.resize(keep_workers);
    }
    return XSW_OK;
}

extern "C" int xsw_host_alloc(xsw_ctx *c, size_t bytes, void **out)
{
    if (!c || !out) return XSW_EINVAL;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return fail(c, XSW_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
    c->host_allocs.push_back(p);
    *out = p;
    return XSW_OK;
}

extern "C" int xsw_host_free(xsw_ctx *c, void *p)
{
    if (!c) return XSW_EINVAL;
    auto it = std::find(c->host_allocs.begin(), c->host_allocs.end(), p);
    if (it == c->host_allocs.end()) return fail(c, XSW_EINVAL, "xsw_host_free: not a pointer of xsw_host_alloc on this context");
    c->host_allocs.erase(it);
    HIPCHK(c, hipHostFree(p));
    return XSW_OK;
}

extern "C" int xsw_synchronize(xsw_ctx *c)
{
    if (!c) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return XSW_OK;
}

extern "C" int xsw_stats_enable(xsw_ctx *c, int on)
{
    if (!c) return XSW_EINVAL;
    c->stats_on = on != 0;
    c->stats_chain = on == 2;  // counters of the PRODUCTION chain (xsw_stats_read_chain), not of the statistics instantiation
    return XSW_OK;
}

extern "C" int xsw_timing_enable(xsw_ctx *c, int on)
{
    if (!c) return XSW_EINVAL;
    for (hipEvent_t e : c->timing_events) (void)hipEventDestroy(e);
    c->timing_events.clear();
    c->timing_on = on != 0;
    return XSW_OK;
}

extern "C" int xsw_timing_read(xsw_ctx *c, xsw_timing *out)
{
    if (!c || !out) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->launches = 0;
    out->first_kernel_ms = out->second_kernel_ms = out->band2_kernel_ms = out->blocks_kernel_ms = 0.0;
    out->last_band2_pixels = 0;
    out->last_list_pixels = 0;
    out->last_blocks_pixels = 0;
    if (c->lists.base) {
        unsigned cnt[3] = {0, 0, 0};
        HIPCHK(c, hipMemcpy(cnt, c->lists.count(WorkLists::G), sizeof cnt, hipMemcpyDeviceToHost));
        out->last_list_pixels = (int64_t)cnt[0];
        out->last_band2_pixels = (int64_t)cnt[1];
        out->last_blocks_pixels = (int64_t)cnt[2];
    }
    for (size_t k = 0; k + 5 <= c->timing_events.size(); k += 5) {  // start, after k_invert_band, k_invert_band2, k_invert_blocks, k_invert_list
        float a = 0.f, b = 0.f, bl = 0.f, d = 0.f;
        HIPCHK(c, hipEventElapsedTime(&a, c->timing_events[k], c->timing_events[k + 1]));
        HIPCHK(c, hipEventElapsedTime(&b, c->timing_events[k + 1], c->timing_events[k + 2]));
        HIPCHK(c, hipEventElapsedTime(&bl, c->timing_events[k + 2], c->timing_events[k + 3]));
        HIPCHK(c, hipEventElapsedTime(&d, c->timing_events[k + 3], c->timing_events[k + 4]));
        out->first_kernel_ms += a;
        out->band2_kernel_ms += b;
        out->blocks_kernel_ms += bl;
        out->second_kernel_ms += d;
        out->launches += 1;
    }
    for (hipEvent_t e : c->timing_events) (void)hipEventDestroy(e);
    c->timing_events.clear();
    return XSW_OK;
}

extern "C" int xsw_stats_read(xsw_ctx *c, xsw_stats *out)
{
    if (!c || !out) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long h[4];
    HIPCHK(c, hipMemcpy(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost));
    out->pixels_co = h[0];
    out->cand_co = h[1];
    out->pixels_exact = h[2];
    out->pixels_cr = h[3];
    return XSW_OK;
}

extern "C" int xsw_stats_read_chain(xsw_ctx *c, xsw_chain_stats *out)
{
    if (!c || !out) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long h[8];
    HIPCHK(c, hipMemcpy(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost));
    out->cand_band2 = h[4];
    out->cand_blocks = h[5];
    out->cand_list = h[6];
    out->pixels_refined = h[7];
    return XSW_OK;
}

// ---------------------------------------------------------------------------------------- LUT upload
// Installs a co-pol LUT.  The dense dB table [n_inc][n_wspd][n_phi] comes from the host (l->db) or is already on the
// device (d_dense, built by xsw_lut_build); the padded float64 copy, the float32 copy, the finiteness flag and max |dB|
// are produced on the device either way (k_pad_co).
static int install_co(xsw_ctx *c, const xsw_lut *l, const double *d_dense)
{
    if ((!l->db && !d_dense) || !l->inc || !l->wspd || !l->phi || l->n_inc < 1 || l->n_wspd < 1 || l->n_phi < 1)
        return fail(c, XSW_EINVAL, "co-pol LUT: null pointer or empty axis");
    if (!strictly_ascending(l->inc, l->n_inc) || !strictly_ascending(l->wspd, l->n_wspd) ||
        !strictly_ascending(l->phi, l->n_phi))
        return fail(c, XSW_EINVAL, "co-pol LUT: axes must be strictly ascending");
    if ((int64_t)l->n_wspd * l->n_phi >= (int64_t)1 << 30) return fail(c, XSW_EINVAL, "co-pol LUT too large");
    // a search queued on the context's stream (an asynchronous device-raster call, possibly on the caller's stream, or on the
    // previous stream that this one waits for since xsw_set_stream) may still read the old tables: it must be through with
    // them before they are freed -- stated here rather than left to whatever hipFree happens to wait for
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_all(c->co_allocs);
    c->have_co = false;
    DevTables &T = c->T;
    const int nI = l->n_inc, nW = l->n_wspd, nP = l->n_phi;
    const CoGeometry g{nI, nW, nP};
    const hipStream_t st = c->stream;

    // the dense table on the device: the caller's (xsw_lut_build), or a temporary of this call
    CallTemps tmp(st);
    if (!d_dense) {
        d_dense = (const double *)tmp.alloc(g.n_dense * sizeof(double), l->db);
        if (tmp.refused) return fail(c, tmp.code(), "LUT install failed: %s", hipGetErrorString(tmp.err));
        if (!tmp.ok()) return fail(c, XSW_EHIP, "LUT upload failed: %s", hipGetErrorString(tmp.err));
    }

    // required tables: the padded float64 and float32 copies (with the finiteness flag and max |dB|), the monotone rows
    DevSeq req{st, c->co_allocs};
    double *d_co = req.table<double>(g.n_pad);
    float *d_co32 = req.table<float>(g.n_pad);
    unsigned long long h_flags[2] = {0, 0}, *d_flags = req.ok() ? (unsigned long long *)tmp.alloc(sizeof h_flags) : nullptr;
    req.check(tmp.err);
    if (req.ok()) {
        req.zero(d_flags, sizeof h_flags);
        req.zero(d_co + g.n_body, g.n_slack * sizeof(double));
        req.zero(d_co32 + g.n_body, g.n_slack * sizeof(float));
    }
    req.run([&] { hipLaunchKernelGGL(k_pad_co, dim3(g.pad_grid), dim3(256), 0, st, d_dense, d_co, d_co32, nP, g.ppad, g.rows, d_flags); });
    std::vector<int> init((size_t)nI, nW);  // read by the copy below until the stream is synchronised (tmp.finish)
    int *d_mono = req.table<int>((size_t)nI);
    // on the launch stream, in order with k_mono_rows (not a null-stream copy whose completion the kernel would rely on)
    if (req.ok()) req.check(hipMemcpyAsync(d_mono, init.data(), (size_t)nI * sizeof(int), hipMemcpyHostToDevice, st));
    req.run([&] { hipLaunchKernelGGL(k_mono_rows, dim3(g.col_grid), dim3(256), 0, st, d_dense, nI, nW, nP, d_mono); });
    T.mono_rows = d_mono;

    // optional tables (DevSeq::usable): absent, the kernels take their older routes
    T.tail_min = nullptr;
    static const bool tail_off = env_flag("XSW_NO_TAIL_CUT");  // A/B measurements only
    if (req.ok() && !tail_off) {
        DevSeq opt{st, c->co_allocs};
        double *d_tail = opt.table<double>(g.tail_n);
        opt.run([&] { hipLaunchKernelGGL(k_tail_min, dim3((unsigned)nI), dim3(256), 0, st, d_dense, nW, nP, g.ppad, d_mono, d_tail); });
        if (opt.usable()) T.tail_min = d_tail;
    }
    // inverse of the monotone rows (co_band_pass starts its sweep from a table look-up instead of a bisection): optional by
    // its gate only, an error while it is built fails the install
    T.inv_rows = nullptr; T.inv_grid = nullptr;
    if (req.ok() && g.inv_ok) {
        unsigned short *d_inv = req.table<unsigned short>(g.inv_n);
        double *d_grid = req.table<double>(g.inv_grid_n);
        req.zero(d_inv, g.inv_n * sizeof(unsigned short));
        req.run([&] {
            hipLaunchKernelGGL(k_inv_range, dim3((unsigned)nI), dim3(256), 0, st, d_dense, nW, nP, d_mono, d_grid);
            hipLaunchKernelGGL(k_inv_rows, dim3(g.col_grid), dim3(256), 0, st, d_dense, nI, nW, nP, g.ppad, d_mono, d_grid, d_inv);
        });
        if (req.ok()) { T.inv_rows = d_inv; T.inv_grid = d_grid; }
    }
    // block pyramid of the general kernel (co_block_search): min / max per block of XSW_BLK_R x XSW_BLK_C candidates and per
    // band of blk_g block rows (6 MB at the default size).  Absent (allocation failure, XSW_NO_BLOCKS=1: A/B measurements and
    // the tests of the old routes): the general kernel sweeps windows and falls back to the exact scan as before.
    T.blk = nullptr; T.bandmm = nullptr; T.blk4 = nullptr; T.cellmm = nullptr;
    static const bool blocks_off = env_flag("XSW_NO_BLOCKS");
    if (req.ok() && !blocks_off && g.blk_ok) {
        DevSeq opt{st, c->co_allocs};
        float2 *d_blk = opt.table<float2>((size_t)g.nblk), *d_band = opt.table<float2>((size_t)g.nband);
        opt.run([&] {
            hipLaunchKernelGGL(k_block_minmax, dim3(blocks_of_256(g.nblk)), dim3(256), 0, st, d_dense, nI, nW, nP, g.nbr, g.nbc, d_blk);
            hipLaunchKernelGGL(k_band_minmax, dim3(blocks_of_256(g.nband)), dim3(256), 0, st, d_blk, nI, g.nbr, g.nbc, g.blk_g, g.nbands, d_band);
        });
        // level 1 of k_invert_blocks: cells of XSW_CELL_R x XSW_CELL_C blocks (a band over ALL directions has a sigma0 range that
        // holds nearly any s and no sector bound: 401 blocks left to bound per outlier pixel where these cells leave 70)
        float2 *d_cell = opt.table<float2>((size_t)g.ncell);
        opt.run([&] {
            hipLaunchKernelGGL(k_block_minmax, dim3(blocks_of_256(g.ncell)), dim3(256), 0, st, d_dense, nI, nW, nP, g.ncr, g.ncc, d_cell,
                               XSW_CELL_C * XSW_BLK_C, XSW_CELL_R * XSW_BLK_R);
        });
        if (opt.usable()) { T.blk = d_blk; T.bandmm = d_band; T.cellmm = d_cell; }
        // the same per sub-block of XSW_BLK_C4 directions (k_invert_blocks bounds the quarters of a kept block before sweeping:
        // sigma0 varies faster with the direction than with the speed where the GMF saturates, so a block 16 directions wide
        // nearly always straddles the contour); 23 MB at the default size.  XSW_NO_BLK4=1: not built (A/B, tests of the old sweep)
        static const bool blk4_off = env_flag("XSW_NO_BLK4");
        if (T.blk && !blk4_off && g.blk4_ok) {
            DevSeq opt4{st, c->co_allocs};
            float2 *d_blk4 = opt4.table<float2>((size_t)g.nblk4);
            opt4.run([&] { hipLaunchKernelGGL(k_block_minmax, dim3(blocks_of_256(g.nblk4)), dim3(256), 0, st, d_dense, nI, nW, nP, g.nbr, g.nbc4, d_blk4, XSW_BLK_C4); });
            if (opt4.usable()) T.blk4 = d_blk4;
        }
    }

    // the flags come back; the temporaries (and `init`) are done with once the stream is
    if (req.ok()) req.check(hipMemcpyAsync(h_flags, d_flags, sizeof h_flags, hipMemcpyDeviceToHost, st));
    req.check(tmp.finish());
    if (!req.ok()) return fail(c, req.code(), "LUT install failed: %s", hipGetErrorString(req.err));
    T.co = d_co;
    T.co32 = d_co32;
    const bool lut_finite = h_flags[0] == 0;
    c->co_finite = lut_finite;
    memcpy(&T.co_absmax, &h_flags[1], sizeof(double));

    // host-built tables: the axes as they are; the output-side tables are the caller's values, or the host libm's (see xsw.h)
    CoHostTables H(l);
    DevSeq up{st, c->co_allocs};
    T.inc = up.table((size_t)nI, l->inc);
    T.w = up.table((size_t)nW, l->wspd);
    T.wh = up.table(H.wh);
    T.wh32 = up.table(H.wh32);
    T.phi = up.table((size_t)nP, l->phi);
    T.cphi = up.table(H.cphi);
    T.sphi = up.table(H.sphi);
    T.csphi = up.table(H.csphi);
    T.csphi32 = up.table(H.csphi32);
    T.out_dir = up.table(H.out_dir);
    T.abs_co = up.table(H.abs_co);
    T.dual_dir = up.table(H.dual_dir);
    T.sol = up.table(H.sol);
    if (!up.ok()) return fail(c, up.code(), "LUT install failed: %s", hipGetErrorString(up.err));
    c->h_sol32.swap(H.sol32);
    c->h_sol.swap(H.sol);
    c->h_dual.swap(H.dual_dir);

    co_scalars(T, l, g, lut_finite, H.trig_ok);

    // transposed slices for the ray scan
    double *dT = (double *)up.alloc(g.coT_n * sizeof(double));
    up.zero(dT, g.coT_n * sizeof(double));
    up.run([&] { hipLaunchKernelGGL(k_transpose_slices, dim3((nP + 31) / 32, (nW + 31) / 32, nI), dim3(256), 0, st, T.co, dT, nW, nP, g.ppad, g.wpad); });
    if (up.ok()) up.check(hipStreamSynchronize(st));
    if (!up.ok()) return fail(c, up.code(), "LUT install failed: %s", hipGetErrorString(up.err));
    T.coT = dT;
    c->have_co = true;
    return XSW_OK;
}

static int upload_cr(xsw_ctx *c, const xsw_lut *l)
{
    if (!l->db || !l->inc || !l->wspd || l->n_inc < 1 || l->n_wspd < 1)
        return fail(c, XSW_EINVAL, "cross-pol LUT: null pointer or empty axis");
    if (!strictly_ascending(l->inc, l->n_inc) || !strictly_ascending(l->wspd, l->n_wspd))
        return fail(c, XSW_EINVAL, "cross-pol LUT: axes must be strictly ascending");
    HIPCHK(c, hipStreamSynchronize(c->stream));  // a queued search may still read the old tables (install_co)
    free_all(c->cr_allocs);
    c->have_cr = false;
    DevTables &T = c->T;
    const CrPlan p(l);
    DevSeq up{c->stream, c->cr_allocs};
    T.cr = up.table(p.pad);
    T.inc_cr = up.table((size_t)l->n_inc, l->inc);
    T.wcr = up.table((size_t)l->n_wspd, l->wspd);
    T.wcrh = up.table(p.wh);
    T.inv_cr = p.inv.empty() ? nullptr : up.table(p.inv);
    T.inv_cr_grid = p.inv.empty() ? nullptr : up.table(p.grid);
    if (!up.ok()) return fail(c, up.code(), "LUT install failed: %s", hipGetErrorString(up.err));
    c->h_wcr.assign(l->wspd, l->wspd + l->n_wspd);
    cr_scalars(T, l, p);
    c->have_cr = true;
    return XSW_OK;
}

extern "C" int xsw_lut_upload(xsw_ctx *c, const xsw_lut *co, const xsw_lut *cr)
{
    if (!c) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if (co && (rc = install_co(c, co, nullptr))) return rc;
    if (cr && (rc = upload_cr(c, cr))) return rc;
    return XSW_OK;
}

extern "C" int xsw_lut_read(xsw_ctx *c, int32_t cross, double *out_db)
{
    if (!c || !out_db) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const DevTables &T = c->T;
    if (cross ? !c->have_cr : !c->have_co) return fail(c, XSW_ENOLUT, "lut_read: no such LUT on this context");
    if (cross)
        HIPCHK(c, hipMemcpy2DAsync(out_db, (size_t)T.n_wcr * 8, T.cr, (size_t)T.wcr_pad * 8, (size_t)T.n_wcr * 8, (size_t)T.n_inc_cr,
                                   hipMemcpyDeviceToHost, c->stream));
    else
        HIPCHK(c, hipMemcpy2DAsync(out_db, (size_t)T.n_phi * 8, T.co, (size_t)T.phi_pad * 8, (size_t)T.n_phi * 8,
                                   (size_t)T.n_inc * T.n_w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return XSW_OK;
}

// Diagnostic: one derived table of the current co-pol install, whole (pads and slack included), or the install's scalars.
// Element counts from CoGeometry, as install_co allocated them.  Read-only, no kernel.
extern "C" int xsw_lut_table_read(xsw_ctx *c, int32_t which, void *out, size_t bytes)
{
    if (!c || !out) return XSW_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->have_co) return fail(c, XSW_ENOLUT, "lut_table_read: no co-pol LUT on this context");
    const DevTables &T = c->T;
    const CoGeometry g{T.n_inc, T.n_w, T.n_phi};
    const void *src = nullptr;
    size_t want = 0;
    switch (which) {
    case XSW_TAB_CO: src = T.co; want = g.n_pad * sizeof(double); break;
    case XSW_TAB_CO32: src = T.co32; want = g.n_pad * sizeof(float); break;
    case XSW_TAB_COT: src = T.coT; want = g.coT_n * sizeof(double); break;
    case XSW_TAB_MONO_ROWS: src = T.mono_rows; want = (size_t)g.n_inc * sizeof(int); break;
    case XSW_TAB_TAIL_MIN: src = T.tail_min; want = g.tail_n * sizeof(double); break;
    case XSW_TAB_INV_GRID: src = T.inv_grid; want = g.inv_grid_n * sizeof(double); break;
    case XSW_TAB_INV_ROWS: src = T.inv_rows; want = g.inv_n * sizeof(unsigned short); break;
    case XSW_TAB_BLK: src = T.blk; want = (size_t)g.nblk * sizeof(float2); break;
    case XSW_TAB_BLK4: src = T.blk4; want = (size_t)g.nblk4 * sizeof(float2); break;
    case XSW_TAB_CELLMM: src = T.cellmm; want = (size_t)g.ncell * sizeof(float2); break;
    case XSW_TAB_BANDMM: src = T.bandmm; want = (size_t)g.nband * sizeof(float2); break;
    case XSW_TAB_SCALARS: want = 3 * sizeof(double); break;
    default: return fail(c, XSW_EINVAL, "lut_table_read: unknown table id %d", (int)which);
    }
    if (which != XSW_TAB_SCALARS && !src) return XSW_TAB_ABSENT;  // an optional table this install did not build
    if (bytes != want) return fail(c, XSW_EINVAL, "lut_table_read: table %d holds %zu bytes, the buffer %zu", (int)which, want, bytes);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (which == XSW_TAB_SCALARS) {
        const double s[3] = {c->co_finite ? 1.0 : 0.0, T.co_absmax, (double)T.prunable};
        memcpy(out, s, sizeof s);
        return XSW_OK;
    }
    HIPCHK(c, hipMemcpy(out, src, want, hipMemcpyDeviceToHost));
    return XSW_OK;
}

// ---------------------------------------------------------------------------------------- invert
static int dispatch_invert(xsw_ctx *c, const KArgs &A, int dtype, int out_dtype, int algo, const LaunchCtl &lc, std::string &err)
{
    return pair_launch(dtype, out_dtype).invert(c, A, algo, lc, err);
}

// Work lists of the device-raster path (capacities: xsw_plan.hpp).  A failed allocation selects the one-kernel path.
static void ensure_list(xsw_ctx *c, long long n, long long lines)
{
    const RouteKnobs &knobs = route_knobs();  // list_cap_test, fail_list_alloc: the tests' overflow and allocation-failure routes
    const size_t want = context_list_cap(n, knobs.list_cap_test), want_strips = strips_for(n, lines);
    if (want <= c->lists.list_cap && want_strips <= c->lists.mask_strips) return;
    (void)hipStreamSynchronize(c->stream);  // the old lists may still be in use
    c->lists.list_cap = c->lists.mask_strips = 0;  // (no lists: the one-kernel path)
    if (grow(c->lists.base, c->lists_bytes, knobs.fail_list_alloc ? 0 : WorkLists{nullptr, want, want_strips}.bytes()) != hipSuccess) (void)hipGetLastError();
    if (c->lists.base) { c->lists.list_cap = want; c->lists.mask_strips = want_strips; }
}

// ---- grid codes -> complex winds (xsw.h: xsw_expand_codes; the codes and their winds: xsw_codes.hpp, expand_co / expand_cr)
template <typename TO>
__global__ __launch_bounds__(256) void k_expand(const double *__restrict__ sol, const double *__restrict__ dual_dir, const double *__restrict__ wcr,
                                                long long plane, int n_wcr, long long n, const unsigned *__restrict__ cc, const unsigned *__restrict__ cr,
                                                typename Cx<TO>::type *__restrict__ out_co, typename Cx<TO>::type *__restrict__ out_cr)
{
    typedef typename Cx<TO>::type cx_t;
    const auto read = [](const double *table, long long k) { const double2 z = ((const double2 *)table)[k]; return Wind{z.x, z.y}; };
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        Wind co;
        const CoPoint p = expand_co(cc ? cc[i] : XSW_CODE_NAN, plane, sol, read, co);
        if (out_co) { cx_t z; z.x = (TO)co.re; z.y = (TO)co.im; out_co[i] = z; }
        if (out_cr && cr) {
            const Wind dual = expand_cr(cr[i], p, co, n_wcr, dual_dir, wcr, read);
            cx_t z; z.x = (TO)dual.re; z.y = (TO)dual.im; out_cr[i] = z;
        }
    }
}

template <typename V>
static inline void stream_store(V *p, V v)  // non-temporal when the address allows it: the output rasters are written once
{
    if (((uintptr_t)p & (sizeof(V) - 1)) == 0) __builtin_nontemporal_store(v, p);
    else memcpy(p, &v, sizeof(V));
}

// Host counterpart of store_pixel / k_expand: the same table values, the same IEEE operations (this file is compiled with
// -ffp-contract=off) -- the bits the device would have stored.  idx: optional int32[n][3] as xsw_invert's out_idx.
template <typename TO>
static void expand_host(const xsw_ctx *c, size_t n, const uint32_t *cc, const uint32_t *cr, TO *out_co, TO *out_cr, int32_t *idx)
{
    typedef TO cx_t __attribute__((ext_vector_type(2)));
    const long long plane = (long long)c->T.n_w * c->T.n_phi, n_wcr = (long long)c->h_wcr.size();
    const int nP = c->T.n_phi;
    const auto read = [](const double *table, long long k) { return Wind{table[2 * k], table[2 * k + 1]}; };
    for (size_t i = 0; i < n; ++i) {
        Wind co;
        const unsigned a = cc ? cc[i] : XSW_CODE_NAN;
        const CoPoint p = expand_co(a, plane, c->h_sol.data(), read, co);
        if (out_co) { cx_t z; z.x = (TO)co.re; z.y = (TO)co.im; stream_store((cx_t *)(out_co + 2 * i), z); }
        if (cr && out_cr) {
            const Wind dual = expand_cr(cr[i], p, co, n_wcr, c->h_dual.data(), c->h_wcr.data(), read);
            cx_t z; z.x = (TO)dual.re; z.y = (TO)dual.im; stream_store((cx_t *)(out_cr + 2 * i), z);
        }
        if (idx) {
            const CrCode b = cr_decode(cr ? cr[i] : XSW_CODE_NO_INDEX);
            const int flat = (int)co_decode(a, plane).flat();
            idx[3 * i + 0] = p.have ? flat / nP : -1;
            idx[3 * i + 1] = p.have ? flat % nP : -1;
            idx[3 * i + 2] = (b.nan_re() || b.foreign() || b.index() == XSW_CODE_NO_INDEX) ? -1 : (int)b.index();
        }
    }
}

static int check_codes_tables(xsw_ctx *c, const uint32_t *code_co, const uint32_t *code_cr)
{
    if (code_co && !c->have_co) return fail(c, XSW_ENOLUT, "co-pol codes given but no co-pol LUT on this context");
    if (code_cr && !c->have_cr) return fail(c, XSW_ENOLUT, "cross-pol codes given but no cross-pol LUT on this context");
    return XSW_OK;
}

static int expand_codes_on(xsw_ctx *c, hipStream_t stream, int64_t n, int32_t mem, int32_t out_dtype, const uint32_t *code_co,
                           const uint32_t *code_cr, void *out_co, void *out_cr);

extern "C" int xsw_expand_codes(xsw_ctx *c, int64_t n, int32_t mem, int32_t out_dtype, const uint32_t *code_co,
                                const uint32_t *code_cr, void *out_co, void *out_cr)
{
    if (!c) return XSW_EINVAL;
    return expand_codes_on(c, c->stream, n, mem, out_dtype, code_co, code_cr, out_co, out_cr);
}

extern "C" int xsw_expand_codes_on_stream(xsw_ctx *c, void *stream, int64_t n, int32_t out_dtype, const uint32_t *code_co,
                                          const uint32_t *code_cr, void *out_co, void *out_cr)
{
    if (!c) return XSW_EINVAL;
    return expand_codes_on(c, (hipStream_t)stream, n, XSW_MEM_DEVICE, out_dtype, code_co, code_cr, out_co, out_cr);
}

static int expand_codes_on(xsw_ctx *c, hipStream_t stream, int64_t n, int32_t mem, int32_t out_dtype, const uint32_t *code_co,
                           const uint32_t *code_cr, void *out_co, void *out_cr)
{
    if (n < 0 || (!code_co && !code_cr)) return fail(c, XSW_EINVAL, "expand_codes: no codes");
    if (out_dtype != XSW_F32 && out_dtype != XSW_F64) return fail(c, XSW_EINVAL, "out_dtype must be XSW_F32 or XSW_F64");
    if ((out_co && !code_co) || (out_cr && !code_cr)) return fail(c, XSW_EINVAL, "expand_codes: an output without its codes");
    int rc = check_codes_tables(c, code_co, code_cr);
    if (rc) return rc;
    if (n == 0) return XSW_OK;
    if (mem == XSW_MEM_DEVICE) {
        HIPCHK(c, hipSetDevice(c->device));
        const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 256 * 16);
        const long long plane = (long long)c->T.n_w * c->T.n_phi;
        if (out_dtype == XSW_F32)
            hipLaunchKernelGGL((k_expand<float>), dim3(blocks), dim3(256), 0, stream, c->T.sol, c->T.dual_dir, c->T.wcr, plane, c->have_cr ? c->T.n_wcr : 0, (long long)n, code_co,
                               code_cr, (Cx<float>::type *)out_co, (Cx<float>::type *)out_cr);
        else
            hipLaunchKernelGGL((k_expand<double>), dim3(blocks), dim3(256), 0, stream, c->T.sol, c->T.dual_dir, c->T.wcr, plane, c->have_cr ? c->T.n_wcr : 0, (long long)n, code_co,
                               code_cr, (Cx<double>::type *)out_co, (Cx<double>::type *)out_cr);
        HIPCHK(c, hipGetLastError());
        return XSW_OK;
    }
    if (out_dtype == XSW_F32) expand_host<float>(c, (size_t)n, code_co, code_cr, (float *)out_co, (float *)out_cr, nullptr);
    else expand_host<double>(c, (size_t)n, code_co, code_cr, (double *)out_co, (double *)out_cr, nullptr);
    return XSW_OK;
}

// ---- the one-pixel-per-lane passes over rasters and the context's tables.  Every entry: check_raster_call, its own refusals,
// pixel_count (xsw_run.hpp), then run(); every check comes before any launch.
// queue(member, A, cr...): the launch of PairLaunch `member` on the context's stream, its message moved into c->err
template <typename Member, typename Args, typename... Cr>
static int queue(xsw_ctx *c, int32_t dtype, int32_t out_dtype, Member member, const Args &A, Cr... cr)
{
    std::string err;
    const int rc = (pair_launch(dtype, out_dtype).*member)(c, A, cr..., c->stream, err);
    return rc ? fail(c, rc, "%s", err.c_str()) : XSW_OK;
}

// ---- the cross-pol step from stored co-pol codes (xsw.h: xsw_cross_from_codes; kernel: xsw_cross.hpp)
extern "C" int xsw_cross_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                    int32_t sigma0_is_db, int32_t dual_select, const void *inc, const uint32_t *code_co,
                                    const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, uint32_t *out_code_cr, void *out_cr)
{
    if (!c) return XSW_EINVAL;
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!inc || !sigma0_cr) return fail(c, XSW_EINVAL, "cross_from_codes: inc or sigma0_cr is NULL");
    if (!out_code_cr && !out_cr) return fail(c, XSW_EINVAL, "cross_from_codes: neither out_code_cr nor out_cr given");
    if (!c->have_cr) return fail(c, XSW_ENOLUT, "cross_from_codes: no cross-pol LUT uploaded");
    if (code_co && !c->have_co) return fail(c, XSW_ENOLUT, "co-pol codes given but no co-pol LUT on this context");
    long long n;
    size_t es, os;
    if (int rc = pixel_count(c, "cross_from_codes", lines, samples, dtype, out_dtype, n, es, os)) return rc;
    if (n == 0) return XSW_OK;
    const size_t px = (size_t)n;
    Buf b[6] = {in_buf(inc, px * es), in_buf(sigma0_cr, px * es), in_buf(dsig_cr, px * es), in_buf(code_co, px * 4),
                out_buf(out_code_cr, px * 4), out_buf(out_cr, px * os * 2)};
    return run(c, mem, b, [&](Buf (&x)[6]) {
        const CrossArgs A{x[0].dev, x[1].dev, x[2].dev, (const unsigned *)x[3].dev, (unsigned *)x[4].dev, x[5].dev, n, dsig_cr_scalar,
                          sigma0_is_db, dual_select};
        return queue(c, dtype, out_dtype, &PairLaunch::cross, A);
    }, "cross_from_codes");
}

// ---- inversion cost / sigma0 residual and wind uncertainty from stored codes (xsw.h: xsw_cost_from_codes, xsw_cost_cr_from_codes,
// xsw_uncertainty_from_codes, xsw_uncertainty_cr_from_codes; kernels: xsw_cost.hpp, xsw_uncertainty.hpp).  One body for the four
// entries: A holds the caller's pointers (cr: a cross-pol entry), `outs` names A's four outputs, the last of last_elem bytes per
// pixel (0: a real of the output dtype, as the other three), `member` is the PairLaunch entry that runs.
template <typename Args>
static int pass_from_codes(xsw_ctx *c, const char *who, bool cr, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                           Args A, void *Args::*const (&outs)[4], size_t last_elem,
                           int (*PairLaunch::*member)(xsw_ctx *, const Args &, bool, hipStream_t, std::string &))
{
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!A.inc || !A.s || (cr ? !A.code_cr : (!A.code_co || !A.anc))) return fail(c, XSW_EINVAL, "%s: an input raster is NULL", who);
    if (!(A.*outs[0]) && !(A.*outs[1]) && !(A.*outs[2]) && !(A.*outs[3])) return fail(c, XSW_EINVAL, "%s: no output requested", who);
    if (cr ? !c->have_cr : !c->have_co) return fail(c, XSW_EINVAL, "%s: no %s LUT installed", who, cr ? "cross-pol" : "co-pol");
    if (cr && A.code_co && !c->have_co) return fail(c, XSW_EINVAL, "%s: co-pol codes given but no co-pol LUT installed", who);
    if (!cr && (A.dsig_co != A.dsig_co || A.dsig_co == 0.0)) return fail(c, XSW_EINVAL, "%s: dsig_co is NaN or 0", who);
    size_t es, os;
    if (int rc = pixel_count(c, who, lines, samples, dtype, out_dtype, A.n, es, os)) return rc;
    if (A.n == 0) return XSW_OK;
    const size_t px = (size_t)A.n;
    Buf b[10] = {in_buf(A.inc, px * es), in_buf(A.s, px * es), in_buf(A.anc, px * es * 2), in_buf(A.dsig_cr, px * es),
                 in_buf(A.code_co, px * 4), in_buf(A.code_cr, px * 4), out_buf(A.*outs[0], px * os), out_buf(A.*outs[1], px * os),
                 out_buf(A.*outs[2], px * os), out_buf(A.*outs[3], px * (last_elem ? last_elem : os))};
    return run(c, mem, b, [&](Buf (&x)[10]) {
        A.inc = x[0].dev; A.s = x[1].dev; A.anc = x[2].dev; A.dsig_cr = x[3].dev;
        A.code_co = (const unsigned *)x[4].dev; A.code_cr = (const unsigned *)x[5].dev;
        for (int k = 0; k < 4; ++k) A.*outs[k] = x[6 + k].dev;
        return queue(c, dtype, out_dtype, member, A, cr);
    }, who);
}

static void *CostArgs::*const cost_outs[4] = {&CostArgs::out_J, &CostArgs::out_Jsig, &CostArgs::out_Jwind, &CostArgs::out_res};
static void *UncArgs::*const unc_outs[4] = {&UncArgs::out_wspd_std, &UncArgs::out_dir_std, &UncArgs::out_corr, &UncArgs::out_flag};

extern "C" int xsw_cost_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                   int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const void *sigma0_co, const void *anc,
                                   double dsig_co, void *out_J, void *out_Jsig, void *out_Jwind, void *out_residual)
{
    if (!c) return XSW_EINVAL;
    CostArgs A{};
    A.inc = inc; A.s = sigma0_co; A.anc = anc; A.code_co = code_co;
    A.out_J = out_J; A.out_Jsig = out_Jsig; A.out_Jwind = out_Jwind; A.out_res = out_residual;
    A.dsig_co = dsig_co; A.is_db = sigma0_is_db;
    return pass_from_codes(c, "cost_from_codes", false, lines, samples, dtype, out_dtype, mem, A, cost_outs, 0, &PairLaunch::cost);
}

extern "C" int xsw_cost_cr_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                      int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const uint32_t *code_cr,
                                      const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, void *out_J, void *out_Jsig,
                                      void *out_Jwind, void *out_residual)
{
    if (!c) return XSW_EINVAL;
    CostArgs A{};
    A.inc = inc; A.s = sigma0_cr; A.dsig_cr = dsig_cr; A.code_co = code_co; A.code_cr = code_cr;
    A.out_J = out_J; A.out_Jsig = out_Jsig; A.out_Jwind = out_Jwind; A.out_res = out_residual;
    A.dsig_cr_scalar = dsig_cr_scalar; A.is_db = sigma0_is_db;
    return pass_from_codes(c, "cost_cr_from_codes", true, lines, samples, dtype, out_dtype, mem, A, cost_outs, 0, &PairLaunch::cost);
}

extern "C" int xsw_uncertainty_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                          int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const void *sigma0_co,
                                          const void *anc, double dsig_co, void *out_wspd_std, void *out_dir_std, void *out_corr,
                                          uint8_t *out_flag)
{
    if (!c) return XSW_EINVAL;
    UncArgs A{};
    A.inc = inc; A.s = sigma0_co; A.anc = anc; A.code_co = code_co;
    A.out_wspd_std = out_wspd_std; A.out_dir_std = out_dir_std; A.out_corr = out_corr; A.out_flag = out_flag;
    A.dsig_co = dsig_co; A.is_db = sigma0_is_db;
    return pass_from_codes(c, "uncertainty_from_codes", false, lines, samples, dtype, out_dtype, mem, A, unc_outs, 1, &PairLaunch::unc);
}

extern "C" int xsw_uncertainty_cr_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                             int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const uint32_t *code_cr,
                                             const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, void *out_wspd_std,
                                             uint8_t *out_flag)
{
    if (!c) return XSW_EINVAL;
    UncArgs A{};
    A.inc = inc; A.s = sigma0_cr; A.dsig_cr = dsig_cr; A.code_co = code_co; A.code_cr = code_cr;
    A.out_wspd_std = out_wspd_std; A.out_flag = out_flag;
    A.dsig_cr_scalar = dsig_cr_scalar; A.is_db = sigma0_is_db;
    return pass_from_codes(c, "uncertainty_cr_from_codes", true, lines, samples, dtype, out_dtype, mem, A, unc_outs, 1, &PairLaunch::unc);
}

// ---- the joint dual-pol inversion from stored co-pol codes (xsw.h: xsw_joint_from_codes; kernel: xsw_joint.hpp)
extern "C" int xsw_joint_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                    int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const void *sigma0_co, const void *anc,
                                    double dsig_co, const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, uint32_t *out_code,
                                    void *out_J, void *out_Jwind, void *out_Jsig_co, void *out_Jsig_cr)
{
    if (!c) return XSW_EINVAL;
    const char *who = "joint_from_codes";
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!inc || !code_co || !sigma0_co || !anc || !sigma0_cr) return fail(c, XSW_EINVAL, "%s: an input raster is NULL", who);
    if (!out_code && !out_J && !out_Jwind && !out_Jsig_co && !out_Jsig_cr) return fail(c, XSW_EINVAL, "%s: no output requested", who);
    if (!c->have_co || !c->have_cr) return fail(c, XSW_ENOLUT, "%s: needs a co-pol and a cross-pol LUT on this context", who);
    if (dsig_co != dsig_co || dsig_co == 0.0) return fail(c, XSW_EINVAL, "%s: dsig_co is NaN or 0", who);
    if (!c->co_finite || !c->T.cr_finite) return fail(c, XSW_EINVAL, "%s: a LUT with a NaN or infinite entry", who);
    JointArgs A{};
    size_t es, os;
    if (int rc = pixel_count(c, who, lines, samples, dtype, out_dtype, A.n, es, os)) return rc;
    if (A.n == 0) return XSW_OK;
    A.dsig_co = dsig_co; A.dsig_cr_scalar = dsig_cr_scalar; A.is_db = sigma0_is_db;
    const size_t px = (size_t)A.n;
    Buf b[11] = {in_buf(inc, px * es), in_buf(sigma0_co, px * es), in_buf(anc, px * es * 2), in_buf(sigma0_cr, px * es), in_buf(dsig_cr, px * es),
                 in_buf(code_co, px * 4), out_buf(out_code, px * 4), out_buf(out_J, px * os), out_buf(out_Jwind, px * os),
                 out_buf(out_Jsig_co, px * os), out_buf(out_Jsig_cr, px * os)};
    return run(c, mem, b, [&](Buf (&x)[11]) {
        A.inc = x[0].dev; A.s_co = x[1].dev; A.anc = x[2].dev; A.s_cr = x[3].dev; A.dsig_cr = x[4].dev;
        A.code_co = (const unsigned *)x[5].dev; A.out_code = (unsigned *)x[6].dev;
        A.out_J = x[7].dev; A.out_Jwind = x[8].dev; A.out_Jsig_co = x[9].dev; A.out_Jsig_cr = x[10].dev;
        if (c->stats_on) {  // candidates scored per pixel (xsw_stats_read: pixels_co, cand_co), reset on the launch stream
            if (hipMemsetAsync(c->d_stats, 0, 8 * sizeof(unsigned long long), c->stream) != hipSuccess) return fail(c, XSW_EHIP, "%s: statistics reset failed", who);
            A.stats = c->d_stats;
        }
        return queue(c, dtype, out_dtype, &PairLaunch::joint, A);
    }, who);
}

// ---- the error bars of the joint solution (xsw.h: xsw_uncertainty_joint_from_codes; kernel: xsw_uncertainty_joint.hpp).  The refusals are
// xsw_joint_from_codes', except that a non-finite table entry is none: nothing here is an arg-min, such a stencil ends in NOT_CONVEX.
extern "C" int xsw_uncertainty_joint_from_codes(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                                int32_t sigma0_is_db, const void *inc, const uint32_t *code, const void *sigma0_co,
                                                const void *anc, double dsig_co, const void *sigma0_cr, const void *dsig_cr,
                                                double dsig_cr_scalar, void *out_wspd_std, void *out_dir_std, void *out_corr,
                                                void *out_u_std, void *out_v_std, void *out_corr_uv, uint8_t *out_flag)
{
    if (!c) return XSW_EINVAL;
    const char *who = "uncertainty_joint_from_codes";
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!inc || !code || !sigma0_co || !anc || !sigma0_cr) return fail(c, XSW_EINVAL, "%s: an input raster is NULL", who);
    if (!out_wspd_std && !out_dir_std && !out_corr && !out_u_std && !out_v_std && !out_corr_uv && !out_flag)
        return fail(c, XSW_EINVAL, "%s: no output requested", who);
    if (!c->have_co || !c->have_cr) return fail(c, XSW_ENOLUT, "%s: needs a co-pol and a cross-pol LUT on this context", who);
    if (dsig_co != dsig_co || dsig_co == 0.0) return fail(c, XSW_EINVAL, "%s: dsig_co is NaN or 0", who);
    UncJointArgs A{};
    size_t es, os;
    if (int rc = pixel_count(c, who, lines, samples, dtype, out_dtype, A.n, es, os)) return rc;
    if (A.n == 0) return XSW_OK;
    A.dsig_co = dsig_co; A.dsig_cr_scalar = dsig_cr_scalar; A.is_db = sigma0_is_db;
    const size_t px = (size_t)A.n;
    Buf b[13] = {in_buf(inc, px * es), in_buf(sigma0_co, px * es), in_buf(anc, px * es * 2), in_buf(sigma0_cr, px * es), in_buf(dsig_cr, px * es),
                 in_buf(code, px * 4), out_buf(out_wspd_std, px * os), out_buf(out_dir_std, px * os), out_buf(out_corr, px * os),
                 out_buf(out_u_std, px * os), out_buf(out_v_std, px * os), out_buf(out_corr_uv, px * os), out_buf(out_flag, px)};
    return run(c, mem, b, [&](Buf (&x)[13]) {
        A.inc = x[0].dev; A.s_co = x[1].dev; A.anc = x[2].dev; A.s_cr = x[3].dev; A.dsig_cr = x[4].dev;
        A.code_co = (const unsigned *)x[5].dev;
        A.out_wspd_std = x[6].dev; A.out_dir_std = x[7].dev; A.out_corr = x[8].dev;
        A.out_u_std = x[9].dev; A.out_v_std = x[10].dev; A.out_corr_uv = x[11].dev; A.out_flag = x[12].dev;
        return queue(c, dtype, out_dtype, &PairLaunch::unc_joint, A);
    }, who);
}

// ---- the forward operator on rasters (xsw.h: xsw_lut_eval, xsw_lut_eval_cr; kernels: xsw_forward.hpp)
// One body for the two entries: A holds the caller's pointers.
static int lut_eval(xsw_ctx *c, const char *who, bool cr, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                    FwdArgs A)
{
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!A.inc || !A.wspd || (!cr && !A.phi)) return fail(c, XSW_EINVAL, "%s: an input raster is NULL", who);
    if (!A.out_db && !A.out_dwspd && !A.out_dphi) return fail(c, XSW_EINVAL, "%s: no output requested", who);
    if (cr ? !c->have_cr : !c->have_co) return fail(c, XSW_ENOLUT, "%s: no %s LUT installed", who, cr ? "cross-pol" : "co-pol");
    if (cr ? (c->T.n_inc_cr < 2 || c->T.n_wcr < 2) : (c->T.n_inc < 2 || c->T.n_w < 2 || c->T.n_phi < 2))  // (no cell to interpolate in)
        return fail(c, XSW_EINVAL, "%s: an axis of the %s LUT has fewer than two points", who, cr ? "cross-pol" : "co-pol");
    size_t es, os;
    if (int rc = pixel_count(c, who, lines, samples, dtype, out_dtype, A.n, es, os)) return rc;
    if (A.n == 0) return XSW_OK;
    const size_t px = (size_t)A.n;
    Buf b[6] = {in_buf(A.inc, px * es), in_buf(A.wspd, px * es), in_buf(A.phi, px * es),
                out_buf(A.out_db, px * os), out_buf(A.out_dwspd, px * os), out_buf(A.out_dphi, px * os)};
    return run(c, mem, b, [&](Buf (&x)[6]) {
        A.inc = x[0].dev; A.wspd = x[1].dev; A.phi = x[2].dev;
        A.out_db = x[3].dev; A.out_dwspd = x[4].dev; A.out_dphi = x[5].dev;
        return queue(c, dtype, out_dtype, &PairLaunch::fwd, A, cr);
    }, who);
}

extern "C" int xsw_lut_eval(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, int32_t fold_phi,
                            const void *inc, const void *wspd, const void *phi, void *out_db, void *out_dwspd, void *out_dphi)
{
    if (!c) return XSW_EINVAL;
    FwdArgs A{};
    A.inc = inc; A.wspd = wspd; A.phi = phi;
    A.out_db = out_db; A.out_dwspd = out_dwspd; A.out_dphi = out_dphi;
    A.fold_phi = fold_phi != 0;
    return lut_eval(c, "lut_eval", false, lines, samples, dtype, out_dtype, mem, A);
}

extern "C" int xsw_lut_eval_cr(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, const void *inc,
                               const void *wspd, void *out_db, void *out_dwspd)
{
    if (!c) return XSW_EINVAL;
    FwdArgs A{};
    A.inc = inc; A.wspd = wspd;
    A.out_db = out_db; A.out_dwspd = out_dwspd;
    return lut_eval(c, "lut_eval_cr", true, lines, samples, dtype, out_dtype, mem, A);
}

// ---- wind speed at a known direction (xsw.h: xsw_wspd_solve, xsw_wspd_solve_cr; kernels: xsw_solve.hpp)
// One body for the two entries: A holds the caller's pointers.
static int wspd_solve(xsw_ctx *c, const char *who, bool cr, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                      SolveArgs A)
{
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!A.inc || !A.s || (!cr && !A.phi)) return fail(c, XSW_EINVAL, "%s: an input raster is NULL", who);
    if (!A.out_wspd && !A.out_sens && !A.out_flag) return fail(c, XSW_EINVAL, "%s: no output requested", who);
    if (cr ? !c->have_cr : !c->have_co) return fail(c, XSW_ENOLUT, "%s: no %s LUT installed", who, cr ? "cross-pol" : "co-pol");
    if (cr ? (c->T.n_inc_cr < 2 || c->T.n_wcr < 2) : (c->T.n_inc < 2 || c->T.n_w < 2 || c->T.n_phi < 2))  // (no cell to solve in)
        return fail(c, XSW_EINVAL, "%s: an axis of the %s LUT has fewer than two points", who, cr ? "cross-pol" : "co-pol");
    size_t es, os;
    if (int rc = pixel_count(c, who, lines, samples, dtype, out_dtype, A.n, es, os)) return rc;
    if (A.n == 0) return XSW_OK;
    const size_t px = (size_t)A.n;
    Buf b[6] = {in_buf(A.inc, px * es), in_buf(A.s, px * es), in_buf(A.phi, px * es),
                out_buf(A.out_wspd, px * os), out_buf(A.out_sens, px * os), out_buf(A.out_flag, px)};
    return run(c, mem, b, [&](Buf (&x)[6]) {
        A.inc = x[0].dev; A.s = x[1].dev; A.phi = x[2].dev;
        A.out_wspd = x[3].dev; A.out_sens = x[4].dev; A.out_flag = x[5].dev;
        return queue(c, dtype, out_dtype, &PairLaunch::solve, A, cr);
    }, who);
}

extern "C" int xsw_wspd_solve(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, int32_t fold_phi,
                              const void *inc, const void *sigma0_db, const void *phi, void *out_wspd, void *out_sens, uint8_t *out_flag)
{
    if (!c) return XSW_EINVAL;
    SolveArgs A{};
    A.inc = inc; A.s = sigma0_db; A.phi = phi;
    A.out_wspd = out_wspd; A.out_sens = out_sens; A.out_flag = out_flag;
    A.fold_phi = fold_phi != 0;
    return wspd_solve(c, "wspd_solve", false, lines, samples, dtype, out_dtype, mem, A);
}

extern "C" int xsw_wspd_solve_cr(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, const void *inc,
                                 const void *sigma0_db, void *out_wspd, void *out_sens, uint8_t *out_flag)
{
    if (!c) return XSW_EINVAL;
    SolveArgs A{};
    A.inc = inc; A.s = sigma0_db;
    A.out_wspd = out_wspd; A.out_sens = out_sens; A.out_flag = out_flag;
    return wspd_solve(c, "wspd_solve_cr", true, lines, samples, dtype, out_dtype, mem, A);
}

// ---- wind direction at a known speed (xsw.h: xsw_dir_solve; kernel: xsw_dirsolve.hpp)
extern "C" int xsw_dir_solve(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, int32_t fold_phi,
                             const void *inc, const void *sigma0_db, const void *wspd, const void *near, void *out_phi1, void *out_phi2,
                             void *out_sens1, void *out_sens2, void *out_phi_near, void *out_sens_near, void *out_phi_closest,
                             uint8_t *out_count, uint8_t *out_flag)
{
    if (!c) return XSW_EINVAL;
    const char *who = "dir_solve";
    if (int rc = check_raster_call(c, lines, samples, dtype, out_dtype, mem)) return rc;
    if (!inc || !sigma0_db || !wspd) return fail(c, XSW_EINVAL, "%s: an input raster is NULL", who);
    if (!out_phi1 && !out_phi2 && !out_sens1 && !out_sens2 && !out_phi_near && !out_sens_near && !out_phi_closest && !out_count && !out_flag)
        return fail(c, XSW_EINVAL, "%s: no output requested", who);
    if (!near && (out_phi_near || out_sens_near)) return fail(c, XSW_EINVAL, "%s: out_phi_near / out_sens_near need the reference direction `near`", who);
    if (!c->have_co) return fail(c, XSW_ENOLUT, "%s: no co-pol LUT installed", who);
    if (c->T.n_inc < 2 || c->T.n_w < 2 || c->T.n_phi < 2)  // (no cell to solve in)
        return fail(c, XSW_EINVAL, "%s: an axis of the co-pol LUT has fewer than two points", who);
    DirArgs A{};
    A.fold_phi = fold_phi != 0;
    size_t es, os;
    if (int rc = pixel_count(c, who, lines, samples, dtype, out_dtype, A.n, es, os)) return rc;
    if (A.n == 0) return XSW_OK;
    const size_t px = (size_t)A.n;
    Buf b[13] = {in_buf(inc, px * es), in_buf(sigma0_db, px * es), in_buf(wspd, px * es), in_buf(near, px * es),
                 out_buf(out_phi1, px * os), out_buf(out_phi2, px * os), out_buf(out_sens1, px * os), out_buf(out_sens2, px * os),
                 out_buf(out_phi_near, px * os), out_buf(out_sens_near, px * os), out_buf(out_phi_closest, px * os),
                 out_buf(out_count, px), out_buf(out_flag, px)};
    return run(c, mem, b, [&](Buf (&x)[13]) {
        A.inc = x[0].dev; A.s = x[1].dev; A.wspd = x[2].dev; A.near = x[3].dev;
        A.out_phi1 = x[4].dev; A.out_phi2 = x[5].dev; A.out_sens1 = x[6].dev; A.out_sens2 = x[7].dev;
        A.out_phi_near = x[8].dev; A.out_sens_near = x[9].dev; A.out_phi_closest = x[10].dev;
        A.out_count = x[11].dev; A.out_flag = x[12].dev;
        return queue(c, dtype, out_dtype, &PairLaunch::dir, A);
    }, who);
}

// ---- host-memory paths: chunks through a ring of workers (thread + stream + page-locked staging + device staging each)
static int host_thread_count(const xsw_ctx *c)
{
    int n = c->host_threads;
    if (n <= 0) {
        n = (int)env_int("XSW_HOST_THREADS", 12);  // read on every call
    }
    return std::max(1, std::min(n, 32));
}

static int worker_reserve(xsw_ctx::Worker &w, size_t pin_bytes, size_t dev_bytes, std::string &err)
{
    if (!w.s && hipStreamCreateWithFlags(&w.s, hipStreamNonBlocking) != hipSuccess) return seterr(err, XSW_EHIP, "stream create failed");
    if (pin_bytes > w.pin_cap && grow(w.pin, w.pin_cap, pin_bytes, nullptr, true) != hipSuccess) return seterr(err, XSW_ENOMEM, "hipHostMalloc(%zu) failed", pin_bytes);
    if (dev_bytes > w.dev_cap && grow(w.dev, w.dev_cap, dev_bytes) != hipSuccess) return seterr(err, XSW_ENOMEM, "hipMalloc(%zu) failed", dev_bytes);
    return XSW_OK;
}

// body(k, worker, err) -> XSW_* runs chunk k start to finish (stage, upload, launch, download, synchronise its stream, write the
// caller's output).  Chunks are dealt to min(threads, nchunks) workers; no exception crosses the ABI.
template <class Body>
static int run_chunks(xsw_ctx *c, long long nchunks, Body &&body)
{
    if (nchunks <= 0) return XSW_OK;
    const int nthreads = (int)std::min<long long>(host_thread_count(c), nchunks);
    if ((int)c->workers.size() < nthreads) c->workers.resize((size_t)nthreads);
    std::atomic<long long> next{0};
    std::atomic<int> rc{XSW_OK};
    std::mutex mu;
    std::string err;
    auto loop = [&](int wi) {
        std::string e;
        int r = hipSetDevice(c->device) == hipSuccess ? XSW_OK : seterr(e, XSW_EHIP, "hipSetDevice failed in a worker thread");
        while (!r && rc.load() == XSW_OK) {
            const long long k = next.fetch_add(1);
            if (k >= nchunks) break;
            r = body(k, c->workers[(size_t)wi], e);
        }
        if (r) {
            std::lock_guard<std::mutex> lk(mu);
            if (rc.load() == XSW_OK) { rc.store(r); err = e; }
        }
    };
    std::vector<std::thread> threads;
    int started = 0;
    if (nthreads > 1) {
        try {
            for (int t = 1; t < nthreads; ++t) { threads.emplace_back(loop, t); ++started; }
        } catch (...) { /* fewer threads than asked: the ones that started (and this one) take all the chunks */ }
    }
    loop(0);
    for (auto &t : threads) t.join();
    (void)started;
    if (rc.load() != XSW_OK) return fail(c, rc.load(), "%s", err.c_str());
    return XSW_OK;
}

// One raster of a chunk: host -> (page-locked staging ->) device, at offset `off` of the worker's two buffers.  The caller's
// staging callback may fill the staging area itself (numpy's own log10 on the bit-parity route); page-locked caller rasters
// (pinned_in) are read by the DMA engine directly.  A raster that is not given (h == nullptr) is nothing to do.
static int stage_upload(const xsw_invert_args *a, xsw_ctx::Worker &w, const ChunkPlan::Chunk &ch, bool pinned_in, int which,
                        const void *h, size_t off, size_t elem, std::string &err)
{
    if (!h) return XSW_OK;
    const char *src = (const char *)h + ch.px0 * elem;
    int staged = 0;
    if (a->stage) {
        staged = a->stage(a->stage_user, which, (int64_t)ch.px0, (int64_t)ch.npx, w.pin + off);
        if (staged < 0) return seterr(err, XSW_EINVAL, "the staging callback failed for raster %d, pixels [%zu, %zu)", which, ch.px0, ch.px0 + ch.npx);
    }
    if (staged > 0) src = w.pin + off;
    else if (!pinned_in) { memcpy(w.pin + off, src, ch.npx * elem); src = w.pin + off; }
    const hipError_t e = hipMemcpyAsync(w.dev + off, src, ch.npx * elem, hipMemcpyHostToDevice, w.s);
    return e == hipSuccess ? XSW_OK : seterr(err, XSW_EHIP, "H2D copy failed: %s", hipGetErrorString(e));
}

// A worker's own work lists for the chunks of `plan`, after `staged` bytes of its device buffer (dev == nullptr: the sizes only).
static WorkLists worker_lists(const ChunkPlan &plan, char *dev, size_t staged)
{
    return WorkLists{dev ? (unsigned *)(dev + staged) : nullptr, worker_list_cap(plan.max_px), strips_for((long long)plan.max_px, plan.lines_per_chunk)};
}

extern "C" int xsw_invert(xsw_ctx *c, const xsw_invert_args *a)
{
    if (!c || !a) return XSW_EINVAL;
    if (a->lines < 0 || a->samples < 0) return fail(c, XSW_EINVAL, "negative raster shape");
    if ((a->dtype != XSW_F32 && a->dtype != XSW_F64) || (a->out_dtype != XSW_F32 && a->out_dtype != XSW_F64))
        return fail(c, XSW_EINVAL, "dtype/out_dtype must be XSW_F32 or XSW_F64");
    if (a->mem != XSW_MEM_HOST && a->mem != XSW_MEM_DEVICE && a->mem != XSW_MEM_HOST_PINNED && a->mem != XSW_MEM_DEVICE_SIGMA0_HOST)
        return fail(c, XSW_EINVAL, "bad mem kind");
    if (!a->inc) return fail(c, XSW_EINVAL, "inc is NULL");
    if (!a->sigma0_co && !a->sigma0_cr) return fail(c, XSW_EINVAL, "neither sigma0_co nor sigma0_cr given");
    if (a->sigma0_co && !c->have_co) return fail(c, XSW_ENOLUT, "sigma0_co given but no co-pol LUT uploaded");
    if (a->sigma0_cr && !c->have_cr) return fail(c, XSW_ENOLUT, "sigma0_cr given but no cross-pol LUT uploaded");
    if (a->sigma0_co && !a->out_co && !a->out_code_co) return fail(c, XSW_EINVAL, "out_co is NULL");
    if (a->algo < XSW_ALGO_AUTO || a->algo > XSW_ALGO_EXHAUSTIVE_F64) return fail(c, XSW_EINVAL, "unknown algo %d", a->algo);
    const long long n = (long long)a->lines * a->samples;
    if (n == 0) return XSW_OK;
    HIPCHK(c, hipSetDevice(c->device));

    int algo = a->algo == XSW_ALGO_AUTO ? XSW_ALGO_PRUNED : a->algo;
    if ((algo == XSW_ALGO_EXHAUSTIVE || algo == XSW_ALGO_EXHAUSTIVE_F64) && !(a->sigma0_co && c->T.prunable && !a->sigma0_cr))
        return fail(c, XSW_EINVAL, "XSW_ALGO_EXHAUSTIVE handles mono co-pol on a uniform finite LUT only");

    KArgs A{};
    A.n = n;
    A.lines = a->lines;
    A.samples = a->samples;
    A.dsig_co = a->dsig_co;
    A.inv_dsig_co = 1.0 / a->dsig_co;
    A.dsig_cr_scalar = a->dsig_cr_scalar;
    A.is_db = a->sigma0_is_db;
    A.dual_select = a->dual_select;
    if (!(std::isfinite(A.inv_dsig_co) && A.inv_dsig_co != 0.0) && algo != XSW_ALGO_EXACT) algo = XSW_ALGO_EXACT;
    if (c->stats_on) {
        HIPCHK(c, hipMemsetAsync(c->d_stats, 0, 8 * sizeof(unsigned long long), c->stream));
        A.stats = c->d_stats;
        A.stats_chain = c->stats_chain ? 1 : 0;
    }

    const size_t es = a->dtype == XSW_F32 ? 4 : 8, os = a->out_dtype == XSW_F32 ? 8 : 16;
    const int dtype = a->dtype, out_dtype = a->out_dtype;
    if (a->mem == XSW_MEM_DEVICE || a->mem == XSW_MEM_DEVICE_SIGMA0_HOST) {  // the caller's device rasters
        A.inc = a->inc; A.dsig_cr = a->dsig_cr; A.anc = a->anc;
        A.out_co = a->out_co; A.out_cr = a->out_cr; A.out_idx = a->out_idx;
        A.code_co = a->out_code_co; A.code_cr = a->out_code_cr;
    }

    if (a->mem == XSW_MEM_DEVICE) {
        A.s_co = a->sigma0_co; A.s_cr = a->sigma0_cr;
        if (algo == XSW_ALGO_PRUNED) ensure_list(c, n, a->lines);
        std::string err;
        const LaunchCtl lc{c->stream, c->timing_on, c->lists};
        // one launch; a flat raster is re-cut as on the host path (ChunkPlan), which makes two: same stream, same work lists, in order
        const ChunkPlan plan(a->lines, a->samples, 0, 1, true);
        int rc = XSW_OK;
        for (long long k = 0; k < plan.nchunks && !rc; ++k) rc = dispatch_invert(c, slice(A, plan.chunk(k), es, os), dtype, out_dtype, algo, lc, err);
        return rc ? fail(c, rc, "%s", err.c_str()) : XSW_OK;
    }

    if (a->mem == XSW_MEM_DEVICE_SIGMA0_HOST) {
        // Device rasters, sigma0 from the host: row chunks (~4 Mpx) through the workers -- stage the chunk's sigma0 into the worker's
        // page-locked buffer (the caller's callback may fill it: numpy's own log10 on the bit-parity route), one upload per sigma0
        // raster, the kernels on the worker's stream with the caller's device pointers advanced to the chunk, results in place.
        if (a->out_idx || a->lines < 4) return fail(c, XSW_EINVAL, "XSW_MEM_DEVICE_SIGMA0_HOST: out_idx is not supported, and the raster needs 4 lines or more");
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the resident rasters' producers, and the statistics reset
        const ChunkPlan plan(a->lines, a->samples, 4LL << 20, 4, false);
        const ChunkStaging st(plan.max_px, es, false, a->sigma0_co, a->sigma0_cr, false, false, false, false);
        const size_t dev_bytes = st.o_end + worker_lists(plan, nullptr, 0).bytes();
        const int rc_all = run_chunks(c, plan.nchunks, [&](long long k, xsw_ctx::Worker &w, std::string &err) -> int {
            int rc = worker_reserve(w, st.o_end, dev_bytes, err);
            if (rc) return rc;
            const ChunkPlan::Chunk ch = plan.chunk(k);
            if ((rc = stage_upload(a, w, ch, false, 1, a->sigma0_co, st.o_co, es, err)) || (rc = stage_upload(a, w, ch, false, 2, a->sigma0_cr, st.o_cr, es, err))) return rc;
            KArgs B = slice(A, ch, es, os);
            B.s_co = a->sigma0_co ? w.dev + st.o_co : nullptr;
            B.s_cr = a->sigma0_cr ? w.dev + st.o_cr : nullptr;
            rc = dispatch_invert(c, B, dtype, out_dtype, algo, LaunchCtl{w.s, false, worker_lists(plan, w.dev, st.o_end)}, err);
            if (rc) return rc;
            const hipError_t e = hipStreamSynchronize(w.s);
            return e == hipSuccess ? XSW_OK : seterr(err, XSW_EHIP, "kernel execution failed: %s", hipGetErrorString(e));
        });
        trim_staging(c);
        return rc_all;
    }

    // Host rasters.  Chunks of whole 4-line tile rows (~2 Mpx; a flat raster re-cut, see ChunkPlan, so that the chunks pipeline)
    // go through the workers: stage the chunk's inputs into the worker's page-locked buffer (XSW_MEM_HOST_PINNED: skipped), ONE
    // upload, the kernels on the worker's stream, ONE download of the grid codes, then the codes are expanded into the caller's
    // rasters by the worker's thread while the other workers' chunks are in other phases.
    if (c->stats_on) HIPCHK(c, hipStreamSynchronize(c->stream));  // the counters were reset on the context's stream
    const bool pinned_in = a->mem == XSW_MEM_HOST_PINNED;
    const bool want_co = a->sigma0_co || a->out_co || a->out_code_co;
    const bool want_cr = a->out_cr || a->out_code_cr || (a->sigma0_cr && a->out_idx);
    const ChunkPlan plan(a->lines, a->samples, 2LL << 20, 4, true);
    const ChunkStaging st(plan.max_px, es, true, a->sigma0_co, a->sigma0_cr, a->dsig_cr, a->anc, want_co, want_cr);
    const size_t dev_bytes = st.o_end + worker_lists(plan, nullptr, 0).bytes();
    static const bool prof = env_flag("XSW_HOST_PROFILE");  // phase times of the pipeline on stderr (experiments)
    std::atomic<long long> t_stage{0}, t_gpu{0}, t_expand{0}, t_reserve{0};
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a0, std::chrono::steady_clock::time_point b0) {
        return (long long)std::chrono::duration_cast<std::chrono::microseconds>(b0 - a0).count(); };
    const auto t_begin = now();
    const int rc_all = run_chunks(c, plan.nchunks, [&](long long k, xsw_ctx::Worker &w, std::string &err) -> int {
        const auto t0 = now();
        int rc = worker_reserve(w, st.o_end, dev_bytes, err);
        if (rc) return rc;
        const auto t1 = now();
        const ChunkPlan::Chunk ch = plan.chunk(k);
        const size_t px0 = ch.px0, npx = ch.npx;
        auto up = [&](int which, const void *h, size_t off, size_t elem) { return stage_upload(a, w, ch, pinned_in, which, h, off, elem, err); };
        if ((rc = up(0, a->inc, st.o_inc, es)) || (rc = up(1, a->sigma0_co, st.o_co, es)) || (rc = up(2, a->sigma0_cr, st.o_cr, es)) ||
            (rc = up(3, a->dsig_cr, st.o_dsig, es)) || (rc = up(4, a->anc, st.o_anc, es * 2)))
            return rc;
        const auto t2 = now();
        KArgs B = slice(A, ch, es, os);  // (A holds no raster: the inputs are the worker's staging, the answer its grid codes)
        B.inc = w.dev + st.o_inc;
        B.s_co = a->sigma0_co ? w.dev + st.o_co : nullptr;
        B.s_cr = a->sigma0_cr ? w.dev + st.o_cr : nullptr;
        B.dsig_cr = a->dsig_cr ? w.dev + st.o_dsig : nullptr;
        B.anc = a->anc ? w.dev + st.o_anc : nullptr;
        B.code_co = want_co ? (unsigned *)(w.dev + st.o_cc) : nullptr;
        B.code_cr = want_cr ? (unsigned *)(w.dev + st.o_ccr) : nullptr;
        rc = dispatch_invert(c, B, dtype, out_dtype, algo, LaunchCtl{w.s, false, worker_lists(plan, w.dev, st.o_end)}, err);
        if (rc) return rc;
        hipError_t e = hipSuccess;
        if (st.o_end > st.o_cc) e = hipMemcpyAsync(w.pin + st.o_cc, w.dev + st.o_cc, st.o_end - st.o_cc, hipMemcpyDeviceToHost, w.s);
        if (e == hipSuccess) e = hipStreamSynchronize(w.s);
        if (e != hipSuccess) return seterr(err, XSW_EHIP, "kernel execution failed: %s", hipGetErrorString(e));
        const auto t3 = now();
        const uint32_t *cc = want_co ? (const uint32_t *)(w.pin + st.o_cc) : nullptr, *ccr = want_cr ? (const uint32_t *)(w.pin + st.o_ccr) : nullptr;
        if (a->out_code_co && cc) memcpy(a->out_code_co + px0, cc, npx * 4);
        if (a->out_code_cr && ccr) memcpy(a->out_code_cr + px0, ccr, npx * 4);
        int32_t *idx = a->out_idx ? a->out_idx + 3 * px0 : nullptr;
        if (a->out_co || a->out_cr || idx) {
            if (out_dtype == XSW_F32)
                expand_host<float>(c, npx, cc, ccr, a->out_co ? (float *)a->out_co + 2 * px0 : nullptr, a->out_cr ? (float *)a->out_cr + 2 * px0 : nullptr, idx);
            else
                expand_host<double>(c, npx, cc, ccr, a->out_co ? (double *)a->out_co + 2 * px0 : nullptr, a->out_cr ? (double *)a->out_cr + 2 * px0 : nullptr, idx);
        }
        if (prof) { const auto t4 = now(); t_reserve += us(t0, t1); t_stage += us(t1, t2); t_gpu += us(t2, t3); t_expand += us(t3, t4); }
        return XSW_OK;
    });
    trim_staging(c);
    if (prof)
        fprintf(stderr, "[xsw host] %lld px, %lld chunks, %d threads: wall %.2f ms; summed over workers: reserve %.2f, stage %.2f, upload+kernels+download %.2f, expand %.2f ms\n",
                n, plan.nchunks, (int)std::min<long long>(host_thread_count(c), plan.nchunks), us(t_begin, now()) / 1e3, t_reserve / 1e3, t_stage / 1e3, t_gpu / 1e3, t_expand / 1e3);
    return rc_all;
}

// ---------------------------------------------------------------------------------------- LUT interpolation
// what a failed temporary is to the caller of the interpolation or the build; `nomem` may name the bytes asked for (%zu)
static int temps_rc(xsw_ctx *c, const CallTemps &tmp, const char *nomem, const char *h2d)
{
    return tmp.ok() ? XSW_OK : tmp.refused ? fail(c, XSW_ENOMEM, nomem, tmp.refused - 8) : fail(c, XSW_EHIP, "%s", h2d);
}

// Interpolation with device-resident raw table and output (d_raw -> d_out); axes are host arrays.  Asynchronous on the
// context's stream except for the small uploads; the temporaries are `tmp`'s (the caller's: freed when its call ends).
static int interp_device(xsw_ctx *c, const double *d_raw, const double *inc_raw, const double *wspd_raw, const double *phi_raw,
                         int32_t n_inc_raw, int32_t n_wspd_raw, int32_t n_phi_raw, const double *inc, const double *wspd,
                         const double *phi, int32_t n_inc, int32_t n_wspd, int32_t n_phi, double *d_out, CallTemps &tmp)
{
    if (!inc_raw || !wspd_raw || !inc || !wspd || n_inc_raw < 2 || n_wspd_raw < 2 || n_inc < 1 || n_wspd < 1)
        return fail(c, XSW_EINVAL, "lut_interp: null pointer or axis shorter than 2");
    const bool has_phi = n_phi_raw > 0;
    if (has_phi && (!phi_raw || !phi || n_phi_raw < 2 || n_phi < 1)) return fail(c, XSW_EINVAL, "lut_interp: bad phi axis");
    if (!strictly_ascending(inc_raw, n_inc_raw) || !strictly_ascending(wspd_raw, n_wspd_raw) ||
        (has_phi && !strictly_ascending(phi_raw, n_phi_raw)))
        return fail(c, XSW_EINVAL, "lut_interp: raw axes must be strictly ascending");
    std::vector<int> loi, low, lop;
    if (!left_neighbours(inc_raw, n_inc_raw, inc, n_inc, loi) || !left_neighbours(wspd_raw, n_wspd_raw, wspd, n_wspd, low) ||
        (has_phi && !left_neighbours(phi_raw, n_phi_raw, phi, n_phi, lop)))
        return fail(c, XSW_EINVAL, "A value in x_new is outside the interpolation range.");
    InterpArgs a{};
    a.raw = d_raw;
    a.xi_raw = (const double *)tmp.alloc((size_t)n_inc_raw * 8, inc_raw);
    a.xw_raw = (const double *)tmp.alloc((size_t)n_wspd_raw * 8, wspd_raw);
    a.xi = (const double *)tmp.alloc((size_t)n_inc * 8, inc);
    a.xw = (const double *)tmp.alloc((size_t)n_wspd * 8, wspd);
    a.loi = (const int *)tmp.alloc(loi.size() * 4, loi.data());
    a.low = (const int *)tmp.alloc(low.size() * 4, low.data());
    if (has_phi) {
        a.xp_raw = (const double *)tmp.alloc((size_t)n_phi_raw * 8, phi_raw);
        a.xp = (const double *)tmp.alloc((size_t)n_phi * 8, phi);
        a.lop = (const int *)tmp.alloc(lop.size() * 4, lop.data());
    }
    int rc = temps_rc(c, tmp, "lut_interp: hipMalloc failed", "lut_interp: H2D failed");
    a.out = d_out;
    a.ni_raw = n_inc_raw; a.nw_raw = n_wspd_raw; a.np_raw = has_phi ? n_phi_raw : 0;
    a.ni = n_inc; a.nw = n_wspd; a.np = has_phi ? n_phi : 0;
    if (!rc) {
        const size_t n_out = (size_t)n_inc * n_wspd * (has_phi ? n_phi : 1);
        long long blocks = (long long)((n_out + 255) / 256);
        if (blocks > 256 * 16) blocks = 256 * 16;
        hipLaunchKernelGGL(k_lut_interp, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
        if (hipGetLastError() != hipSuccess) rc = fail(c, XSW_EHIP, "lut_interp: launch failed");
    }
    // the copies above are queued on the launch stream, in order with k_lut_interp; loi / low / lop are locals of this function
    hipError_t se = hipStreamSynchronize(c->stream);
    if (!rc && se != hipSuccess) rc = fail(c, XSW_EHIP, "lut_interp: %s", hipGetErrorString(se));
    return rc;
}

extern "C" int xsw_lut_interp(xsw_ctx *c, const double *raw, const double *inc_raw, const double *wspd_raw,
                              const double *phi_raw, int32_t n_inc_raw, int32_t n_wspd_raw, int32_t n_phi_raw,
                              const double *inc, const double *wspd, const double *phi, int32_t n_inc, int32_t n_wspd,
                              int32_t n_phi, double *out)
{
    if (!c) return XSW_EINVAL;
    if (!raw || !out) return fail(c, XSW_EINVAL, "lut_interp: null pointer or axis shorter than 2");
    HIPCHK(c, hipSetDevice(c->device));
    const bool has_phi = n_phi_raw > 0;
    CallTemps tmp(c->stream);
    const size_t n_raw = (size_t)std::max(n_inc_raw, 0) * std::max(n_wspd_raw, 0) * (has_phi ? n_phi_raw : 1);
    const size_t n_out = (size_t)std::max(n_inc, 0) * std::max(n_wspd, 0) * (has_phi ? std::max(n_phi, 0) : 1);
    const void *d_raw = tmp.alloc(n_raw * 8, raw, 8);
    void *d_out = tmp.alloc(n_out * 8, nullptr, 8);
    int rc = temps_rc(c, tmp, "lut_interp: hipMalloc failed", "lut_interp: H2D failed");
    if (!rc) rc = interp_device(c, (const double *)d_raw, inc_raw, wspd_raw, phi_raw, n_inc_raw, n_wspd_raw, n_phi_raw, inc, wspd, phi,
                                n_inc, n_wspd, n_phi, (double *)d_out, tmp);
    if (!rc && hipMemcpyAsync(out, d_out, n_out * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(c, XSW_EHIP, "lut_interp: D2H failed");
    const hipError_t se = tmp.finish();
    if (!rc && se != hipSuccess) rc = fail(c, XSW_EHIP, "lut_interp: %s", hipGetErrorString(se));
    return rc;
}

// ---------------------------------------------------------------------------------------- device-side LUT build
extern "C" int xsw_lut_build(xsw_ctx *c, int32_t gmf_id, const double *inc_raw, int32_t n_inc_raw, const double *wspd_raw,
                             int32_t n_wspd_raw, const double *phi_raw, int32_t n_phi_raw, const xsw_lut *target)
{
    if (!c) return XSW_EINVAL;
    if (gmf_id < 0 || gmf_id >= GMF_COUNT) return fail(c, XSW_EINVAL, "unknown gmf_id %d", gmf_id);
    if (!target || !inc_raw || !wspd_raw || !target->inc || !target->wspd || n_inc_raw < 1 || n_wspd_raw < 1 ||
        target->n_inc < 1 || target->n_wspd < 1)
        return fail(c, XSW_EINVAL, "lut_build: null pointer or empty axis");
    const bool copol = gmf_id <= GMF_CMODIFR2;
    if (copol != (n_phi_raw > 0) || copol != (target->n_phi > 0) || (copol && (!phi_raw || !target->phi)))
        return fail(c, XSW_EINVAL, "lut_build: a co-pol GMF needs phi axes, a cross-pol GMF must not have them");
    HIPCHK(c, hipSetDevice(c->device));
    const int npr = copol ? n_phi_raw : 1, npt = copol ? target->n_phi : 1;
    const size_t n_raw = (size_t)n_inc_raw * n_wspd_raw * npr, n_out = (size_t)target->n_inc * target->n_wspd * npt;
    // the uploads are queued on the launch stream, in order with the kernels that read them (synchronised before this function returns)
    CallTemps tmp(c->stream);
    const double *d_i = (const double *)tmp.alloc((size_t)n_inc_raw * 8, inc_raw, 8), *d_w = (const double *)tmp.alloc((size_t)n_wspd_raw * 8, wspd_raw, 8);
    const double *d_p = copol ? (const double *)tmp.alloc((size_t)n_phi_raw * 8, phi_raw, 8) : nullptr;
    double *d_raw = (double *)tmp.alloc(n_raw * 8, nullptr, 8);
    int rc = temps_rc(c, tmp, "lut_build: hipMalloc(%zu) failed", "lut_build: H2D failed");
    if (!rc) {
        XSW_GMF_DISPATCH(gmf_id, hipLaunchKernelGGL((k_gmf_grid<M>), dim3((unsigned)std::min<size_t>((n_raw + 255) / 256, 256 * 16)), dim3(256), 0, c->stream,
                                                    (int)gmf_id, d_i, d_w, d_p, n_inc_raw, n_wspd_raw, copol ? n_phi_raw : 0, d_raw));
        if (hipGetLastError() != hipSuccess) rc = fail(c, XSW_EHIP, "lut_build: launch failed");
    }
    // resolution change only when the grids differ (Model._normalize_lut returns the raw LUT as is otherwise)
    const bool same = same_axis(inc_raw, n_inc_raw, target->inc, target->n_inc) && same_axis(wspd_raw, n_wspd_raw, target->wspd, target->n_wspd) &&
                      (!copol || same_axis(phi_raw, n_phi_raw, target->phi, target->n_phi));
    double *d_dense = d_raw;
    if (!rc && !same) {
        d_dense = (double *)tmp.alloc(n_out * 8, nullptr, 8);
        if (!(rc = temps_rc(c, tmp, "lut_build: hipMalloc(%zu) failed", "lut_build: H2D failed"))) rc = interp_device(c, d_raw, inc_raw, wspd_raw, phi_raw, n_inc_raw, n_wspd_raw, copol ? n_phi_raw : 0, target->inc,
                                    target->wspd, target->phi, target->n_inc, target->n_wspd, copol ? target->n_phi : 0, d_dense, tmp);
    }
    if (!rc) {
        hipLaunchKernelGGL(k_to_db, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 256 * 16)), dim3(256), 0, c->stream, d_dense, (long long)n_out);
        if (hipGetLastError() != hipSuccess) rc = fail(c, XSW_EHIP, "lut_build: launch failed");
    }
    if (!rc && copol) rc = install_co(c, target, d_dense);
    if (!rc && !copol) {  // cross-pol tables are small (a few MB): the host-side checks of upload_cr are reused
        std::vector<double> h(n_out);
        hipError_t e = hipMemcpyAsync(h.data(), d_dense, n_out * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, XSW_EHIP, "lut_build: D2H failed: %s", hipGetErrorString(e));
        if (!rc) {
            xsw_lut t = *target;
            t.db = h.data();
            rc = upload_cr(c, &t);
        }
    }
    const hipError_t se = tmp.finish();
    if (!rc && se != hipSuccess) rc = fail(c, XSW_EHIP, "lut_build: %s", hipGetErrorString(se));
    return rc;
}

// ---------------------------------------------------------------------------------------- forward GMF
extern "C" int xsw_gmf_eval(xsw_ctx *c, int32_t gmf_id, int64_t n, int32_t mem, const double *inc, const double *wspd,
                            const double *phi, double *out)
{
    if (!c) return XSW_EINVAL;
    if (gmf_id < 0 || gmf_id >= GMF_COUNT) return fail(c, XSW_EINVAL, "unknown gmf_id %d", gmf_id);
    if (n < 0 || !inc || !wspd || !out) return fail(c, XSW_EINVAL, "gmf_eval: bad argument");
    if (gmf_id <= GMF_CMODIFR2 && !phi) return fail(c, XSW_EINVAL, "gmf_eval: this GMF needs phi");
    if (n == 0) return XSW_OK;
    const size_t bytes = (size_t)n * 8;
    Buf b[4] = {in_buf(inc, bytes), in_buf(wspd, bytes), in_buf(phi, bytes), out_buf(out, bytes)};
    return run(c, mem, b, [&](Buf (&x)[4]) {
        const long long blocks = std::min<long long>((n + 255) / 256, 256 * 16);
        XSW_GMF_DISPATCH(gmf_id, hipLaunchKernelGGL((k_gmf_eval<M>), dim3((unsigned)blocks), dim3(256), 0, c->stream, (int)gmf_id, (long long)n,
                                                    (const double *)x[0].dev, (const double *)x[1].dev, (const double *)x[2].dev, (double *)x[3].dev));
    }, "gmf_eval");
}

// ---------------------------------------------------------------------------------------- detrend
template <typename T, typename TO>
static void launch_detrend(hipStream_t s, const void *in, const double *ratio, const double *rinv, bool fast, void *out,
                           long long lines, long long samples)
{
#ifndef XSW_DETREND_WG_PER_CU
#define XSW_DETREND_WG_PER_CU 16
#endif
    const Strips g = strip_grid(lines, (samples + 3) / 4, XSW_DETREND_WG_PER_CU);  // columns: quads of samples
    const dim3 grid((unsigned)g.gx, (unsigned)g.gy);
    const long long lpb = g.rows_per_block;
    if (fast)
        hipLaunchKernelGGL((k_detrend<T, TO, 1>), grid, dim3(256), 0, s, (const T *)in, ratio, rinv, (TO *)out, lines, samples, lpb);
    else
        hipLaunchKernelGGL((k_detrend<T, TO, 0>), grid, dim3(256), 0, s, (const T *)in, ratio, rinv, (TO *)out, lines, samples, lpb);
}

extern "C" int xsw_detrend(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                           const void *sigma0, const double *ratio_row, void *out)
{
    if (!c) return XSW_EINVAL;
    if (lines < 0 || samples < 0 || !sigma0 || !ratio_row || !out) return fail(c, XSW_EINVAL, "bad detrend argument");
    const long long n = (long long)lines * samples;
    if (n == 0) return XSW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t es = dtype == XSW_F32 ? 4 : 8, os = out_dtype == XSW_F32 ? 4 : 8;
    // the ratio row lives in a context-owned buffer (grown on demand): no allocation on the steady-state path
    const size_t row_bytes = 2 * (size_t)samples * sizeof(double) + 64;
    if (row_bytes > c->ratio_cap)  // (synchronised first: a previous asynchronous call may still read the old row)
        HIPCHK(c, grow(c->d_ratio, c->ratio_cap, row_bytes, &c->stream));
    std::vector<double> both;
    const bool fast = detrend_row(ratio_row, (size_t)samples, both);
    double *d_rinv = c->d_ratio + samples;
    hipError_t e = hipMemcpyAsync(c->d_ratio, both.data(), 2 * (size_t)samples * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // `both` is a local
    auto launch = [&](const void *din, void *dout, long long nl, hipStream_t st) {
        if (dtype == XSW_F32 && out_dtype == XSW_F32) launch_detrend<float, float>(st, din, c->d_ratio, d_rinv, fast, dout, nl, samples);
        else if (dtype == XSW_F32) launch_detrend<float, double>(st, din, c->d_ratio, d_rinv, fast, dout, nl, samples);
        else if (out_dtype == XSW_F32) launch_detrend<double, float>(st, din, c->d_ratio, d_rinv, fast, dout, nl, samples);
        else launch_detrend<double, double>(st, din, c->d_ratio, d_rinv, fast, dout, nl, samples);
        return hipGetLastError();
    };
    if (mem == XSW_MEM_DEVICE) {  // device rasters: asynchronous on the context's stream
        if (e == hipSuccess) e = launch(sigma0, out, lines, c->stream);
        if (e != hipSuccess) return fail(c, XSW_EHIP, "detrend failed: %s", hipGetErrorString(e));
        return XSW_OK;
    }
    // Host rasters (synchronous): line chunks through the workers of the host-memory path (page-locked staging, one stream per
    // worker: staging copies, uploads, kernels and downloads of different chunks overlap).
    if (e != hipSuccess) return fail(c, XSW_EHIP, "detrend failed: %s", hipGetErrorString(e));
    const bool pinned = mem == XSW_MEM_HOST_PINNED;
    const ChunkPlan plan(lines, samples, 4LL << 20, 1, false);  // ~4 Mpx of whole lines
    const size_t o_out = pad256(plan.max_px * es), total = o_out + plan.max_px * os;
    const int rc_det = run_chunks(c, plan.nchunks, [&](long long k, xsw_ctx::Worker &w, std::string &err) -> int {
        int rc = worker_reserve(w, pinned ? 0 : total, total, err);
        if (rc) return rc;
        const ChunkPlan::Chunk ch = plan.chunk(k);
        const size_t px0 = ch.px0, npx = ch.npx;
        const char *src = (const char *)sigma0 + px0 * es;
        char *dst = (char *)out + px0 * os;
        hipError_t ee;
        if (pinned) ee = hipMemcpyAsync(w.dev, src, npx * es, hipMemcpyHostToDevice, w.s);
        else { memcpy(w.pin, src, npx * es); ee = hipMemcpyAsync(w.dev, w.pin, npx * es, hipMemcpyHostToDevice, w.s); }
        if (ee == hipSuccess) ee = launch(w.dev, w.dev + o_out, ch.lines, w.s);
        if (ee == hipSuccess) ee = hipMemcpyAsync(pinned ? dst : w.pin + o_out, w.dev + o_out, npx * os, hipMemcpyDeviceToHost, w.s);
        if (ee == hipSuccess) ee = hipStreamSynchronize(w.s);
        if (ee != hipSuccess) return seterr(err, XSW_EHIP, "detrend failed: %s", hipGetErrorString(ee));
        if (!pinned) memcpy(dst, w.pin + o_out, npx * os);
        return XSW_OK;
    });
    trim_staging(c);
    return rc_det;
}

// ---------------------------------------------------------------------------------------- cross-pol noise flattening
// The context scratch of one raster: [column partials | noise_mean, inc_row | x0 (+ pad) | fit[lines][2]] (nesz_blocks sizes it)
struct NeszScratch {
    NeszPartial *part;
    double *col, *x0, *fit;
    NeszScratch(void *scratch, long long samples, int nb)
        : part((NeszPartial *)scratch), col((double *)((char *)scratch + (size_t)nb * samples * sizeof(NeszPartial))),
          x0(col + 2 * samples), fit(x0 + 8) {}
};

// The fit half, shared by xsw_nesz_flatten and xsw_dsig_flat: column means, centring abscissa, (slope, icpt) of every line
template <typename T>
static void launch_nesz_fit(hipStream_t s, const void *noise, const void *inc, const NeszScratch &k, long long lines, long long samples,
                            int nb, long long lpb)
{
    const unsigned gx = (unsigned)((samples + 255) / 256);
    hipLaunchKernelGGL((k_nesz_colsum<T, 1>), dim3(gx, (unsigned)nb), dim3(256), 0, s, (const T *)noise, (const T *)inc, k.part, lines, samples, lpb);
    hipLaunchKernelGGL(k_nesz_colmean, dim3(gx), dim3(256), 0, s, k.part, k.col, samples, nb);
    hipLaunchKernelGGL(k_nesz_center, dim3(1), dim3(1024), 0, s, k.col, k.x0, samples);
    hipLaunchKernelGGL((k_nesz_fit<T>), dim3((unsigned)((lines + XSW_NESZ_LINES - 1) / XSW_NESZ_LINES)), dim3(XSW_NESZ_THREADS), 0, s, (const T *)noise, k.col,
                       k.x0, k.fit, lines, samples);
}

// The grid of the passes that evaluate the fit (k_nesz_eval, k_dsig_flat): column groups x line blocks, ~16 workgroups per CU
static Strips nesz_eval_grid(long long lines, long long samples)
{
    return strip_grid(lines, (samples + XSW_NESZ_EV - 1) / XSW_NESZ_EV);  // columns: groups of XSW_NESZ_EV samples
}

template <typename T>
static hipError_t launch_nesz(hipStream_t s, const void *noise, const void *inc, void *scratch, double *out, long long lines,
                              long long samples, int nb, long long lpb)
{
    const NeszScratch k(scratch, samples, nb);
    launch_nesz_fit<T>(s, noise, inc, k, lines, samples, nb, lpb);
    const Strips e = nesz_eval_grid(lines, samples);  // the write pass
    hipLaunchKernelGGL((k_nesz_eval<sizeof(T) == 4>), dim3((unsigned)e.gx, (unsigned)e.gy), dim3(256), 0, s, k.col, k.fit, out, lines, samples, e.rows_per_block);
    return hipGetLastError();
}

// Moves `bytes` between a host buffer and the device through the workers' page-locked staging (32 MB pieces, side by side).
static int move_through_workers(xsw_ctx *c, void *host, void *dev, size_t bytes, bool to_device, bool pinned)
{
    const size_t piece = (size_t)32 << 20;
    const long long np = (long long)((bytes + piece - 1) / piece);
    return run_chunks(c, np, [&](long long k, xsw_ctx::Worker &w, std::string &err) -> int {
        int rc = worker_reserve(w, pinned ? 0 : piece, 0, err);
        if (rc) return rc;
        const size_t off = (size_t)k * piece, nb = std::min(piece, bytes - off);
        char *h = (char *)host + off, *d = (char *)dev + off;
        hipError_t e;
        if (to_device) {
            if (pinned) e = hipMemcpyAsync(d, h, nb, hipMemcpyHostToDevice, w.s);
            else { memcpy(w.pin, h, nb); e = hipMemcpyAsync(d, w.pin, nb, hipMemcpyHostToDevice, w.s); }
            if (e == hipSuccess) e = hipStreamSynchronize(w.s);
        } else {
            e = hipMemcpyAsync(pinned ? h : w.pin, d, nb, hipMemcpyDeviceToHost, w.s);
            if (e == hipSuccess) e = hipStreamSynchronize(w.s);
            if (e == hipSuccess && !pinned) memcpy(h, w.pin, nb);
        }
        return e == hipSuccess ? XSW_OK : seterr(err, XSW_EHIP, "staged copy failed: %s", hipGetErrorString(e));
    });
}

extern "C" int xsw_nesz_flatten(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *noise,
                                const void *inc, double *out)
{
    if (!c) return XSW_EINVAL;
    if (lines < 0 || samples < 0 || !noise || !inc || !out) return fail(c, XSW_EINVAL, "bad nesz_flatten argument");
    if (dtype != XSW_F32 && dtype != XSW_F64) return fail(c, XSW_EINVAL, "dtype must be XSW_F32 or XSW_F64");
    if (mem != XSW_MEM_HOST && mem != XSW_MEM_DEVICE && mem != XSW_MEM_HOST_PINNED) return fail(c, XSW_EINVAL, "bad mem kind");
    if (lines > 0x7fffffffLL) return fail(c, XSW_EINVAL, "raster too large for one launch");
    const long long n = (long long)lines * samples;
    if (n == 0) return XSW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t es = dtype == XSW_F32 ? 4 : 8;
    const NeszBlocks nbk = nesz_blocks(lines, samples, sizeof(NeszPartial));
    // context-owned scratch (column partials, means, centring abscissa), grown on demand: no allocation on the steady-state path
    if (nbk.scratch_bytes > c->nesz_cap)  // (synchronised first: a previous call may still be using the old scratch)
        HIPCHK(c, grow(c->nesz_scratch, c->nesz_cap, nbk.scratch_bytes, &c->stream));
    auto launch = [&](const void *dn, const void *di, double *dout) {
        return dtype == XSW_F32 ? launch_nesz<float>(c->stream, dn, di, c->nesz_scratch, dout, lines, samples, (int)nbk.nb, nbk.lpb)
                                : launch_nesz<double>(c->stream, dn, di, c->nesz_scratch, dout, lines, samples, (int)nbk.nb, nbk.lpb);
    };
    if (mem == XSW_MEM_DEVICE) {  // asynchronous on the context's stream, like xsw_invert / xsw_detrend
        const hipError_t e = launch(noise, inc, out);
        if (e != hipSuccess) return fail(c, XSW_EHIP, "nesz_flatten failed: %s", hipGetErrorString(e));
        return XSW_OK;
    }
    // host rasters: the column means need the whole raster before the per-line pass, so the rasters are uploaded whole (through
    // the workers' page-locked staging), the four kernels run, and the result comes back the same way
    const size_t in_b = ((size_t)n * es + 255) & ~(size_t)255, need = 2 * in_b + (size_t)n * 8;
    if (need > c->arena_cap && grow(c->arena, c->arena_cap, need) != hipSuccess) return fail(c, XSW_ENOMEM, "hipMalloc(%zu) failed", need);
    const bool pinned = mem == XSW_MEM_HOST_PINNED;
    char *d_noise = c->arena, *d_inc = c->arena + in_b;
    double *d_out = (double *)(c->arena + 2 * in_b);
    int rc = move_through_workers(c, (void *)noise, d_noise, (size_t)n * es, true, pinned);
    if (!rc) rc = move_through_workers(c, (void *)inc, d_inc, (size_t)n * es, true, pinned);
    if (!rc) {
        hipError_t e = launch(d_noise, d_inc, d_out);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, XSW_EHIP, "nesz_flatten failed: %s", hipGetErrorString(e));
    }
    if (!rc) rc = move_through_workers(c, out, d_out, (size_t)n * 8, false, pinned);
    trim_staging(c);
    if (c->arena_cap > XSW_ARENA_KEEP) (void)grow(c->arena, c->arena_cap, 0);  // do not sit on a huge staging area
    return rc;
}

// ---------------------------------------------------------------------------------------- dsig_cr
#define XSW_DSIG_RULES(rule, CALL)                                       \
    do {                                                                 \
        if ((rule) == XSW_DSIG_S1_V2) { CALL(XSW_DSIG_S1_V2); }          \
        else if ((rule) == XSW_DSIG_RS2_V2) { CALL(XSW_DSIG_RS2_V2); }   \
        else { CALL(XSW_DSIG_CMODMS1AHW); }                              \
    } while (0)

template <typename T, typename TN>
static void launch_dsig(hipStream_t s, int rule, const void *inc, const void *sigma0, const void *nesz, void *out, long long n)
{
    const unsigned blocks = (unsigned)((n + 256LL * XSW_DSIG_V - 1) / (256LL * XSW_DSIG_V));
#define XSW_CALL(R) hipLaunchKernelGGL((k_dsig<T, TN, R>), dim3(blocks), dim3(256), 0, s, (const T *)sigma0, (const TN *)nesz, (const T *)inc, \
                                       (typename DsigOut<T, TN, R>::type *)out, n)
    XSW_DSIG_RULES(rule, XSW_CALL);
#undef XSW_CALL
}

static bool dsig_dtype_ok(int32_t dt) { return dt == XSW_F32 || dt == XSW_F64; }
static bool dsig_rule_ok(int32_t rule) { return rule >= XSW_DSIG_S1_V2 && rule <= XSW_DSIG_CMODMS1AHW; }

extern "C" int xsw_dsig(xsw_ctx *c, int32_t rule, int64_t lines, int64_t samples, int32_t dtype, int32_t nesz_dtype, int32_t mem,
                        const void *inc, const void *sigma0_cr, const void *nesz_cr, void *out)
{
    if (!c) return XSW_EINVAL;
    if (!dsig_rule_ok(rule)) return fail(c, XSW_EINVAL, "dsig: unknown rule %d", (int)rule);
    if (!dsig_dtype_ok(dtype) || !dsig_dtype_ok(nesz_dtype)) return fail(c, XSW_EINVAL, "dsig: dtype must be XSW_F32 or XSW_F64");
    if (mem != XSW_MEM_HOST && mem != XSW_MEM_DEVICE) return fail(c, XSW_EINVAL, "dsig: bad mem kind");
    if (lines < 0 || samples < 0 || !sigma0_cr || !nesz_cr || !out) return fail(c, XSW_EINVAL, "dsig: bad argument");
    if (rule == XSW_DSIG_S1_V2 && !inc) return fail(c, XSW_EINVAL, "dsig: XSW_DSIG_S1_V2 needs inc");
    if (samples && lines > (int64_t)(0x7fffffffLL * 256 * XSW_DSIG_V) / samples) return fail(c, XSW_EINVAL, "raster too large for one launch");
    const long long n = (long long)lines * samples;
    if (n == 0) return XSW_OK;
    const size_t es = dtype == XSW_F32 ? 4 : 8, ns = nesz_dtype == XSW_F32 ? 4 : 8;
    const size_t os = (rule != XSW_DSIG_S1_V2 && es == 4 && ns == 4) ? 4 : 8;
    Buf b[4] = {in_buf(rule == XSW_DSIG_S1_V2 ? inc : nullptr, (size_t)n * es), in_buf(sigma0_cr, (size_t)n * es), in_buf(nesz_cr, (size_t)n * ns),
                out_buf(out, (size_t)n * os)};
    return run(c, mem, b, [&](Buf (&x)[4]) {
        if (es == 4 && ns == 4) launch_dsig<float, float>(c->stream, rule, x[0].dev, x[1].dev, x[2].dev, x[3].dev, n);
        else if (es == 4) launch_dsig<float, double>(c->stream, rule, x[0].dev, x[1].dev, x[2].dev, x[3].dev, n);
        else if (ns == 4) launch_dsig<double, float>(c->stream, rule, x[0].dev, x[1].dev, x[2].dev, x[3].dev, n);
        else launch_dsig<double, double>(c->stream, rule, x[0].dev, x[1].dev, x[2].dev, x[3].dev, n);
    }, "dsig");
}

template <typename T, typename TO>
static void launch_dsig_flat(hipStream_t s, int rule, const void *noise, const void *inc, const void *sigma0, void *scratch, void *out,
                                   long long lines, long long samples, int nb, long long lpb)
{
    const NeszScratch k(scratch, samples, nb);
    launch_nesz_fit<T>(s, noise, inc, k, lines, samples, nb, lpb);
    const Strips e = nesz_eval_grid(lines, samples);
#define XSW_CALL(R) hipLaunchKernelGGL((k_dsig_flat<T, TO, R>), dim3((unsigned)e.gx, (unsigned)e.gy), dim3(256), 0, s, k.col, k.fit, (const T *)sigma0, \
                                       (const T *)inc, (TO *)out, lines, samples, e.rows_per_block)
    XSW_DSIG_RULES(rule, XSW_CALL);
#undef XSW_CALL
}

extern "C" int xsw_dsig_flat(xsw_ctx *c, int32_t rule, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                             const void *noise, const void *inc, const void *sigma0_cr, void *out)
{
    if (!c) return XSW_EINVAL;
    if (!dsig_rule_ok(rule)) return fail(c, XSW_EINVAL, "dsig_flat: unknown rule %d", (int)rule);
    if (!dsig_dtype_ok(dtype) || !dsig_dtype_ok(out_dtype)) return fail(c, XSW_EINVAL, "dsig_flat: dtype must be XSW_F32 or XSW_F64");
    if (mem != XSW_MEM_HOST && mem != XSW_MEM_DEVICE) return fail(c, XSW_EINVAL, "dsig_flat: bad mem kind");
    if (lines < 0 || samples < 0 || !noise || !inc || !sigma0_cr || !out) return fail(c, XSW_EINVAL, "dsig_flat: bad argument");
    if (lines > 0x7fffffffLL) return fail(c, XSW_EINVAL, "raster too large for one launch");
    const long long n = (long long)lines * samples;
    if (n == 0) return XSW_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t es = dtype == XSW_F32 ? 4 : 8, os = out_dtype == XSW_F32 ? 4 : 8;
    const NeszBlocks nbk = nesz_blocks(lines, samples, sizeof(NeszPartial));
    if (nbk.scratch_bytes > c->nesz_cap)  // (synchronised first: a previous call may still be using the old scratch)
        HIPCHK(c, grow(c->nesz_scratch, c->nesz_cap, nbk.scratch_bytes, &c->stream));
    Buf b[4] = {in_buf(noise, (size_t)n * es), in_buf(inc, (size_t)n * es), in_buf(sigma0_cr, (size_t)n * es), out_buf(out, (size_t)n * os)};
    return run(c, mem, b, [&](Buf (&x)[4]) {
#define XSW_CALL(T, TO) launch_dsig_flat<T, TO>(c->stream, rule, x[0].dev, x[1].dev, x[2].dev, c->nesz_scratch, x[3].dev, lines, samples, (int)nbk.nb, nbk.lpb)
        if (es == 4 && os == 4) XSW_CALL(float, float);
        else if (es == 4) XSW_CALL(float, double);
        else if (os == 4) XSW_CALL(double, float);
        else XSW_CALL(double, double);
#undef XSW_CALL
    }, "dsig_flat");
}

extern "C" int xsw_dsig_wspd(xsw_ctx *c, int32_t rule, int64_t n, int32_t mem, const double *U, const double *snr, double *out)
{
    // (b, c0, gamma, k) of windspeed/utils.py:27-42
    static const DsigWspdCoef coef[3] = {
        {-0.4908643753212401, 16.763199934792965, 1.3891445172991084, 20.616914824394343},
        {-0.5858970325653666, 16.50039320910609, 1.1032031322520397, 7.434663633997121},
        {-0.7920301376936547, 15.8288289109038, 0.24040294696606557, 0.2538177092195224},
    };
    if (!c) return XSW_EINVAL;
    if (rule < XSW_DSIG_WSPD_RS2_V3 || rule > XSW_DSIG_WSPD_RCM_V3) return fail(c, XSW_EINVAL, "dsig_wspd: unknown rule %d", (int)rule);
    if (mem != XSW_MEM_HOST && mem != XSW_MEM_DEVICE) return fail(c, XSW_EINVAL, "dsig_wspd: bad mem kind");
    if (n < 0 || !U || !snr || !out) return fail(c, XSW_EINVAL, "dsig_wspd: bad argument");
    if (n == 0) return XSW_OK;
    const size_t bytes = (size_t)n * 8;
    Buf b[3] = {in_buf(U, bytes), in_buf(snr, bytes), out_buf(out, bytes)};
    return run(c, mem, b, [&](Buf (&x)[3]) {
        const long long blocks = std::min<long long>((n + 255) / 256, 256 * 16);
        hipLaunchKernelGGL(k_dsig_wspd, dim3((unsigned)blocks), dim3(256), 0, c->stream, (const double *)x[0].dev, (const double *)x[1].dev,
                           (double *)x[2].dev, (long long)n, coef[rule]);
    }, "dsig_wspd");
}
