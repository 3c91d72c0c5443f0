// Host-side types shared by the translation units of libxsw (xsw.hip: context, LUT install, C ABI; xsw_invert_tu.hip: the
// kernel launches of one (input dtype, output dtype) pair each, compiled side by side).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "xsw.h"
#include "xsw_device.hpp"
#include "xsw_plan.hpp"
#include "xsw_lutplan.hpp"

#ifndef XSW_ARENA_KEEP
#define XSW_ARENA_KEEP ((size_t)24 << 30)
#endif
struct xsw_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    xsw::DevTables T{};
    std::vector<void *> co_allocs, cr_allocs;
    bool have_co = false, have_cr = false;
    bool co_finite = false;  // the installed co-pol table holds no NaN / inf (xsw_joint_from_codes refuses others; the cross-pol one: T.cr_finite)
    unsigned long long *d_stats = nullptr;
    bool stats_on = false;
    bool stats_chain = false;               // xsw_stats_enable(ctx, 2): the production chain keeps running, its kernels count what they score
    bool timing_on = false;                 // xsw_timing_enable: HIP events around the kernels of every device-memory inversion
    std::vector<hipEvent_t> timing_events;  // quintuples (start, after k_invert_band, k_invert_band2, k_invert_blocks, k_invert_list) on the launch stream
    size_t lists_bytes = 0;
    WorkLists lists;  // of the device-raster path (context-owned, grown on demand: list G an eighth of the largest raster seen)
    double *d_ratio = nullptr;  // detrend ratio row (context-owned, grown on demand)
    size_t ratio_cap = 0;       // its bytes
    void *nesz_scratch = nullptr;  // xsw_nesz_flatten: column partials + means (context-owned, grown on demand)
    size_t nesz_cap = 0;
    // host-memory paths: worker w owns a stream, a page-locked staging buffer and a device staging buffer, all kept between calls
    struct Worker { hipStream_t s = nullptr; char *pin = nullptr; size_t pin_cap = 0; char *dev = nullptr; size_t dev_cap = 0; };
    std::vector<Worker> workers;
    int host_threads = 0;  // 0: XSW_HOST_THREADS or 12
    char *arena = nullptr;      // whole-raster device staging (xsw_nesz_flatten on host rasters; kept up to XSW_ARENA_KEEP bytes)
    size_t arena_cap = 0;
    std::vector<void *> host_allocs;  // xsw_host_alloc
    // host copies of the output-forming tables (xsw_expand_codes on host memory; the expansion of the host-memory paths)
    std::vector<double> h_sol, h_dual, h_wcr;
    std::vector<float> h_sol32;
    std::string err;
};


static inline void timing_mark(xsw_ctx *c)

{
    if (!c->timing_on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) == hipSuccess && hipEventRecord(e, c->stream) == hipSuccess) c->timing_events.push_back(e);
    else c->timing_on = false;  // never half a quintuple
}


static inline int seterr(std::string &e, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    e = buf;
    return code;
}

// The text xsw_last_error returns: the context's, or this thread's when there is no context yet (xsw_ctx_create).
inline std::string &create_err()
{
    static thread_local std::string e;
    return e;
}
static inline int fail(xsw_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (c ? c->err : create_err()) = buf;
    return code;
}

// Environment knobs: env_int / env_flag (xsw_plan.hpp).  A caller keeps the value in a function-local static, so a knob is read
// once per process.  The switches that shape an inversion are read together, on their first use by an inversion launch
// (launch_invert, ensure_list); not `static inline`: one copy for the whole library, not one per translation unit.
inline const RouteKnobs &route_knobs()
{
    static const RouteKnobs k = RouteKnobs::from_env();
    return k;
}

// ---- device memory.  Two patterns, each spelled once: a sequence of allocations and stream operations whose first error
// sticks (DevSeq; CallTemps is one that owns what it allocates), and a buffer that is kept and replaced by a larger one (grow).
static inline void free_all(std::vector<void *> &v)
{
    for (void *p : v) (void)hipFree(p);
    v.clear();
}

// Allocations recorded in `owner` and operations queued on `stream`, in order; after the first error every later call is a
// no-op that returns nullptr, so a caller writes its steps as a list and asks once.
struct DevSeq {
    hipStream_t stream;
    std::vector<void *> &owner;
    hipError_t err = hipSuccess;
    size_t refused = 0;  // bytes (slack included) of the allocation that failed: the callers' XSW_ENOMEM; 0: any other error

    bool ok() const { return err == hipSuccess; }
    void check(hipError_t e) { if (ok()) err = e; }
    void zero(void *p, size_t bytes) { if (ok()) err = hipMemsetAsync(p, 0, bytes, stream); }
    template <typename F> void run(F &&launches) { if (ok()) { launches(); err = hipGetLastError(); } }  // kernel launches on `stream`
    void *alloc(size_t bytes, const void *host = nullptr, size_t slack = 0)  // host: uploaded, asynchronously
    {
        void *p = nullptr;
        if (!ok()) return nullptr;
        if ((err = hipMalloc(&p, bytes + slack)) != hipSuccess) { refused = bytes + slack; return nullptr; }
        owner.push_back(p);
        if (host && bytes) err = hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, stream);
        return p;
    }
    // a table of a LUT install: count elements and XSW_OWNED_SLACK; one uploaded from `host` is synchronised at once (the
    // host vector may be a temporary of the caller's)
    template <typename V> V *table(size_t count, const V *host = nullptr)
    {
        V *p = (V *)alloc(count * sizeof(V), host, XSW_OWNED_SLACK);
        if (p && host) check(hipStreamSynchronize(stream));
        return p;
    }
    template <typename V> V *table(const std::vector<V> &host) { return table(host.size(), host.data()); }
    // for a table an install can do without: true when every step since the construction succeeded; otherwise the runtime's
    // sticky error is cleared, the caller leaves the table's pointer null and goes on
    bool usable() const { if (!ok()) (void)hipGetLastError(); return ok(); }
    int code() const { return err == hipErrorOutOfMemory ? XSW_ENOMEM : XSW_EHIP; }
};

// Temporaries of one call on one stream: freed after ONE stream synchronisation -- finish(), for a caller that wants its
// result, or scope exit on a path that did not get there (work queued before a failure may still use them).
struct CallTemps : DevSeq {
    std::vector<void *> bufs;
    explicit CallTemps(hipStream_t s) : DevSeq{s, bufs} {}
    ~CallTemps() { if (!bufs.empty()) (void)finish(); }
    hipError_t finish()
    {
        const hipError_t e = hipStreamSynchronize(stream);
        free_all(bufs);
        return e;
    }
};

// A buffer kept between calls (device memory, or page-locked host memory) is replaced here and nowhere else: free, null,
// cap = 0, then `need` bytes (0: release only) and cap = need.  wait_for: work queued on that stream may still use the old
// buffer and is waited for first (nullptr: no wait; a null stream handle is the default stream, hence the pointer); when
// the wait fails the buffer is left as it is.
template <typename P>
static inline hipError_t grow(P *&ptr, size_t &cap, size_t need, const hipStream_t *wait_for = nullptr, bool pinned = false)
{
    hipError_t e = wait_for ? hipStreamSynchronize(*wait_for) : hipSuccess;
    if (e != hipSuccess) return e;
    if (ptr) (void)(pinned ? hipHostFree(ptr) : hipFree(ptr));
    ptr = nullptr;
    cap = 0;
    if (!need) return hipSuccess;
    e = pinned ? hipHostMalloc((void **)&ptr, need, hipHostMallocDefault) : hipMalloc((void **)&ptr, need);
    if (e == hipSuccess) cap = need;
    return e;
}

// Where an inversion launches: its stream and the work lists that hand pixels from k_invert_band to the other kernels (device
// rasters: the context's; host rasters: the worker's own, so that the chunks of different workers run side by side).
struct LaunchCtl {
    hipStream_t stream;
    bool timing;      // xsw_timing_enable events (context stream only)
    WorkLists lists;  // base == nullptr: one-kernel path
};

// What launch_invert's route plan (ChainPlan, xsw_plan.hpp) reads of the tables, the call and its work lists.
static_assert(RouteFacts::PRUNED == XSW_ALGO_PRUNED && RouteFacts::EXHAUSTIVE == XSW_ALGO_EXHAUSTIVE && RouteFacts::EXACT == XSW_ALGO_EXACT &&
              RouteFacts::EXHAUSTIVE_F64 == XSW_ALGO_EXHAUSTIVE_F64, "RouteFacts::Algo (xsw_plan.hpp) is XSW_ALGO_*");
static inline RouteFacts route_facts(const xsw::DevTables &T, const xsw::KArgs &A, int algo, const LaunchCtl &lc)
{
    RouteFacts f;
    f.prunable = T.prunable; f.co_off32 = T.co_off32; f.band_mul24 = T.band_mul24; f.cr_monotone = T.cr_monotone; f.blk_span_ok = T.blk_span_ok;
    f.mono_rows = T.mono_rows; f.inv_rows = T.inv_rows; f.blk = T.blk; f.csphi32 = T.csphi32; f.tail_min = T.tail_min;
    f.n_w = T.n_w; f.n_phi = T.n_phi;
    f.lines = A.lines; f.samples = A.samples; f.n = A.n;
    f.algo = algo;
    f.s_co = A.s_co; f.s_cr = A.s_cr;
    f.mono = !A.s_cr && !A.out_cr && !A.code_cr;
    f.stats = A.stats; f.stats_chain = A.stats_chain;
    f.lists = lc.lists.base; f.mask_strips = lc.lists.mask_strips;
    return f;
}

// A for one chunk of its raster: the chunk's shape, and every raster pointer that is set moved to the chunk's first pixel
// (es: bytes of an input element, os: of an output pixel).
static inline xsw::KArgs slice(const xsw::KArgs &A, const ChunkPlan::Chunk &ch, size_t es, size_t os)
{
    auto shift = [&](auto *p, size_t elem) -> decltype(p) { return p ? (decltype(p))((uintptr_t)p + ch.px0 * elem) : nullptr; };
    xsw::KArgs B = A;
    B.lines = ch.lines; B.samples = ch.samples; B.n = (long long)ch.npx;
    B.inc = shift(A.inc, es); B.s_co = shift(A.s_co, es); B.s_cr = shift(A.s_cr, es);
    B.dsig_cr = shift(A.dsig_cr, es); B.anc = shift(A.anc, es * 2);
    B.out_co = shift(A.out_co, os); B.out_cr = shift(A.out_cr, os);
    B.out_idx = shift(A.out_idx, 12);
    B.code_co = shift(A.code_co, 4); B.code_cr = shift(A.code_cr, 4);
    return B;
}

// The arguments of k_cross_from_codes (xsw_cross.hpp; xsw.h: xsw_cross_from_codes).
namespace xsw {
struct CrossArgs {
    const void *inc, *s_cr, *dsig_cr;  // dsig_cr nullable: dsig_cr_scalar broadcast as in load_pixel
    const unsigned *code_co;           // nullable: every pixel XSW_CODE_NAN (cross-pol only)
    unsigned *code_cr;                 // nullable
    void *out_cr;                      // nullable: complex of the output dtype
    long long n;
    double dsig_cr_scalar;
    int is_db, dual_select;
};

// What the cost and the uncertainty passes read (xsw_cost.hpp, xsw_uncertainty.hpp): the codes and the rasters they were found from.
struct CodesIn {
    const void *inc, *s, *anc, *dsig_cr;  // s: sigma0_co (co-pol kernels, with anc) or sigma0_cr (cross-pol ones, with the nullable dsig_cr)
    const unsigned *code_co, *code_cr;    // cross-pol kernels: code_co nullable (every pixel XSW_CODE_NAN)
    long long n;
    double dsig_co, dsig_cr_scalar;
    int is_db;
};
// k_cost_co / k_cost_cr (xsw.h: xsw_cost_from_codes, xsw_cost_cr_from_codes): each output nullable, reals of the output dtype
struct CostArgs : CodesIn { void *out_J, *out_Jsig, *out_Jwind, *out_res; };
// k_unc_co / k_unc_cr (xsw.h: xsw_uncertainty_from_codes, xsw_uncertainty_cr_from_codes): likewise (k_unc_cr: out_wspd_std alone);
// out_flag: nullable, uint8 XSW_UNC_* bits
struct UncArgs : CodesIn { void *out_wspd_std, *out_dir_std, *out_corr, *out_flag; };

// The arguments of k_joint_from_codes (xsw_joint.hpp; xsw.h: xsw_joint_from_codes).
struct JointArgs {
    const void *inc, *s_co, *anc, *s_cr, *dsig_cr;  // dsig_cr nullable: dsig_cr_scalar broadcast as in load_pixel
    const unsigned *code_co;
    unsigned *out_code;                                  // nullable, as every output
    void *out_J, *out_Jwind, *out_Jsig_co, *out_Jsig_cr;  // reals of the output dtype
    unsigned long long *stats;                           // nullable: [0] pixels searched, [1] candidates scored (xsw_stats_enable)
    long long n;
    double dsig_co, dsig_cr_scalar;
    int is_db;
};

// The arguments of k_unc_joint (xsw_uncertainty_joint.hpp; xsw.h: xsw_uncertainty_joint_from_codes): JointArgs' inputs, each output nullable.
struct UncJointArgs {
    const void *inc, *s_co, *anc, *s_cr, *dsig_cr;  // dsig_cr nullable: dsig_cr_scalar broadcast as in load_pixel
    const unsigned *code_co;
    void *out_wspd_std, *out_dir_std, *out_corr, *out_u_std, *out_v_std, *out_corr_uv;  // reals of the output dtype
    void *out_flag;                                                                     // uint8 XSW_UNC_* bits
    long long n;
    double dsig_co, dsig_cr_scalar;
    int is_db;
};

// The arguments of k_lut_eval_co / k_lut_eval_cr (xsw_forward.hpp; xsw.h: xsw_lut_eval, xsw_lut_eval_cr).
struct FwdArgs {
    const void *inc, *wspd, *phi;          // phi: k_lut_eval_co only
    void *out_db, *out_dwspd, *out_dphi;   // each nullable: reals of the output dtype (k_lut_eval_cr: no out_dphi)
    long long n;
    int fold_phi;
};

// The arguments of k_wspd_solve_co / k_wspd_solve_cr (xsw_solve.hpp; xsw.h: xsw_wspd_solve, xsw_wspd_solve_cr).
struct SolveArgs {
    const void *inc, *s, *phi;             // s: sigma0 in dB; phi: k_wspd_solve_co only
    void *out_wspd, *out_sens, *out_flag;  // each nullable: two reals of the output dtype, uint8 XSW_SOLVE_* bits
    long long n;
    int fold_phi;
};

// The arguments of k_dir_solve_co (xsw_dirsolve.hpp; xsw.h: xsw_dir_solve).
struct DirArgs {
    const void *inc, *s, *wspd, *near;  // s: sigma0 in dB; near: nullable, the reference direction of the selection
    void *out_phi1, *out_phi2, *out_sens1, *out_sens2, *out_phi_near, *out_sens_near, *out_phi_closest;  // each nullable: reals of the output dtype
    void *out_count, *out_flag;         // each nullable: uint8, the number of solutions and the XSW_DIR_* bits
    long long n;
    int fold_phi;
};
}  // namespace xsw

// The launch of every one-pixel-per-lane raster pass (k_cross_from_codes, k_cost_*, k_unc_*, k_lut_eval_*, k_wspd_solve_*, k_dir_solve_co, k_joint_from_codes, k_unc_joint): 256 lanes per block
// over n pixels.  An XSW_* code and, with a non-zero one, its message in `err`.
template <typename Kernel, typename Args>
static int launch_pixels(Kernel kernel, const xsw::DevTables &tables, const Args &A, long long n, hipStream_t stream, std::string &err)
{
    const long long nblocks = (n + 255) / 256;
    if (nblocks > 0x7fffffffLL) return seterr(err, XSW_EINVAL, "raster too large for one launch");
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(256), 0, stream, tables, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(err, XSW_EHIP, "launch failed: %s", hipGetErrorString(e));
    return XSW_OK;
}

// The launches of one (input dtype, output dtype) pair: the inversion kernels, k_cross_from_codes, k_cost_co / k_cost_cr,
// k_unc_co / k_unc_cr, k_lut_eval_co / k_lut_eval_cr, k_wspd_solve_co / k_wspd_solve_cr, k_dir_solve_co, k_joint_from_codes and k_unc_joint.
// Each returns an XSW_* code and, with a non-zero one, its message in `err`.  One instance per translation unit
// (xsw_invert_tu.hip, -DXSW_PAIR=0..3: f32->f32, f32->f64, f64->f32, f64->f64), so that the four sets of kernel
// instantiations compile side by side; it sits behind a host function, which keeps it out of the device pass.
struct PairLaunch {
    int (*invert)(xsw_ctx *c, const xsw::KArgs &A, int algo, const LaunchCtl &lc, std::string &err);
    int (*cross)(xsw_ctx *c, const xsw::CrossArgs &A, hipStream_t stream, std::string &err);
    int (*cost)(xsw_ctx *c, const xsw::CostArgs &A, bool cr, hipStream_t stream, std::string &err);
    int (*unc)(xsw_ctx *c, const xsw::UncArgs &A, bool cr, hipStream_t stream, std::string &err);
    int (*fwd)(xsw_ctx *c, const xsw::FwdArgs &A, bool cr, hipStream_t stream, std::string &err);
    int (*solve)(xsw_ctx *c, const xsw::SolveArgs &A, bool cr, hipStream_t stream, std::string &err);
    int (*dir)(xsw_ctx *c, const xsw::DirArgs &A, hipStream_t stream, std::string &err);
    int (*joint)(xsw_ctx *c, const xsw::JointArgs &A, hipStream_t stream, std::string &err);
    int (*unc_joint)(xsw_ctx *c, const xsw::UncJointArgs &A, hipStream_t stream, std::string &err);
};
const PairLaunch &xsw_pair_0(), &xsw_pair_1(), &xsw_pair_2(), &xsw_pair_3();

// dtype, out_dtype: XSW_F32 or XSW_F64 each (the entries check that first).
static inline const PairLaunch &pair_launch(int dtype, int out_dtype)
{
    static const PairLaunch &(*const pairs[4])() = {xsw_pair_0, xsw_pair_1, xsw_pair_2, xsw_pair_3};
    return pairs[2 * (dtype == XSW_F64) + (out_dtype == XSW_F64)]();
}
