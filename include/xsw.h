/* libxsw -- MI355X (gfx950) wind-inversion hot path of xsarsea, flat C ABI.
 *
 * The reference (umr-lops/xsarsea) is pure Python; its "native" layer for this path is what numba
 * JIT-compiles at run time.  This header is the boundary a maintainer binds with ctypes in place of
 * those JIT kernels.  Each entry point names the reference interface it
 * replaces (paths relative to the reference's src/xsarsea/).
 *
 * Conventions
 *   - every function returns 0 on success, a negative XSW_E* code otherwise; the message is
 *     available from xsw_last_error(ctx);  no exception crosses the ABI;
 *   - pointers are caller-owned; `mem` says whether raster buffers are host or device pointers
 *     (device pointers must belong to the context's device);  LUT/axis pointers are always host;
 *   - rasters are flat, C-contiguous, `lines*samples` pixels; pixels are independent
 *     (the reference's gufunc core dimension "(n)" is only a loop, windspeed/windspeed.py:190);
 *   - complex values are interleaved (re, im);
 *   - a context is bound to one device and one stream; calls on one context are not thread-safe,
 *     different contexts are independent (one process per GPU uses one context; one process driving several GPUs
 *     uses one context per GPU from one host thread each -- xsarsea_amd.options.devices does exactly that).
 *
 * Host rasters (XSW_MEM_HOST) travel through a context-owned ring of page-locked staging buffers filled and drained by
 * host worker threads (XSW_HOST_THREADS, default 12, at most 32), one HIP stream per worker: chunk k is staged, uploaded,
 * inverted, downloaded and written to the caller's output while the other workers do the same for other chunks.  What
 * comes down the link is the answer as 4-byte GRID CODES (see xsw_invert_args.out_code_co), expanded to complex values
 * on the host from the same tables and by the same IEEE operations as on the device: bit-identical, 4 instead of 8 / 16
 * bytes per pixel and output over PCIe.
 */
#ifndef XSW_H
#define XSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XSW_VERSION 4

enum { XSW_F32 = 0, XSW_F64 = 1 };           /* raster element type (complex rasters: c64 / c128) */
enum { XSW_MEM_HOST = 0, XSW_MEM_DEVICE = 1,
       XSW_MEM_HOST_PINNED = 2 /* host rasters in page-locked memory (xsw_host_alloc / hipHostMalloc): DMA reads them directly,
                                  the staging copy of XSW_MEM_HOST is skipped for the inputs */,
       XSW_MEM_DEVICE_SIGMA0_HOST = 3 /* XSW_VERSION >= 3, xsw_invert only: every raster lives in device memory EXCEPT sigma0_co /
                                  sigma0_cr, which are host rasters (pageable).  They travel through the workers' staging ring in
                                  row chunks -- the `stage` callback may fill a chunk itself: the bit-parity route converts
                                  sigma0 to dB there with numpy's own float32 log10 (windspeed.py:126-130) -- and each chunk is
                                  searched on its worker's stream against the resident incidence / ancillary rasters, results
                                  written in place.  Synchronous.  The context's stream is synchronised first. */ };
enum {
    XSW_ALGO_AUTO = 0,       /* pruned when the LUT axes are uniform and finite, else exact        */
    XSW_ALGO_PRUNED = 1,     /* exact branch-and-bound search (production kernel)                   */
    XSW_ALGO_EXHAUSTIVE = 2, /* full (wspd x phi) sweep, LUT slice tiled through LDS; float32 screening,
                                float64 settle (results identical to the reference's)                */
    XSW_ALGO_EXACT = 3,      /* full sweep in the reference's operation order (slow, any LUT)       */
    XSW_ALGO_EXHAUSTIVE_F64 = 4 /* the LDS-tiled sweep with float64 screening                       */
};
enum {
    XSW_OK = 0,
    XSW_EINVAL = -1,   /* bad argument */
    XSW_EHIP = -2,     /* HIP runtime error */
    XSW_ENOLUT = -3,   /* required LUT not uploaded */
    XSW_ENOMEM = -4
};

typedef struct xsw_ctx xsw_ctx;

/* A model LUT in dB, as produced by the reference's Model.to_lut(units="dB") (windspeed/models.py:186-230)
 * but kept incidence-major: co-pol db[n_inc][n_wspd][n_phi], cross-pol db[n_inc][n_wspd] (n_phi = 0).
 * Replaces the closure arrays of _invert_from_model_numpy (windspeed/windspeed.py:144-181).
 *
 * The remaining tables are OPTIONAL (NULL = filled by the library with the host libm).  They exist so
 * that a caller can hand over the values ITS math library produces for the handful of transcendental
 * expressions of the reference whose last bit is platform dependent (numpy dispatches SIMD variants
 * of cos/sin/arctan2/abs), making the device results bit-identical to that caller's CPU path:
 *   cos_phi, sin_phi [n_phi]        cos/sin(radians(phi)) of the candidate vectors (windspeed.py:167-168)
 *   out_dir [2][n_phi][2]           exp(1j*deg2rad(+phi)) and exp(1j*deg2rad(-phi)) as (re, im) (:235-236, :247)
 *   abs_co  [n_wspd][n_phi]         abs(wspd*exp(1j*deg2rad(phi)))  (np.abs(wind_co), :257-274)
 *   dual_dir [2][n_wspd][n_phi][2]  exp(1j*angle(sol)), exp(1j*angle(sol_2)) as (re, im) (:270-276)     */
typedef struct {
    const double *db;
    const double *inc;
    const double *wspd;
    const double *phi;
    const double *cos_phi;
    const double *sin_phi;
    const double *out_dir;
    const double *abs_co;
    const double *dual_dir;
    int32_t n_inc, n_wspd, n_phi;
} xsw_lut;

/* Arguments of one inversion call == the five gufunc inputs and two outputs of
 * __invert_from_model_1d (windspeed/windspeed.py:183-282, wrapper :306-323), plus the sigma0->dB
 * conversion of invert_from_model (:126-130) and the dual-pol select (:426-428) fused on request. */
typedef struct {
    int64_t lines, samples;
    int32_t dtype;          /* XSW_F32 / XSW_F64: inc, sigma0_co, sigma0_cr, dsig_cr; anc is complex of it */
    int32_t out_dtype;      /* XSW_F32 -> complex64 outputs, XSW_F64 -> complex128 (reference)      */
    int32_t mem;            /* XSW_MEM_HOST / XSW_MEM_DEVICE, applies to every raster pointer below   */
    int32_t sigma0_is_db;   /* 0: linear sigma0, converted as 10*log10(x + 1e-15) in `dtype` arithmetic
                               (:126-130);  1: already dB                                             */
    int32_t algo;           /* XSW_ALGO_*                                                             */
    int32_t dual_select;    /* 1: out_cr receives where(|co|<5 or |dual|<5, co, dual) (:426-428)      */
    const void *inc;        /* incidence, degrees                                                     */
    const void *sigma0_co;  /* NULL: no co-pol search (cross-pol only)                                */
    const void *sigma0_cr;  /* NULL: no cross-pol search                                              */
    const void *dsig_cr;    /* NULL: use dsig_cr_scalar (:122-123)                                    */
    const void *anc;        /* ancillary wind, complex, antenna convention; NULL: all NaN             */
    double dsig_co;         /* :24 default 0.1                                                        */
    double dsig_cr_scalar;
    void *out_co;           /* complex; NULL allowed when sigma0_co is NULL                           */
    void *out_cr;           /* complex; NULL: not written                                             */
    int32_t *out_idx;       /* optional int32[n][3] = (i_wspd, i_phi, i_wspd_cr), -1 where no search  */
    /* XSW_VERSION >= 2.  Optional: the answer as grid codes, 4 bytes per pixel and search -- the retrieved wind IS a grid
     * point of the LUT (windspeed.py:228-232, :269), so this is the whole result; xsw_expand_codes turns codes into the
     * complex values out_co / out_cr would have received, bit for bit.  When a code pointer is given the corresponding
     * complex output may be NULL (nothing else is written for that search): 4 B/px instead of 8 or 16 to store, gather
     * over xGMI (multi-GPU) or move over PCIe.
     *   co code: i_wspd * n_phi + i_phi in bits 0..29, bit 30 set when the -phi solution was chosen (:234-242);
     *            XSW_CODE_NAN_RE = (nan, 0) [incidence NaN, :198-201 / ancillary NaN, :204-207], XSW_CODE_NAN = (nan, nan) [:250]
     *   cr code: i_wspd_cr in bits 0..29 (XSW_CODE_NO_INDEX: no cross-pol search ran, wind_dual = (nan, nan) :278), bit 30
     *            (XSW_CODE_PICK_CO) set when dual_select picked the co-pol wind; XSW_CODE_NAN_RE as above.                  */
    uint32_t *out_code_co;
    uint32_t *out_code_cr;
    /* Optional caller-side staging (host rasters only; ignored for XSW_MEM_DEVICE).  When non-NULL, a worker thread that is
     * about to stage pixels [px0, px0 + npx) of input raster `which` (0 inc, 1 sigma0_co, 2 sigma0_cr, 3 dsig_cr, 4 anc) calls
     *     stage(stage_user, which, px0, npx, dst)
     * with `dst` = the page-locked staging area for that piece (npx elements of `dtype`, complex for anc).  Return 1 when the
     * callback has filled dst (the library then does not read the raster pointer, which must still be non-NULL to request the
     * search), 0 to let the library copy from the raster pointer as usual, < 0 to abort the call (XSW_EINVAL is returned).
     * Called concurrently from several threads, for disjoint pieces.  This is how the Python layer runs numpy's own float32
     * log10 (the reference's sigma0 -> dB arithmetic, :126-130) inside the pipeline instead of in a pass of its own. */
    int (*stage)(void *stage_user, int32_t which, int64_t px0, int64_t npx, void *dst);
    void *stage_user;
} xsw_invert_args;

#define XSW_CODE_NAN_RE  0xFFFFFFFFu
#define XSW_CODE_NAN     0xFFFFFFFEu
#define XSW_CODE_PICK_CO  0x40000000u
#define XSW_CODE_NO_INDEX 0x3FFFFFFFu

/* Evaluated-work counters of the last xsw_invert call with stats enabled. */
typedef struct {
    uint64_t pixels_co;        /* pixels that ran a co-pol search                   */
    uint64_t cand_co;          /* co-pol candidates actually scored                 */
    uint64_t pixels_exact;     /* pixels that took the exact full-scan path         */
    uint64_t pixels_cr;        /* pixels that ran a cross-pol search (XSW_ALGO_EXHAUSTIVE: pixels the float32
                                  sweep could not decide, finished by the float64 box search) */
} xsw_stats;

int xsw_version(void);
int xsw_device_count(void);

int xsw_ctx_create(int device, xsw_ctx **ctx);
int xsw_ctx_destroy(xsw_ctx *ctx);
const char *xsw_last_error(const xsw_ctx *ctx); /* ctx may be NULL: last creation error */

/* Launch on a caller-provided hipStream_t (e.g. torch's current stream; NULL = the default stream).
 * A new context launches on a private non-blocking stream; xsw_use_own_stream() returns to it.
 * XSW_MEM_DEVICE buffers are read and written in stream order ON THAT STREAM ONLY: a caller whose producers run on another
 * stream (torch's, say) must either hand that stream over here or synchronise it before xsw_invert / xsw_detrend / ... */
/* Changing the stream orders the new stream after the work the context queued on the previous one (an event the new stream
 * waits for; the host does not block): the work list that hands pixels from k_invert_band to k_invert_list and the scratch of
 * xsw_nesz_flatten are context-owned and reused by the next call. */
int xsw_set_stream(xsw_ctx *ctx, void *hip_stream);
int xsw_use_own_stream(xsw_ctx *ctx);
int xsw_synchronize(xsw_ctx *ctx);

/* Replaces Model.to_lut(...) -> closure arrays (windspeed.py:144-181).  Either may be NULL (kept).
 * Device memory held per context for the default co-pol table (501 x 499 x 181): 368 MB float64 + 184 MB float32 copies,
 * 363 MB transposed copy, 394 MB inverse-row table (first row of every direction at or above each of 2048 dB thresholds
 * per incidence slice: what the band search reads instead of bisecting), 6 MB of block / band {min, max} tables (block
 * pyramid), 6 MB of tail minima, ~10 MB of small tables; all derived copies are produced on the device at install (a few ms). */
int xsw_lut_upload(xsw_ctx *ctx, const xsw_lut *co, const xsw_lut *cr);

/* Replaces _invert_from_model_numpy (windspeed.py:132-331).  Asynchronous on the context's stream
 * when mem == XSW_MEM_DEVICE; synchronous (returns with outputs filled) for host memory.
 * XSW_ALGO_PRUNED on a LUT whose columns rise monotonically with wind speed (every built-in GMF over most of its rows) runs
 * as FOUR launches on one stream:
 *   k_invert_band    decides the pixels its band rule can (windows inside the monotone rows, short runs of band rows; wide windows
 *                    narrowed to the directions in which the band can meet the disc, from the inverse-row table); hands the
 *                    pixels whose band holds a long run of rows along the a-priori direction (XSW_LONG_RUN = 5 or more), or a
 *                    window that reaches past the monotone rows by a tail it can sweep, to list B as 48-byte records;
 *   k_invert_band2   list B: per record a bound from the sigma0 contour itself (inverse-row table), the live arc of directions,
 *                    per direction the joint shrink of band and chord, batched sweep;
 *   k_invert_blocks  list C: the finite pixels the band rule is not for (windows past the monotone rows, bands of thousands of
 *                    candidates, sigma0 outliers): branch-and-bound over min / max tables of LUT cells (32 x 32 candidates), blocks
 *                    (4 x 16) and quarter blocks (4 x 4), both cost terms bound together, four pixels per wave;
 *   k_invert_list    list G: the rest (non-finite inputs, near-ties, whatever overflowed), the general algorithm.
 * The work lists are owned by the context and sized by the largest raster seen (n pixels): list G n/8 entries, lists B and C
 * n/2 entries each (4 bytes per entry), list B's records 48 bytes x n/2, two strip masks of one bit per pixel -- 28.8 bytes per
 * pixel in all (11.5 GB for a 20000 x 20000 raster; HBM holds 288 GB).  A list that overflows is continued in its strip mask:
 * the consumer takes the list, then exactly the marked pixels (stage 1 is redone for those of list B).  If the lists cannot be
 * allocated the one-kernel path runs; any other LUT, and XSW_ALGO_EXACT, take the general kernel (k_invert).
 * Results do not depend on the route.  Environment switches for A/B measurements and the tests of every route: XSW_LONG_RUN=0
 * (no k_invert_band2), XSW_NO_BLOCKS_KERNEL=1, XSW_NO_BAND=1 (general kernel only), XSW_NO_RECORDS=1, XSW_NO_STRIP_MASKS=1,
 * XSW_B2_REFINE_MIN / XSW_B2_AREA / XSW_B2_ROWS_MAX / XSW_TAIL_SWEEP (routing thresholds), XSW_LIST_CAP_TEST / XSW_FAIL_LIST_ALLOC
 * (tiny work lists / none): the table is in INTEGRATION.md, the switches and what follows from them in csrc/xsw_plan.hpp
 * (RouteKnobs, ChainPlan). */
int xsw_invert(xsw_ctx *ctx, const xsw_invert_args *args);

/* Grid codes -> complex winds (the store of __invert_from_model_1d: wind_co = wspd * exp(1j * deg2rad(+-phi)) :235-247,
 * wind_dual = wspd_dual * exp(1j * angle(wind_co)) :270-276), from the tables of the context's current LUTs.  code_co may be
 * NULL when only cross-pol codes exist (cross-pol-only inversion: wind_dual = wspd_dual + 0j), code_cr / out_cr may be NULL.
 * out_dtype XSW_F32 -> complex64, XSW_F64 -> complex128.  mem = XSW_MEM_DEVICE: one HBM-bound kernel, asynchronous on the
 * context's stream; XSW_MEM_HOST: on the calling thread.  Both give the bits xsw_invert writes to out_co / out_cr. */
int xsw_expand_codes(xsw_ctx *ctx, int64_t n, int32_t mem, int32_t out_dtype, const uint32_t *code_co,
                     const uint32_t *code_cr, void *out_co, void *out_cr);

/* XSW_VERSION >= 3.  The device form of xsw_expand_codes on a stream of the caller's choice (a HIP stream handle), without
 * touching the context's launch stream: a consumer that receives codes piece by piece (the row chunks of a multi-GPU gather)
 * expands each piece on a side stream as it lands, next to the inversions still queued on the launch stream. */
int xsw_expand_codes_on_stream(xsw_ctx *ctx, void *stream, int64_t n, int32_t out_dtype, const uint32_t *code_co,
                               const uint32_t *code_cr, void *out_co, void *out_cr);

/* Additive to XSW_VERSION 4.  The cross-pol step of a dual-pol inversion from STORED co-pol codes: replaces windspeed.py:252-278
 * (cross-pol cost Jsig_cr [+ Jwind_cr], argmin, wind_dual = wspd_dual * exp(1j * angle(wind_co))) and, with dual_select, the
 * select :426-428, for a co-pol answer that is already there as xsw_invert's out_code_co.  The code holds all the cross-pol
 * step needs of the co-pol search -- whether it ran, whether the pixel was an early NaN (:198-207), |wind_co| and its direction
 * (tables of the context's co-pol LUT) -- so another cross-pol GMF or another dsig_cr costs ONE pass of 16-20 B per pixel, not
 * the co-pol search again.  out_code_cr / out_cr receive, bit for bit, what one dual-pol xsw_invert of the same rasters writes
 * to out_code_cr / out_cr (either may be NULL, not both).
 *   code_co      the co-pol codes of these pixels from the context's CURRENT co-pol LUT; NULL: every pixel XSW_CODE_NAN, i.e. the
 *                cross-pol-only inversion (J_cr = Jsig_cr, wind_dual = wspd_dual + 0j).  A value that is no code of that LUT
 *                (bit 31 set and neither NaN code, or an index at or beyond n_wspd * n_phi) reads no table: the pixel is
 *                handled as XSW_CODE_NAN_RE.  The ancillary wind is no input: its effect is in the code.
 *   sigma0_cr    `dtype` raster, converted to dB as xsw_invert does (sigma0_is_db as there); dsig_cr a `dtype` raster, or NULL:
 *                dsig_cr_scalar broadcast as sigma0_cr * 0 + dsig_cr in `dtype` (:122-123).
 *   out_dtype    XSW_F32 -> complex64 out_cr, XSW_F64 -> complex128.
 * XSW_ENOLUT without a cross-pol LUT, or with code_co and no co-pol LUT; XSW_EINVAL for both outputs NULL, a NULL inc or
 * sigma0_cr, a bad dtype or mem.  XSW_MEM_DEVICE: one kernel (k_cross_from_codes), asynchronous on the context's stream;
 * XSW_MEM_HOST: upload, kernel, download, returns with the outputs filled. */
int xsw_cross_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                         int32_t sigma0_is_db, int32_t dual_select, const void *inc, const uint32_t *code_co,
                         const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, uint32_t *out_code_cr, void *out_cr);

/* Additive to XSW_VERSION 4.  The VALUE of the minimum the co-pol search found, from its stored codes: J_co = Jwind_co + Jsig_co
 * of windspeed.py:216-225 at the grid point (i_wspd, i_phi) the code names -- the reference takes the arg-min of J and drops
 * J -- with its two terms and the forward-model residual, one pass over the rasters and ONE LUT entry gathered per pixel:
 *   out_J        Jwind + Jsig: bit for bit the minimum of the reference's dense J_co array (float64 arithmetic in its order)
 *   out_Jsig     ((lut_db - sigma0_db) / dsig_co)^2: large where the grid point does not reproduce the observation
 *   out_Jwind    ((w cos(phi) - Re anc) / 2)^2 + ((w sin(phi) - Im anc) / 2)^2, |Im anc| for a 0..180 LUT (:218-219): large where
 *                the retrieval was pulled far from the a-priori wind
 *   out_residual lut_db - sigma0_db, in dB
 * Each output is a `lines x samples` real raster of out_dtype (XSW_F32: the float64 value rounded once) or NULL: a NULL output
 * is not computed and never written; at least one must be given.  inc, sigma0_co (converted to dB as xsw_invert does,
 * sigma0_is_db as there) and anc (complex of `dtype`) are the rasters the codes were computed from, dsig_co that call's.
 * NaN in all outputs: a pixel whose code is XSW_CODE_NAN, XSW_CODE_NAN_RE or no code of the context's CURRENT co-pol LUT (bit 31
 * set, or an index at or beyond n_wspd * n_phi: no table is read), or whose incidence is NaN.  Bit 30 (the -phi solution) does
 * not enter the cost.  A NaN sigma0 or ancillary wind next to a grid code gives NaN by the arithmetic.
 * Bytes per pixel, float32 rasters: 20 read (code, incidence, sigma0, ancillary wind; 12 without out_J / out_Jwind), one 8-byte
 * LUT entry gathered, 4 or 8 written per output.
 * XSW_EINVAL, before any launch, with a message in xsw_last_error: no output requested, no co-pol LUT installed, dsig_co NaN or
 * 0, a NULL input, a bad dtype or mem, a raster too large for one launch (more than 0x7fffffff * 256 pixels).
 * XSW_MEM_DEVICE: one kernel (k_cost_co), asynchronous on the context's stream; XSW_MEM_HOST: upload, kernel, download,
 * returns with the outputs filled. */
int xsw_cost_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                        int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const void *sigma0_co, const void *anc,
                        double dsig_co, void *out_J, void *out_Jsig, void *out_Jwind, void *out_residual);

/* Additive to XSW_VERSION 4.  The same for the cross-pol search (windspeed.py:254-264), from the cross-pol codes xsw_invert or
 * xsw_cross_from_codes wrote (with or without dual_select: XSW_CODE_PICK_CO is ignored, the cost is the cross-pol search's
 * whichever wind the select returned):
 *   out_Jsig     ((lut_cr_db - sigma0_cr_db) / dsig_cr)^2 at i_wspd_cr = the code's index; dsig_cr a `dtype` raster, or NULL:
 *                dsig_cr_scalar broadcast as sigma0_cr * 0 + dsig_cr in `dtype` (:122-123)
 *   out_Jwind    ((wspd_cr - |wind_co|) / 2)^2 where the co-pol code names a grid point of the context's co-pol LUT, else NaN
 *   out_J        Jsig + Jwind, or Jsig alone without a co-pol wind (:259-264): the minimum of the reference's dense J_cr
 *   out_residual lut_cr_db - sigma0_cr_db
 *   code_co      the co-pol codes of these pixels, or NULL: every pixel XSW_CODE_NAN (cross-pol-only inversion)
 * NaN in all outputs: a pixel no cross-pol search ran for (code_cr XSW_CODE_NAN_RE, index XSW_CODE_NO_INDEX, an index at or
 * beyond n_wspd_cr: no table is read) or whose incidence is NaN.  Outputs, out_dtype and mem as in xsw_cost_from_codes.
 * Bytes per pixel, float32 rasters: 16 read (two codes, incidence, sigma0_cr; + 4 with a dsig_cr raster), one 8-byte LUT entry
 * gathered, 4 or 8 written per output.
 * XSW_EINVAL, before any launch: no output requested, no cross-pol LUT installed, code_co given and no co-pol LUT installed, a
 * NULL inc / code_cr / sigma0_cr, a bad dtype or mem, a raster too large for one launch.  One kernel (k_cost_cr). */
int xsw_cost_cr_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                           int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const uint32_t *code_cr,
                           const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, void *out_J, void *out_Jsig,
                           void *out_Jwind, void *out_residual);

/* Additive to XSW_VERSION 4.  The WIDTH of the minimum the co-pol search found, from its stored codes: the error bars of the
 * retrieved wind.  J_co (windspeed.py:216-225) is a Bayesian cost, the posterior is ~ exp(-J / 2), so near the minimum the
 * covariance of (wind speed, direction) is 2 H^-1 with H the Hessian of J.  H is taken by second differences over the 3 x 3
 * grid points around (iw, ip), the point the code names; J[k][l] is the cost at (iw + k, ip + l), evaluated exactly as
 * xsw_cost_from_codes evaluates it (each is an element of the reference's dense J_co, bit for bit), and the spacings are the
 * LUT axes' own (hw- = w[iw] - w[iw-1], hw+ = w[iw+1] - w[iw], hp-, hp+ likewise in degrees; the axes may be non-uniform):
 *   Jww = 2 ((J[1][0] - J[0][0]) / hw+ + (J[-1][0] - J[0][0]) / hw-) / (hw+ + hw-)
 *   Jpp = 2 ((J[0][1] - J[0][0]) / hp+ + (J[0][-1] - J[0][0]) / hp-) / (hp+ + hp-)
 *   Jwp = ((J[1][1] - J[1][-1]) - (J[-1][1] - J[-1][-1])) / ((hw+ + hw-) (hp+ + hp-))
 *   det = Jww Jpp - Jwp Jwp
 *   out_wspd_std sqrt(2 Jpp / det), m/s      out_dir_std sqrt(2 Jww / det), degrees      out_corr -Jwp / sqrt(Jww Jpp)
 *   out_flag     uint8, XSW_UNC_* bits; any bit set: the three real outputs are NaN
 * XSW_UNC_NO_SOLUTION: the code is no grid code of the context's CURRENT co-pol LUT, or the incidence is NaN (the rules of
 * xsw_cost_from_codes).  XSW_UNC_WSPD_BORDER / XSW_UNC_PHI_BORDER: iw / ip is the first or last index of its axis (both may be
 * set).  There is NO wrap of a 0..360 axis and NO mirror of a 0..180 axis -- with a 0..180 LUT the folded cost is not symmetric
 * about 0 / 180 deg, because of |Im anc| -- so a solution on a border has no estimate.  For these three nothing outside the
 * table, indeed nothing of it, is read.  XSW_UNC_NOT_CONVEX: interior, but not (Jww > 0 and Jpp > 0 and det > 0): a saddle or
 * flat stencil, or a NaN sigma0 / ancillary wind next to a valid code.  Bit 30 of the code (the -phi solution) does not enter.
 * Real outputs are `lines x samples` rasters of out_dtype (XSW_F32: the float64 value rounded once), out_flag one of uint8;
 * each may be NULL (not computed, never written), at least one must be given.  Inputs as in xsw_cost_from_codes.
 * Bytes per pixel, float32 rasters: 20 read (code, incidence, sigma0, ancillary wind), nine 8-byte LUT entries gathered as three
 * 24-byte runs phi_pad * 8 bytes apart, 4 or 8 written per real output and 1 for the flag.
 * XSW_EINVAL, before any launch, with a message in xsw_last_error: no output requested, no co-pol LUT installed, dsig_co NaN or
 * 0, a NULL input, a bad dtype or mem, a raster too large for one launch.  XSW_MEM_DEVICE: one kernel (k_unc_co), asynchronous
 * on the context's stream; XSW_MEM_HOST: upload, kernel, download, returns with the outputs filled. */
#define XSW_UNC_NO_SOLUTION 1u
#define XSW_UNC_WSPD_BORDER 2u
#define XSW_UNC_PHI_BORDER  4u
#define XSW_UNC_NOT_CONVEX  8u
int xsw_uncertainty_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                               int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const void *sigma0_co, const void *anc,
                               double dsig_co, void *out_wspd_std, void *out_dir_std, void *out_corr, uint8_t *out_flag);

/* Additive to XSW_VERSION 4.  The 1-D analogue for the cross-pol search: J_cr[k] (windspeed.py:257-264) at icr + k, k = -1, 0, 1,
 * by the rules of xsw_cost_cr_from_codes (Jwind_cr enters only where the co-pol code names a grid point; XSW_CODE_PICK_CO is
 * ignored; code_co NULL: every pixel XSW_CODE_NAN; dsig_cr a raster or NULL: dsig_cr_scalar broadcast):
 *   Jww = the same second difference on the cross-pol speed axis      out_wspd_std sqrt(2 / Jww), m/s
 *   out_flag     XSW_UNC_NO_SOLUTION (no cross-pol search ran for the pixel, an index at or beyond n_wspd_cr, NaN incidence),
 *                XSW_UNC_WSPD_BORDER (icr is 0 or n_wspd_cr - 1), XSW_UNC_NOT_CONVEX (interior, not Jww > 0; also a NaN
 *                sigma0_cr / dsig_cr next to a valid code)
 * Bytes per pixel, float32 rasters: 16 read (+ 4 with a dsig_cr raster), one 24-byte run of the LUT gathered, 4 or 8 + 1 written.
 * XSW_EINVAL, before any launch: no output requested, no cross-pol LUT installed, code_co given and no co-pol LUT installed, a
 * NULL inc / code_cr / sigma0_cr, a bad dtype or mem, a raster too large for one launch.  One kernel (k_unc_cr). */
int xsw_uncertainty_cr_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                  int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const uint32_t *code_cr,
                                  const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, void *out_wspd_std,
                                  uint8_t *out_flag);

/* ---- the joint dual-pol inversion.  Additive to XSW_VERSION 4.  The grid wind of the co-pol LUT that best explains BOTH
 * observations and the a-priori wind: per pixel the arg-min over (iw, ip) of ONE cost
 *     J(iw, ip) = (Jwind_co(iw, ip) + Jsig_co(iw, ip)) + Jsig_cr(iw)
 * where the first two terms are xsw_cost_from_codes' and Jsig_cr(iw) = ((crw - sigma0_cr_db) / dsig_cr)^2 with crw the cross-pol
 * table at the co-pol speed: x = min(max(w[iw], wcr[0]), wcr[n - 1]) (the table is held constant beyond its speed axis),
 * k = clip(searchsorted(wcr, x), 1, n - 1), slope = (cr[i][k] - cr[i][k-1]) / (wcr[k] - wcr[k-1]), crw = slope * (x - wcr[k-1]) +
 * cr[i][k-1], i the nearest cross-pol incidence row.  Float64, IEEE + - * / only; ties go to the smallest iw * n_phi + ip: the
 * result is numpy.argmin of the dense array.  There is no Jwind_cr term: the a-priori speed enters through Jwind_co.
 *   code_co      the co-pol codes of these pixels from the context's CURRENT co-pol LUT (xsw_invert's out_code_co): a real
 *                candidate, hence an upper bound J_ub of the minimum, which confines the search to a window that provably holds
 *                the arg-min.  Any grid code gives the same answer; a good one makes the pass cheap.
 *   inc, sigma0_co, anc, dsig_co   as in xsw_cost_from_codes; sigma0_cr, dsig_cr, dsig_cr_scalar as in xsw_cross_from_codes.
 *   out_code     the joint grid point in the co-pol code format (bit 30: the -phi choice of a 0..180 LUT, by the inversion's own
 *                rule applied to the joint point): xsw_expand_codes reads it.
 *   out_J, out_Jwind, out_Jsig_co, out_Jsig_cr   J and its three terms at the joint point, reals of out_dtype (XSW_F32: one
 *                final rounding).  Every output may be NULL (not computed, never written); at least one must be given.
 * Gates: XSW_CODE_NAN / XSW_CODE_NAN_RE keep their code; a code of no LUT and a NaN incidence give XSW_CODE_NAN_RE; in these the
 * costs are NaN and no table is read.  A grid code next to a NaN sigma0_cr or dsig_cr (no cross-pol information): the input code,
 * the co-pol terms and J = J_co at its point, Jsig_cr NaN.  Otherwise a J_ub that is not finite (NaN sigma0_co or a-priori wind,
 * dsig_cr == 0) gives XSW_CODE_NAN and NaN costs.
 * With xsw_stats_enable the call counts its work: xsw_stats_read's pixels_co = pixels searched, cand_co = candidates scored.
 * XSW_ENOLUT without both LUTs; XSW_EINVAL, before any launch: a NULL input, no output, dsig_co NaN or 0, a bad dtype or mem, a
 * raster too large for one launch, a LUT with a NaN or infinite entry.  An empty raster returns XSW_OK.  XSW_MEM_DEVICE: one
 * kernel (k_joint_from_codes), asynchronous on the context's stream; XSW_MEM_HOST: upload, kernel, download. */
int xsw_joint_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                         int32_t sigma0_is_db, const void *inc, const uint32_t *code_co, const void *sigma0_co, const void *anc,
                         double dsig_co, const void *sigma0_cr, const void *dsig_cr, double dsig_cr_scalar, uint32_t *out_code,
                         void *out_J, void *out_Jwind, void *out_Jsig_co, void *out_Jsig_cr);

/* ---- the error bars of the joint solution.  Additive to XSW_VERSION 4.  xsw_uncertainty_from_codes on a code that
 * xsw_joint_from_codes returned gives the curvature of the CO-POL cost at the joint point, which is not the function that point
 * minimises.  This entry takes the 3 x 3 stencil of the joint cost itself,
 *     J[k][l] = (Jwind_co + Jsig_co)(iw + k, ip + l) + Jsig_cr(iw + k),
 * every element evaluated exactly as xsw_joint_from_codes scores it (bit for bit an element of the dense joint cost), and from
 * it, with the second differences, determinant and convexity test of xsw_uncertainty_from_codes:
 *   out_wspd_std, out_dir_std, out_corr   as xsw_uncertainty_from_codes (m/s, degrees, correlation)
 *   out_u_std, out_v_std, out_corr_uv     the same covariance 2 H^-1 in the components of the complex wind xsw_expand_codes returns
 *                for the code (u = Re, v = Im, antenna convention).  With Sww = 2 Jpp / det, Spp = 2 Jww / det, Swp = -2 Jwp / det,
 *                w = w[iw], c = cos_phi[ip], s = sin_phi[ip] of the installed LUT, r = 0.017453292519943295 -- and, when bit 30 of
 *                the code is set (the wind points along -phi), s and Swp negated: the direction whose covariance with the speed
 *                enters is the wind's own -- tu = -(w s) r, tv = (w c) r (du and dv per degree of that direction):
 *                    var_u  = (c c) Sww + 2 (c tu) Swp + (tu tu) Spp
 *                    var_v  = (s s) Sww + 2 (s tv) Swp + (tv tv) Spp
 *                    cov_uv = (c s) Sww + (c tv + s tu) Swp + (tu tv) Spp
 *                out_u_std sqrt(var_u), out_v_std sqrt(var_v), m/s; out_corr_uv cov_uv / sqrt(var_u var_v).  No clamp: a variance
 *                that rounding makes negative gives NaN.
 *   out_flag     uint8.  XSW_UNC_NO_SOLUTION, XSW_UNC_WSPD_BORDER, XSW_UNC_PHI_BORDER, XSW_UNC_NOT_CONVEX as in
 *                xsw_uncertainty_from_codes, tested in its order: any of them means NaN in all six real outputs, and for the first
 *                three no table is read.  XSW_UNC_NO_CROSSPOL: sigma0_cr or dsig_cr of the pixel is NaN (set whatever the other
 *                bits are).  The joint inversion kept the co-pol answer there; the stencil leaves Jsig_cr out and the real outputs
 *                are xsw_uncertainty_from_codes' bit for bit.  This bit alone does not mean NaN.
 * code: any grid code of the context's CURRENT co-pol LUT, from xsw_joint_from_codes or from the co-pol search.  The other inputs
 * are xsw_joint_from_codes'.  dsig_cr = +inf gives Jsig_cr = 0: xsw_uncertainty_from_codes' outputs, XSW_UNC_NO_CROSSPOL clear.
 * A dsig_cr of 0, an infinite sigma0_cr or a non-finite table entry makes the stencil non-finite and ends in XSW_UNC_NOT_CONVEX
 * (unlike the joint search, a table with such an entry is not refused: nothing here is an arg-min).
 * Every output may be NULL (not computed, never written); at least one must be given.  Bytes per pixel, float32 rasters: 24 read
 * (+ 4 with a dsig_cr raster), three 24-byte runs of the co-pol table and up to three cells of the cross-pol one gathered, 4 or 8
 * written per real output and 1 for the flag.
 * XSW_ENOLUT without both LUTs; XSW_EINVAL, before any launch: a NULL input, no output, dsig_co NaN or 0, a bad dtype or mem, a
 * raster too large for one launch.  An empty raster returns XSW_OK.  XSW_MEM_DEVICE: one kernel (k_unc_joint), asynchronous on
 * the context's stream; XSW_MEM_HOST: upload, kernel, download, one synchronisation. */
#define XSW_UNC_NO_CROSSPOL 16u
int xsw_uncertainty_joint_from_codes(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                                     int32_t sigma0_is_db, const void *inc, const uint32_t *code, const void *sigma0_co,
                                     const void *anc, double dsig_co, const void *sigma0_cr, const void *dsig_cr,
                                     double dsig_cr_scalar, void *out_wspd_std, void *out_dir_std, void *out_corr, void *out_u_std,
                                     void *out_v_std, void *out_corr_uv, uint8_t *out_flag);

/* ---- the forward operator on rasters.  Additive to XSW_VERSION 4.  sigma0 in dB that the context's CURRENT co-pol table
 * T[i][w][p] (axes ai, aw, ap) predicts for the wind (wspd, phi) at incidence inc, per pixel, and the derivatives of that
 * interpolant.  Every input is up-cast to float64; only IEEE + - * / follow, in this order, without fused multiply-adds:
 *   fold (fold_phi != 0 only): p = fmod(phi, 360); if (p < 0) p = p + 360; reflected = p > ap[n_phi - 1]; if (reflected)
 *        p = 360 - p  (sigma0(phi) = sigma0(-phi): a 0..180 table reflects, a 0..360 table never does, a 0..90 table leaves such
 *        a pixel outside).  fold_phi == 0: p = phi, reflected = false.
 *   cell, per axis: hi = clip(first index with axis[hi] >= x, 1, n - 1), lo = hi - 1 (numpy.searchsorted, side left: a value
 *        equal to node j > 0 takes the cell below it).
 *   lerp, always slope = (y_hi - y_lo) / (x_hi - x_lo), y = slope * (x - x_lo) + y_lo: along the incidence for the four (w, p)
 *        corners (v[a][b]), then along the wind speed (slopes s_b, values u_b, b = 0, 1), then along the direction (slope sp).
 *   out_db    the last value, dB
 *   out_dwspd ((s_1 - s_0) / (p_hi - p_lo)) * (p - p_lo) + s_0, dB per m/s
 *   out_dphi  reflected ? -sp : sp, dB per degree
 * NaN in every output where one of the three coordinates is NaN or lies outside [axis[0], axis[n - 1]] (the direction: after the
 * fold); such a pixel reads nothing of the table.  out_db is bit for bit the table's linear interpolation axis by axis
 * (scipy interp1d's statements).  Outputs are `lines x samples` rasters of out_dtype (XSW_F32: the float64 value rounded once);
 * each may be NULL (not computed, never written), at least one must be given.
 * Bytes per pixel, float32 rasters: 12 read, eight 8-byte LUT entries gathered as four adjacent pairs in two incidence planes,
 * 4 or 8 written per output.
 * Before any launch, with a message in xsw_last_error: XSW_ENOLUT without a co-pol LUT; XSW_EINVAL for no output requested, a
 * NULL input, a bad shape, dtype or mem, an axis of the LUT with fewer than two points (there is no cell on it), a raster too
 * large for one launch.  An empty raster returns XSW_OK and launches nothing.  XSW_MEM_DEVICE: one kernel (k_lut_eval_co),
 * asynchronous on the context's stream; XSW_MEM_HOST: upload, kernel, download, returns with the outputs filled. */
int xsw_lut_eval(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, int32_t fold_phi,
                 const void *inc, const void *wspd, const void *phi, void *out_db, void *out_dwspd, void *out_dphi);

/* Additive to XSW_VERSION 4.  The 2-D analogue on the cross-pol table cr[i][w]: incidence, then wind speed; out_dwspd is the
 * speed slope; there is no direction.  Bytes per pixel, float32 rasters: 8 read, four LUT entries gathered as two adjacent
 * pairs, 4 or 8 written per output.  Refusals as xsw_lut_eval, for the cross-pol LUT.  One kernel (k_lut_eval_cr). */
int xsw_lut_eval_cr(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, const void *inc,
                    const void *wspd, void *out_db, void *out_dwspd);

/* ---- wind speed at a known direction: the inverse of xsw_lut_eval along the wind-speed axis.  Additive to XSW_VERSION 4.  The
 * classical SAR scheme: the direction comes from elsewhere (wind streaks, a model), the speed is read off the table at that
 * direction.  Per pixel s = sigma0 in dB, inc, phi; the direction is folded as xsw_lut_eval folds it (fold_phi).  Every input is
 * up-cast to float64; only IEEE + - * / follow, without fused multiply-adds, every lerp in xsw_lut_eval's two statements:
 *   gate     inc, phi or s NaN, inc or phi (after the fold) outside its axis, s not finite: outputs NaN, flag XSW_SOLVE_NAN;
 *            such a pixel reads nothing of the table.
 *   cells    (il, ih) on the incidence axis, (pl, ph) on the direction axis: xsw_lut_eval's.
 *   c(k)     node value at speed node k: the lerp over direction of lerp_inc(T[il][k][pl], T[ih][k][pl]) and
 *            lerp_inc(T[il][k][ph], T[ih][k][ph]) -- incidence FIRST, then direction; xsw_lut_eval orders its axes incidence,
 *            speed, direction, so xsw_lut_eval(inc, out_wspd, phi) returns s to rounding (~1e-13 dB), not bit for bit.
 *   bracket  M = min(mono_rows[il], mono_rows[ih]), the leading rows over which every column of both slices is non-decreasing.
 *            M >= 2: lo = 0, hi = M - 1; while lo < hi: mid = (lo + hi) >> 1; c(mid) < s ? lo = mid + 1 : hi = mid.  j = lo.
 *            c(j) >= s and j > 0: cell k = j - 1.  j == 0 and c(0) == s: k = 0.  Otherwise none in these rows.
 *   tail     no bracket yet, or M < 2: k from max(M - 1, 0) to n_wspd - 2, the first with min(c(k), c(k+1)) <= s <= max(c(k), c(k+1));
 *            found here: XSW_SOLVE_TAIL is set.  None: outputs NaN, flag XSW_SOLVE_BELOW where s < c(0), XSW_SOLVE_ABOVE where
 *            s > c(0) (XSW_SOLVE_NAN where neither holds: a NaN in the table).
 *   solution slope = (c(k+1) - c(k)) / (aw[k+1] - aw[k]); w = aw[k] + (s - c(k)) / slope, aw[k] in a flat cell (c(k+1) == c(k)),
 *            clamped to [aw[k], aw[k+1]].
 *   out_wspd w, m/s: the LOWEST speed that reproduces s; a table that turns over holds a second one higher up
 *   out_sens 1 / slope, m/s per dB (+-inf in a flat cell): |out_sens| * dsig is the a-posteriori speed error
 *   out_flag uint8, XSW_SOLVE_* bits; any of the low three set: the real outputs are NaN.  XSW_SOLVE_TAIL: the answer lies in
 *            the rows past the monotone ones (CMOD5.N turns over below 41 degrees of incidence, from 23.6 m/s on).
 * Real outputs are `lines x samples` rasters of out_dtype (XSW_F32: the float64 value rounded once), out_flag one of uint8; each
 * may be NULL (never written), at least one must be given.
 * Bytes per pixel, float32 rasters: 12 read; per c(k) four 8-byte LUT entries gathered as two adjacent pairs in two incidence
 * planes, about ceil(log2(M)) + 1 of them in the leading rows; 4 or 8 written per real output and 1 for the flag.
 * Before any launch, with a message in xsw_last_error: XSW_ENOLUT without a co-pol LUT; XSW_EINVAL for no output requested, a
 * NULL input, a bad shape, dtype or mem, an axis of the LUT with fewer than two points, a raster too large for one launch.  An
 * empty raster returns XSW_OK and launches nothing.  XSW_MEM_DEVICE: one kernel (k_wspd_solve_co), asynchronous on the context's
 * stream; XSW_MEM_HOST: upload, kernel, download, returns with the outputs filled. */
#define XSW_SOLVE_NAN   1u
#define XSW_SOLVE_BELOW 2u
#define XSW_SOLVE_ABOVE 4u
#define XSW_SOLVE_TAIL  8u
int xsw_wspd_solve(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, int32_t fold_phi,
                   const void *inc, const void *sigma0_db, const void *phi, void *out_wspd, void *out_sens, uint8_t *out_flag);

/* Additive to XSW_VERSION 4.  The 1-D analogue on the cross-pol table cr[i][w]: c(k) = lerp_inc(cr[il][k], cr[ih][k]); no
 * direction.  A table whose rows all rise on a uniform speed axis (the search's cr_monotone) is bisected over all its rows;
 * any other is scanned from row 0, and a bracket the scan finds sets XSW_SOLVE_TAIL as above.  Bytes per pixel, float32
 * rasters: 8 read, two LUT entries gathered per c(k), 4 or 8 + 1 written.  Refusals as xsw_wspd_solve, for the cross-pol LUT.
 * One kernel (k_wspd_solve_cr). */
int xsw_wspd_solve_cr(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, const void *inc,
                      const void *sigma0_db, void *out_wspd, void *out_sens, uint8_t *out_flag);

/* ---- wind direction at a known speed: the inverse of xsw_lut_eval along the direction axis.  Additive to XSW_VERSION 4.  What a
 * dual-pol user needs once xsw_wspd_solve_cr has given a speed that needs no direction: at which directions does the co-pol table
 * give the sigma0 observed?  Per pixel s = sigma0 in dB, inc, w = wind speed; optional `near`, a reference direction in degrees
 * (antenna convention, any range).  Every input is up-cast to float64; only IEEE + - * / (and fmod) follow, without fused
 * multiply-adds, every lerp in xsw_lut_eval's two statements:
 *   gate     inc, w or s NaN, inc or w outside its axis, s not finite: real outputs NaN, count 0, flag XSW_DIR_NAN; such a pixel
 *            reads nothing of the table.
 *   cells    (il, ih) on the incidence axis, (wl, wh) on the speed axis: xsw_lut_eval's.
 *   d(j)     node value at direction node j: lerp_w(lerp_inc(T[il][wl][j], T[ih][wl][j]), lerp_inc(T[il][wh][j], T[ih][wh][j])) --
 *            incidence FIRST, then speed, xsw_lut_eval's order: d(pl), d(ph) are its two direction-cell values bit for bit.
 *   scan     every cell k = 0 .. n_phi - 2 in ascending order.  Cell k holds a solution iff d(k) <= s < d(k+1), or
 *            d(k) >= s > d(k+1), or k == n_phi - 2 and s == d(k+1): low node inclusive, high node exclusive but for the last; a flat
 *            run at s counts once, at its end; a cell with a NaN node holds none.
 *   solution slope = (d(k+1) - d(k)) / (p[k+1] - p[k]); phi = p[k] + (s - d(k)) / slope, p[k] in a flat cell, clamped to
 *            [p[k], p[k+1]]; sens = 1 / slope, degrees per dB (+-inf in a flat cell).
 *   out_phi1 / out_phi2, out_sens1 / out_sens2: the first and second solution in scan order and their sens; NaN where there is none.
 *   out_count uint8: the number of cells holding a solution, saturating at 255.
 *   out_flag  uint8, XSW_DIR_* bits: XSW_DIR_MORE where count > 2; where count == 0, XSW_DIR_BELOW if s < d(0), XSW_DIR_ABOVE if
 *            s > d(0), else XSW_DIR_NAN (a NaN in the table).
 *   out_phi_closest: for every gated pixel p[j] of the first node j that minimises |d(j) - s| among the nodes with a finite d: the
 *            fallback for BELOW / ABOVE (crosswind, or up / downwind).
 *   selection (near given): the candidates are, in scan order, every solution +phi and, with fold_phi, -phi right after it (the
 *            mirror image by sigma0(phi) = sigma0(-phi)); r = fmod(c - near, 360); r < 0: r += 360; dist = r > 180 ? 360 - r : r;
 *            out_phi_near is the candidate of the smallest dist (strict <: the earlier one on a tie), out_sens_near its sens,
 *            negated for a mirrored candidate; over ALL solutions of the scan, not only the two stored.  NaN where near is NaN or
 *            count == 0.
 * Real outputs are `lines x samples` rasters of out_dtype (XSW_F32: the float64 value rounded once), out_count / out_flag of uint8;
 * each may be NULL (never written), at least one must be given.
 * Bytes per pixel, float32 rasters: 12 read (16 with near); the four rows T[il | ih][wl | wh][0 .. n_phi - 1] are walked from entry
 * 0 as aligned 16-byte loads; 4 or 8 written per real output and 1 per uint8 one.  Three float64 divisions per node.
 * Before any launch, with a message in xsw_last_error: XSW_ENOLUT without a co-pol LUT; XSW_EINVAL for no output requested, a
 * NULL inc, sigma0_db or wspd, out_phi_near or out_sens_near without near, a bad shape, dtype or mem, an axis of the LUT with fewer
 * than two points, a raster too large for one launch.  An empty raster returns XSW_OK and launches nothing.  XSW_MEM_DEVICE: one
 * kernel (k_dir_solve_co), asynchronous on the context's stream; XSW_MEM_HOST: upload, kernel, download, returns with the outputs
 * filled.  There is no cross-pol counterpart: that table has no direction axis. */
#define XSW_DIR_NAN   1u
#define XSW_DIR_BELOW 2u
#define XSW_DIR_ABOVE 4u
#define XSW_DIR_MORE  8u
int xsw_dir_solve(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem, int32_t fold_phi,
                  const void *inc, const void *sigma0_db, const void *wspd, const void *near, void *out_phi1, void *out_phi2,
                  void *out_sens1, void *out_sens2, void *out_phi_near, void *out_sens_near, void *out_phi_closest, uint8_t *out_count,
                  uint8_t *out_flag);

/* Page-locked host memory for rasters a caller fills itself (XSW_MEM_HOST_PINNED); freed by xsw_host_free or with the context. */
int xsw_host_alloc(xsw_ctx *ctx, size_t bytes, void **out);
int xsw_host_free(xsw_ctx *ctx, void *p);
/* Host worker threads of the XSW_MEM_HOST paths (0 = default: XSW_HOST_THREADS or 12; at most 32).  Every worker keeps one
 * page-locked staging buffer and one device buffer of a chunk between calls (~2 Mpx: 40 MB each for float32 mono rasters,
 * ~110 MB for float64 dual-pol), so a context holds up to threads x chunk of pinned host memory; after every host-memory call
 * what exceeds XSW_STAGING_KEEP_MB (environment, default 1536 MB per context, a worker counted with the larger of its page-locked
 * and its device buffer: the device side also holds the chunk's work lists and records) is released again, and lowering the thread count
 * frees the workers that are no longer used at once. */
int xsw_set_host_threads(xsw_ctx *ctx, int n);

/* Enable (1) / disable (0) device-side work counters; read them after synchronising.  on = 1: XSW_ALGO_PRUNED runs its statistics
 * instantiation (k_invert_band sweeps every window itself and counts every candidate it scores: cand_co is what the band rule
 * leaves of the grid).  XSW_VERSION >= 4, on = 2: the PRODUCTION chain runs unchanged and the kernels behind k_invert_band count
 * what THEY score (xsw_stats_read_chain): measured candidates per second of k_invert_band2 / k_invert_blocks / k_invert_list. */
int xsw_stats_enable(xsw_ctx *ctx, int on);
int xsw_stats_read(xsw_ctx *ctx, xsw_stats *out);
typedef struct {
    uint64_t cand_band2;      /* candidates scored by k_invert_band2 (after contour bound and joint shrink)          */
    uint64_t cand_blocks;     /* candidates scored by k_invert_blocks (16 per swept quarter block)                    */
    uint64_t cand_list;       /* candidates scored by k_invert_list                                                   */
    uint64_t pixels_refined;  /* list-B records k_invert_band2 put through its refinement (contour bound, live arc)  */
} xsw_chain_stats;
int xsw_stats_read_chain(xsw_ctx *ctx, xsw_chain_stats *out);

/* Measurement aid (no reference counterpart): while enabled, every XSW_ALGO_PRUNED inversion of DEVICE rasters that takes the
 * four-kernel chain (k_invert_band, k_invert_band2, k_invert_blocks, k_invert_list: see xsw_invert) is bracketed by HIP events on the
 * launch stream, one between every two kernels.  xsw_timing_read synchronises, returns the summed durations since the last read and
 * forgets them. */
typedef struct {
    int64_t launches;        /* inversions measured                                                   */
    double first_kernel_ms;  /* k_invert_band, summed over the launches                               */
    double second_kernel_ms; /* k_invert_list, summed over the launches                               */
    int64_t last_list_pixels;/* pixels the most recent launch left to k_invert_list                   */
    double band2_kernel_ms;  /* k_invert_band2 (the pixels with long runs of band rows, between the two), summed   */
    int64_t last_band2_pixels;/* pixels the most recent launch handed to k_invert_band2              */
    double blocks_kernel_ms; /* XSW_VERSION >= 3: k_invert_blocks (block pyramid, after k_invert_band2), summed */
    int64_t last_blocks_pixels;/* pixels the most recent launch handed to k_invert_blocks             */
} xsw_timing;
int xsw_timing_enable(xsw_ctx *ctx, int on);
int xsw_timing_read(xsw_ctx *ctx, xsw_timing *out);

/* Replaces the low->high resolution interpolation of Model._normalize_lut (windspeed/models.py:142-168:
 * `lut.interp(incidence=, wspd=, phi=)`, i.e. three sequential linear 1-D interpolations in the order
 * incidence -> wspd -> phi) on the device, with the arithmetic of scipy.interp1d
 * (slope = (y_hi-y_lo)/(x_hi-x_lo); y = slope*(x_new-x_lo) + y_lo) so that the result is bit-identical.
 * raw[n_inc_raw][n_wspd_raw][n_phi_raw] and out[n_inc][n_wspd][n_phi] are host pointers (n_phi* = 0 for a
 * cross-pol table).  ValueError-equivalent (XSW_EINVAL) when a target point lies outside the raw axis
 * (bounds_error=True) or an axis is not strictly ascending. */
int xsw_lut_interp(xsw_ctx *ctx, const double *raw, const double *inc_raw, const double *wspd_raw,
                   const double *phi_raw, int32_t n_inc_raw, int32_t n_wspd_raw, int32_t n_phi_raw,
                   const double *inc, const double *wspd, const double *phi, int32_t n_inc, int32_t n_wspd,
                   int32_t n_phi, double *out);

/* Device-side LUT preparation for the built-in GMFs (gmf_id: XSW_GMF_* below): evaluates the model on its RAW grid
 * (GmfModel._raw_lut, windspeed/gmfs.py:350-395), brings it to the TARGET grid with the three sequential linear
 * interpolations of Model._normalize_lut (windspeed/models.py:142-168; skipped when the two grids are equal, e.g.
 * resolution="low"), converts to dB (models.py:210-216) and installs the result as the context's co-pol (phi axes given)
 * or cross-pol (n_phi_raw == 0, target->n_phi == 0) LUT, exactly as xsw_lut_upload would -- without the table visiting
 * the host.  `target` carries the target axes and the optional host tables of xsw_lut; target->db is ignored.
 * Values agree with the host-built LUT to ~1e-13 dB (device libm), not bit for bit: use xsw_lut_upload with a
 * host-built table when bit parity with a CPU run is wanted. */
int xsw_lut_build(xsw_ctx *ctx, int32_t gmf_id, const double *inc_raw, int32_t n_inc_raw, const double *wspd_raw,
                  int32_t n_wspd_raw, const double *phi_raw, int32_t n_phi_raw, const xsw_lut *target);

/* Copies the context's current co-pol (cross == 0: out_db[n_inc][n_wspd][n_phi]) or cross-pol (cross != 0:
 * out_db[n_inc][n_wspd]) dB table back to the host, unpadded -- what Model.to_lut(units="dB") would hold
 * (windspeed/models.py:186-230) for a LUT that was built on the device.  Synchronous. */
int xsw_lut_read(xsw_ctx *ctx, int32_t cross, double *out_db);

/* DIAGNOSTIC, no caller needs it: copies one of the tables a co-pol install derived on the device back to the host, whole,
 * pads and slack included (they are part of what the kernels read unmasked), for the tests that hold every table to a host
 * restatement.  Additive to XSW_VERSION 4.  With ppad = n_phi rounded up to 4, wpad = n_wspd rounded up to 4, nbr = ceil(n_wspd /
 * 4), nbc = ceil(n_phi / 16), nbc4 = ceil(n_phi / 4), ncr = ceil(nbr / 8), ncc = ceil(nbc / 2), blk_g = max(1, 64 / nbc) and
 * nbands = ceil(nbr / blk_g) (csrc/xsw_lutplan.hpp: CoGeometry), the tables and their sizes are:
 *   XSW_TAB_CO         double  [n_inc * n_wspd + 260][ppad]          the phi-padded table, 260 slack rows
 *   XSW_TAB_CO32       float   the same layout
 *   XSW_TAB_COT        double  [n_inc][n_phi][wpad] + 512 elements   the transposed slices
 *   XSW_TAB_MONO_ROWS  int32   [n_inc]
 *   XSW_TAB_TAIL_MIN   double  [n_inc][8][ppad]                      optional
 *   XSW_TAB_INV_GRID   double  [n_inc][3]                            optional (with XSW_TAB_INV_ROWS)
 *   XSW_TAB_INV_ROWS   uint16  [n_inc][2048][ppad]                   optional
 *   XSW_TAB_BLK        float   [n_inc][nbr][nbc][2]   {min, max}     optional (with XSW_TAB_CELLMM, XSW_TAB_BANDMM)
 *   XSW_TAB_BLK4       float   [n_inc][nbr][nbc4][2]                 optional
 *   XSW_TAB_CELLMM     float   [n_inc][ncr][ncc][2]                  optional
 *   XSW_TAB_BANDMM     float   [n_inc][nbands][2]                    optional
 *   XSW_TAB_SCALARS    double  [3]: 1.0 when the table holds no NaN / inf else 0.0, the largest finite |dB|, `prunable` (0 or 1)
 * Synchronises the context's stream, then copies; launches nothing.  Returns XSW_OK, or XSW_TAB_ABSENT (> 0, no message, `out`
 * untouched) for an optional table the current install did not build -- its gate failed, an environment switch, an allocation
 * that was refused -- whatever `bytes` says.  XSW_ENOLUT without a co-pol LUT; XSW_EINVAL, `out` untouched, for an unknown id or
 * a `bytes` that is not the table's size. */
enum { XSW_TAB_CO = 0, XSW_TAB_CO32 = 1, XSW_TAB_COT = 2, XSW_TAB_MONO_ROWS = 3, XSW_TAB_TAIL_MIN = 4, XSW_TAB_INV_GRID = 5,
       XSW_TAB_INV_ROWS = 6, XSW_TAB_BLK = 7, XSW_TAB_BLK4 = 8, XSW_TAB_CELLMM = 9, XSW_TAB_BANDMM = 10, XSW_TAB_SCALARS = 11 };
#define XSW_TAB_ABSENT 1
int xsw_lut_table_read(xsw_ctx *ctx, int32_t which, void *out, size_t bytes);

/* Built-in analytic GMFs on the device: out[i] = gmf(inc[i], wspd[i], phi[i]) over n already-broadcast float64
 * elements (phi may be NULL for cross-pol models).  Replaces the numba-vectorised forward GMF of
 * GmfModel.__call__(..., broadcast=True) (windspeed/gmfs.py:202-214, :293-316) for the models of gmfs_impl.py.
 * gmf_id: XSW_GMF_* below.  Values agree with the host evaluation to ~1e-14 relative (device libm), not bitwise. */
enum {
    XSW_GMF_CMOD5 = 0, XSW_GMF_CMOD5N = 1, XSW_GMF_CMOD5N_PR_ZHANGA = 2, XSW_GMF_CMOD5N_PR_MOUCHE1 = 3,
    XSW_GMF_CMODIFR2 = 4, XSW_GMF_RS2_V2 = 5, XSW_GMF_S1_V2 = 6, XSW_GMF_RCM_NOAA = 7, XSW_GMF_S1_V3_EW_REC = 8,
    XSW_GMF_RS2_V3 = 9, XSW_GMF_RCM_V3 = 10, XSW_GMF_RCM_V4 = 11, XSW_GMF_RS2_V4 = 12
};
int xsw_gmf_eval(xsw_ctx *ctx, int32_t gmf_id, int64_t n, int32_t mem, const double *inc, const double *wspd,
                 const double *phi, double *out);

/* Replaces the per-pixel part of sigma0_detrend (detrend.py:63-64):
 * out[l][s] = sigma0[l][s] / ratio_row[s], ratio_row = g / nanmean(g) (float64, host pointer).
 * out is float64 (the reference's result dtype) when out_dtype == XSW_F64.  Host rasters: synchronous; device
 * rasters: asynchronous on the context's stream (ratio_row is consumed before the call returns). */
int xsw_detrend(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                const void *sigma0, const double *ratio_row, void *out);

/* Replaces nesz_flattening (windspeed/utils.py:94-163), the full-raster pass in front of the dual-pol inversion:
 * out[l][s] = 10 ** ((inc_row[s] * slope_l + icpt_l - 1) / 10), with inc_row = nanmean(inc, axis 0), and (slope_l, icpt_l)
 * the degree-1 least-squares fit of 10*log10(noise[l], NaNs replaced by the column nan-mean) against inc_row over the
 * finite samples of line l; a line without any finite sample is NaN.  noise/inc are `dtype` rasters (host or device per
 * `mem`), out is float64 (the reference's result dtype).  Sums are float64 and the fit is closed-form: agrees with
 * numpy's polyfit-based result to ~1e-13 relative for float64 rasters (float32 rasters: float32 dB arithmetic like the
 * reference's own, 1e-5).  Device rasters: asynchronous on the context's stream (scratch is context-owned); host rasters:
 * returns with `out` filled. */
int xsw_nesz_flatten(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *noise,
                     const void *inc, double *out);

/* ---- dsig_cr from the cross-pol signal-to-noise ratio (windspeed/utils.py:47-91 get_dsig, :18-44 get_dsig_wspd).  Additive to
 * XSW_VERSION 4.  mem is XSW_MEM_HOST or XSW_MEM_DEVICE: device calls are asynchronous on the context's stream, host calls
 * upload, run the same kernels, download, and return with `out` filled.  XSW_EINVAL for a bad rule, dtype or mem, a NULL
 * required pointer, or XSW_DSIG_S1_V2 without inc; an empty raster returns XSW_OK and launches nothing. */
enum { XSW_DSIG_S1_V2 = 0,      /* gmf_s1_v2: 1 / sqrt(r ** c), c = d0 + d1 / (1 + exp(-c0 (inc - c1))) */
       XSW_DSIG_RS2_V2 = 1,     /* gmf_rs2_v2: 1 / sqrt(r ** 8) */
       XSW_DSIG_CMODMS1AHW = 2  /* sarwing_lut_cmodms1ahw, nc_lut_cmodms1ahw: (1.25 / r) ** 4 */ };
enum { XSW_DSIG_WSPD_RS2_V3 = 0, XSW_DSIG_WSPD_S1_EW_REC_V3 = 1, XSW_DSIG_WSPD_RCM_V3 = 2 };

/* Replaces get_dsig, elementwise: r = sigma0_cr / nesz_cr, one IEEE division in the common type of the two (`dtype`: sigma0_cr
 * and inc; `nesz_dtype`: nesz_cr).  XSW_DSIG_S1_V2 goes on in float64 and `out` is float64; the other rules go on in the type of
 * r, which is also `out`'s: float32 only when both rasters are.  inc is read by XSW_DSIG_S1_V2 only (NULL otherwise).  Special
 * values as numpy's: r < 0 is NaN under S1_V2 and finite under the even powers, r == 0 gives inf, r == inf gives 0, NaN in gives
 * NaN out.  One kernel (k_dsig). */
int xsw_dsig(xsw_ctx *ctx, int32_t rule, int64_t lines, int64_t samples, int32_t dtype, int32_t nesz_dtype, int32_t mem,
             const void *inc, const void *sigma0_cr, const void *nesz_cr, void *out);

/* get_dsig(rule, inc, sigma0_cr, nesz_flattening(noise, inc)) without the flattened raster: the fit of xsw_nesz_flatten (same
 * kernels, same context scratch), then one pass (k_dsig_flat) that forms each pixel's flattened noise in a register -- the bits
 * xsw_nesz_flatten would have stored -- and applies the rule in float64.  noise, inc and sigma0_cr are `dtype` rasters, all
 * required; out is float64 (the reference's result type) or, with out_dtype == XSW_F32, that value rounded once.  Bit-equal to
 * xsw_nesz_flatten followed by xsw_dsig (nesz_dtype XSW_F64).  Device rasters: asynchronous on the context's stream; the scratch
 * is context-owned, so the stream hand-over rule of xsw_nesz_flatten applies. */
int xsw_dsig_flat(xsw_ctx *ctx, int32_t rule, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem,
                  const void *noise, const void *inc, const void *sigma0_cr, void *out);

/* Replaces get_dsig_wspd on n float64 values: clip(1 / (1 + exp(-b (U - c0 + gamma snr))) * 1 / (1 + exp((U - 30) k)), 0, 1)
 * with the rule's (b, c0, gamma, k).  An exp that overflows gives 0 for its factor, NaN passes through the clip.  One kernel
 * (k_dsig_wspd). */
int xsw_dsig_wspd(xsw_ctx *ctx, int32_t rule, int64_t n, int32_t mem, const double *U, const double *snr, double *out);

/* ---- wind-streak direction histograms (Koch 2004; reference: gradients.py).  Additive to XSW_VERSION 4.  Raster pointers are
 * host or device per `mem` (XSW_MEM_HOST / XSW_MEM_DEVICE); device calls are asynchronous on the context's stream, host calls
 * return with the outputs filled.  Sums are float64 in a fixed order: results are bit-identical from run to run. */

/* Replaces Gradients._sigma0_resample (gradients.py:343-367, cv2.resize INTER_AREA at an integer factor):
 * out[Y][X] = (sum of in[f*Y + i][f*X + j], i, j < f) * (1 / f^2), float64 sums rounded to `dtype` (the output has the input's
 * dtype, as cv2's); NaN propagates.  out is (lines / f) x (samples / f) (floor: the remainder is trimmed). */
int xsw_grad_area(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t factor, int32_t dtype, int32_t mem, const void *in,
                  void *out);

/* Replaces R2 (gradients.py:689-722) and, with take_sqrt != 0, Gradients2D.ampl = sqrt(R2(sigma0)) (:126-134):
 * scipy convolve2d(B4 = B2*B2, 5x5, boundary="symm"), xarray coarsen(2 x 2, boundary="trim").mean() (NaN-skipping: a block
 * with some NaN is the mean of the others, an all-NaN block is NaN), convolve2d(B2, 3x3, "symm") -- each reflection at that
 * stage's own array edge.  The divisions by convolve2d(ones) are divisions by 1.0 and are not performed.  `in` is a float32 or
 * float64 raster (converted to float64 as scipy does), out is float64 (lines / 2) x (samples / 2). */
int xsw_grad_r2(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, int32_t take_sqrt, const void *in,
                double *out);

/* Replaces local_gradients (gradients.py:588-634) on the float64 amplitude raster `ampl` (lines x samples):
 * grad = Scharr_x + 1j * Scharr_y (cv2.Scharr, CV_64F, BORDER_REFLECT_101; dx along sample, dy along line), squared;
 * g2 (complex128) = sqrt(R2(grad**2)) (principal root), g3 = R2(|grad**2|), quality = |R2(grad**2)| / (g3 + 1e-5), set to 0
 * where above 1 or NaN.  Outputs are (lines / 2) x (samples / 2). */
int xsw_grad_local(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *ampl, double *g2, double *g3,
                   double *quality);

/* Replaces Gradients2D.histogram over its windows (gradients.py:87-121 with gradient_histogram :828-879): for every window
 * centre (rows[a], cols[b]) on the g2 / quality grid (lines x samples), the window of xarray's rolling(center=True) -- rows
 * rows[a] - window_lines/2 .. rows[a] - window_lines/2 + window_lines - 1, columns likewise with window_samples, pixels outside
 * the raster are NaN -- is reduced to
 *   kept      = pixels whose |g2| is not NaN and > 0,  m = median(|g2| over kept) (numpy: mean of the middle two for an even count)
 *   weight[a][b][k] = sum over kept of |g2| / (|g2| + m) * quality, k = rint((angle(g2) - angle_start) / angle_step) (round half
 *                     to even), divided by window_lines * window_samples when normalise != 0 (:118-120);  k = n_angles
 *                     (angle = +pi/2) is folded onto bin 0 (the reference raises IndexError there), k = -n_angles .. -1
 *                     are numpy's negative indices; a pixel with any other k (possible only for a g2 that is not a principal
 *                     square root; the reference raises IndexError) is skipped: nothing outside weight[a][b] is written
 *   used_ratio[a][b] = count(kept) / (window_lines * window_samples).
 * One workgroup per window; the median is exact (radix select on the float64 bit patterns, integer counters only).
 * rows (n_rows) and cols (n_cols) are int32 indices; weight is [n_rows][n_cols][n_angles], used_ratio [n_rows][n_cols] (float64). */
int xsw_grad_hist(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *g2, const double *quality,
                  int32_t window_lines, int32_t window_samples, int32_t n_rows, const int32_t *rows, int32_t n_cols, const int32_t *cols, int32_t n_angles, double angle_start,
                  double angle_step, int32_t normalise, double *weight, double *used_ratio);

/* xsw_grad_hist with a keep mask on the g2 / quality grid (`keep`: lines x samples bytes): a pixel whose byte is 0 behaves
 * exactly as if its g2 were NaN -- it is not kept, stays out of the median, adds to no bin and does not count in used_ratio's
 * numerator (the denominator stays window_lines * window_samples).  The thread -> pixel assignment and every summation order are
 * xsw_grad_hist's: the result is bit-identical to xsw_grad_hist on a copy of g2 with NaN written at the masked pixels.  The mask
 * byte is read before g2, so a masked pixel costs 1 B.  keep == NULL is XSW_EINVAL. */
int xsw_grad_hist_masked(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *g2, const double *quality,
                         const uint8_t *keep, int32_t window_lines, int32_t window_samples, int32_t n_rows, const int32_t *rows,
                         int32_t n_cols, const int32_t *cols, int32_t n_angles, double angle_start, double angle_step, int32_t normalise,
                         double *weight, double *used_ratio);

/* Keep masks for xsw_grad_hist_masked: out[i][j] = 1 iff every one of the block x block inputs src[block*i .. ][block*j .. ] is
 * usable, else 0; out is (lines / block) x (samples / block) bytes, rows (samples / block) bytes apart, the remainder of src
 * trimmed.  _f64: usable iff x >= threshold (an IEEE comparison: NaN is not usable; +-Inf thresholds are allowed, a NaN threshold is
 * XSW_EINVAL).  _u8: usable iff non-zero.  and_with (may be NULL) is a mask on the OUTPUT grid that is AND-ed in (non-zero = keep).
 * block is 2 for filtering_parameters' F (half -> quarter resolution) and 4 f for a mask on the sigma0 grid at downscale factor f.
 * XSW_EINVAL for block < 1 or an empty output.  A streaming pass: each input read once, 1 B written per block. */
int xsw_grad_keep_f64(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *src, double threshold, int32_t block,
                      const uint8_t *and_with, uint8_t *out);
int xsw_grad_keep_u8(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const uint8_t *src, int32_t block, const uint8_t *and_with,
                     uint8_t *out);

/* ---- rain / heterogeneity mask (filtering_parameters, gradients.py:758-825).  Additive to XSW_VERSION 4; conventions as above. */

/* R2(sqrt(sigma0)) (gradients.py:773 and :776 with R2 :689-722): xsw_grad_r2 with the square root taken on load, in the input's
 * dtype (float32: the correctly rounded float32 root, widened to float64 afterwards, as np.sqrt on a float32 array; negative
 * input gives NaN).  No full-resolution amplitude raster is written.  out is float64 (lines / 2) x (samples / 2). */
int xsw_grad_r2_sqrt(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *sigma0, double *out);

/* local_gradients(sqrt(sigma0)) (gradients.py:773 and :777 with local_gradients :588-634): xsw_grad_local with the square
 * root taken on load from a float32 or float64 sigma0 raster.  g2 may be NULL (filtering_parameters uses G3 and c only). */
int xsw_grad_local_sqrt(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t dtype, int32_t mem, const void *sigma0, double *g2,
                        double *g3, double *quality);

/* smoothing (gradients.py:675-686): out = scipy convolve2d(x, B2, 3x3, boundary="symm"); the division by convolve2d(ones) is
 * by 1.0 and is not performed.  coarsen == 0: x = in, out is lines x samples.  coarsen != 0: x = the NaN-skipping 2 x 2 mean of
 * `in` with the remainder trimmed (xarray coarsen(trim).mean(), :791), out is (lines / 2) x (samples / 2): the quarter-resolution
 * raster smoothing(resampl) of :794. */
int xsw_grad_smooth(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t coarsen, const double *in, double *out);

/* Mean (gradients.py:724-755): convolve2d(in, B4, "symm") then convolve2d(., B42, "symm"), B42 = convolve(B22, B22) = B4
 * dilated by 2 (9 x 9, 25 non-zero taps k/256), each stage reflecting at the raster's own edge, the divisions by
 * convolve2d(ones, B4) == 1.0 not performed.  Evaluated separably; the zero taps multiply as in scipy's direct sum, so one
 * NaN or Inf makes its whole 9 x 9 footprint NaN.  out is lines x samples. */
int xsw_grad_mean(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *in, double *out);

/* The rest of filtering_parameters (gradients.py:780-819) in one pass over the half-resolution grid (lines x samples here):
 * r2 = R2(ampl), g3 and quality = G3 and c of local_gradients(ampl), smooth4 = smoothing(coarsen(r2)) ((lines / 2) x (samples / 2)).
 *   J = Mean(r2), J1 = Mean(r2**2), P1 = sqrt(J1 - J**2) / (J + 1e-5)     (a negative difference gives NaN)
 *   K = r2 - zoom(smooth4), P2 = K**2 / (J**2 + 1e-5): scipy.ndimage.zoom(order=1, mode="constant", grid_mode=False) to
 *       lines x samples: output o of an axis reads the coordinate o * (n_in - 1) / (n_out - 1), two taps per axis; a tap of
 *       weight 0 still multiplies, and the second tap of the last output is the mirrored element n_in - 2
 *   P3 = g3 / (Mean(g3) + 1e-5), P4 = sqrt(quality)
 *   f_i = clip(a_i P_i + b_i, 0, 1), (a, b) = (-50, 2.75), (-5000, 3), (-2.5, 4), (-10, 6.3); NaN passes through clip
 *   F = sqrt(1/4 (f1**2 + f2**2 + f3**2 + f4**2))
 * out is [5][lines][samples] = f1, f2, f3, f4, F.  Lines :822-823 of the reference cannot run (F has half the shape of
 * image_ori) and are not ported. */
int xsw_grad_filter(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *r2, const double *g3, const double *quality,
                    const double *smooth4, double *out);

/* ---- streak directions -> a-priori wind raster (xsarsea_amd.streaks; the steps of the reference's docs/examples/streaks.ipynb
 * and the ambiguity removal / interpolation that follow them).  Additive to XSW_VERSION 4; conventions as above.  Complex
 * arrays are interleaved (re, im) float64 pairs, antenna convention (re = sample axis, im = line axis). */

/* The notebook's hist.mean(pol, downscale_factor, window_size) -> circ_smooth -> peak bin, one wave per window:
 *   m[a]  = NaN-skipping mean of weight[c][w][a] over c (sum in the order of c, one division by the count; all NaN -> NaN)
 *   m     = Bx, Bx2, Bx4, Bx8 applied circularly in that order when smooth != 0 (gradients.py:882-923; every tap of a kernel
 *           multiplies, the zero ones too, the sum starting at 0 with the first tap)
 *   index[w] = the first arg-max of (isnan(m) ? 0 : m) (an all-zero or all-NaN window: 0), weight_out[w] = m[index[w]] (NaN stays
 *   NaN), used_ratio_out[w] = NaN-skipping mean of used_ratio[c][w] over c.
 * weight is [n_lead][n_windows][n_angles], used_ratio [n_lead][n_windows] (n_lead = product of the histogram's leading axes, >= 1);
 * n_angles 8 .. 512, XSW_EINVAL outside.  The caller turns index into an angle with its own table of bin centres. */
int xsw_streaks_peak(xsw_ctx *ctx, int64_t n_lead, int64_t n_windows, int32_t n_angles, int32_t mem, int32_t smooth, const double *weight,
                     const double *used_ratio, int32_t *index, double *weight_out, double *used_ratio_out);

/* Removes the 180 degree ambiguity of the windows' unit vectors dirs[w] (complex) against the a-priori wind ancillary[w]
 * (complex, the value at the window): out[w] = -dirs[w] when dirs.re * anc.re + dirs.im * anc.im < 0, else dirs[w] (a zero dot
 * product keeps it); NaN + NaN j where dirs[w] or weight[w] is NaN, where ancillary[w] has a NaN part or is 0, where
 * weight[w] < min_weight or used_ratio[w] < min_used_ratio (a NaN threshold switches that test off). */
int xsw_streaks_resolve(xsw_ctx *ctx, int64_t n_windows, int32_t mem, const double *dirs, const double *weight, const double *used_ratio,
                        const double *ancillary, double min_weight, double min_used_ratio, double *out);

/* The a-priori raster of the inversion from the resolved window directions dirs [n_rows][n_cols] (complex; NaN = no direction):
 * per pixel (l, s) of the lines x samples complex raster `ancillary`, with the bracket of each axis prepared by the caller --
 * i0 = line_first[l], i1 = min(i0 + 1, n_rows - 1), weights wl = (1 - line_t[l], line_t[l]); j0, j1, ws likewise from
 * sample_first / sample_t (indices are clamped into range, never trusted) --
 *   v   = sum over the corners (i0,j0), (i0,j1), (i1,j0), (i1,j1), in that order and from 0, of (wl * ws) * dirs[corner],
 *         NaN corners skipped
 *   out = hypot(a) * v / hypot(v) per part ((|a| * v.re) / |v|: one multiplication, one IEEE division);  out = a where
 *         hypot(v) == 0 (no valid corner, or they cancel);  out = NaN + NaN j where a has a NaN part.
 * HBM-bound: 16 B read and 16 B written per pixel, the bracket tables and dirs stay in cache.  out must not alias ancillary. */
int xsw_streaks_ancillary(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, const double *ancillary, int32_t n_rows, int32_t n_cols,
                          const double *dirs, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                          const double *sample_t, double *out);

/* ---- a-priori wind raster from a coarse model grid (xsarsea_amd.ancillary; what the reference's
 * docs/examples/windspeed_retrieval_L1.ipynb does by hand before the inversion).  Additive to XSW_VERSION 4; conventions as above.
 *
 * The complex128 lines x samples raster `out` (antenna convention) from the model wind u, v [n_lat][n_lon] (dtype XSW_F32 or
 * XSW_F64, both of it; eastward / northward components, "blowing to") on the uniform grid lon0 + i * dlon, lat0 + j * dlat
 * (n_lat, n_lon >= 2; dlon, dlat finite and non-zero, dlat signed) and the scene's tie-point grid [n_tie_lines][n_tie_samples]:
 * tie_lon, tie_lat in degrees (continuous: no jump of 360 between neighbours) and tie_cos, tie_sin, the cosine and sine of the
 * ground heading (the azimuth of the line axis from north), which the caller computes: the kernel calls no trigonometric
 * function.  The bracket of each raster axis between tie points is prepared by the caller as for xsw_streaks_ancillary --
 * i0 = line_first[l], i1 = min(i0 + 1, n_tie_lines - 1), weights wl = (1 - line_t[l], line_t[l]); j0, j1, ws likewise from
 * sample_first / sample_t (indices are clamped into range, never trusted).  Per pixel (l, s), every operation float64 and
 * rounded once, in this order:
 *   f(l, s) = wl0 * (ws0 * f[i0][j0] + ws1 * f[i0][j1]) + wl1 * (ws0 * f[i1][j0] + ws1 * f[i1][j1])   for f = lon, lat, cos, sin
 *   n = hypot(cos, sin), ch = cos / n, sh = sin / n       (n == 0, the headings cancel: the pixel is NaN + NaN j)
 *   x = (lon - lon0) / dlon, y = (lat - lat0) / dlat
 *   periodic != 0 (the longitude axis closes: n_lon * dlon is 360):  x = x - floor(x / n_lon) * n_lon, and 0 where that is not
 *     inside [0, n_lon);  cell i = floor(x), its upper node i + 1, or 0 after node n_lon - 1
 *   otherwise, and always for y:  the pixel is NaN + NaN j unless 0 <= x <= n - 1;  cell i = min(floor(x), n - 2), so that a
 *     pixel exactly on the last node uses cell n - 2 with weight 1
 *   tx = x - i, ty = y - j
 *   g = (1 - ty) * ((1 - tx) * g[j][i] + tx * g[j][i + 1]) + ty * ((1 - tx) * g[j + 1][i] + tx * g[j + 1][i + 1])   for g = u, v
 *     (plain arithmetic: a NaN node makes the pixel NaN, also where its weight is 0)
 *   out = -(u + 1j v) * (ch + 1j sh):  re = -(u * ch - v * sh), im = -(u * sh + v * ch)
 * which is the notebook's speed * exp(1j * dir_meteo_to_sample((90 - atan2(v, u) in degrees + 180) % 360, heading)) in closed
 * form; the sign is the GMF's "from" sense (heading 0, a wind blowing to the east: -speed).
 * Nothing is read per pixel but the eight nodes, which stay in cache; 16 B are written. */
int xsw_ancillary_model(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t dtype, const void *u, const void *v, int32_t n_lat,
                        int32_t n_lon, double lon0, double dlon, int32_t periodic, double lat0, double dlat, int32_t n_tie_lines,
                        int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos, const double *tie_sin,
                        const int32_t *line_first, const double *line_t, const int32_t *sample_first, const double *sample_t, double *out);

/* ---- wind product cells: block statistics of a raster on a product grid (xsarsea_amd.cells), the way out of device memory:
 * kilobytes instead of the raster.  Additive to XSW_VERSION 4; conventions as above.
 *
 * The lines x samples raster is tiled from pixel (0, 0) by cells of cell_lines x cell_samples pixels: nLc = ceil(lines /
 * cell_lines) by nSc = ceil(samples / cell_samples) cells, the last cell of an axis clipped to the raster.  Every output is
 * [nLc][nSc].  A cell's pixels are numbered p = r * w + c, r the row and c the column inside the cell, w the cell's actual
 * (clipped) width.
 *
 * Validity.  A pixel is valid iff its keep byte is non-zero (keep NULL: all are) and
 *   XSW_CELLS_C128 / XSW_CELLS_C64 (interleaved (re, im) float64 / float32 pairs): neither part is NaN;
 *   XSW_CELLS_CODES (co-pol grid codes, out_code_co above): the code names a grid point of the context's CURRENT co-pol LUT
 *     (bit 31 clear and the flat index below n_wspd * n_phi); its (re, im) is the `sol` entry xsw_expand_codes reads, so codes
 *     give bit for bit what the expanded complex128 raster gives;
 *   a real raster: the value is not NaN.
 * Invalid pixels contribute nothing to any sum.
 *
 * Order of every sum.  All arithmetic is float64 (float32 inputs are widened first), every operation rounded once:
 *   pixel p goes to accumulator p mod 256; each of the 256 accumulators starts at +0.0 and adds its pixels in ascending p;
 *   then a[i] += a[i + h] for i < h, for h = 128, 64, 32, 16, 8, 4, 2, 1; a[0] is the sum.
 * The order does not depend on how the launch maps lanes to pixels (one wave or one workgroup per cell: csrc/xsw_cells.hip),
 * no atomic is used, and tests/cells_ref.py restates it in numpy bit for bit.  It lies within (N - 1) * 2**-53 * sum|x| of the
 * exact sum.
 *
 * Sums per cell.  Wind: per valid pixel q = re * re + im * im, s = sqrt(q); n, Sre, Sim, Ss, Sq.  Real: n, Sx, Sxx (x * x).
 * Per cell from the sums, n used as a double:
 *   count      = n (int32)
 *   wind       = Sre / n + 1j * Sim / n                      the vector mean, antenna convention (interleaved pair)
 *   wspd       = Ss / n                                      the scalar mean
 *   wspd_std   = NaN for n < 2, else sqrt(var < 0 ? 0 : var) with var = (Sq - (Ss * Ss) / n) / (n - 1)
 *   steadiness = sqrt(mre * mre + mim * mim) / wspd          (mre, mim the parts of wind; NaN where wspd is 0)
 *   mean = Sx / n, std from Sxx, Sx, n by the expression of wspd_std
 * n = 0 gives NaN everywhere (0 / 0) with count 0; there is no minimum count: the caller masks on count.
 *
 * With tie points (tie_lon != NULL; tie grids, tie_cos / tie_sin and the brackets as for xsw_ancillary_model, the brackets being
 * those of the cells' CENTRE coordinates: line_first / line_t [nLc], sample_first / sample_t [nSc]): lon, lat, ch, sh at the centre
 * by exactly the first two steps of xsw_ancillary_model (the same device code), then
 *   u = -(mre * ch + mim * sh),  v = -(mim * ch - mre * sh)
 * the east / north components ("blowing to", the inverse of xsw_ancillary_model's last step), and longitude / latitude of the
 * centre (the tie points' continuous longitude, not wrapped).  tie_lon == NULL: no geolocation; the four geographic outputs must
 * then be NULL.  Every output pointer may be NULL: it is not computed and never written. */
enum { XSW_CELLS_C128 = 0, XSW_CELLS_C64 = 1, XSW_CELLS_CODES = 2 };
int xsw_wind_cells(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                   int32_t cell_lines, int32_t cell_samples, int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon,
                   const double *tie_lat, const double *tie_cos, const double *tie_sin, const int32_t *line_first, const double *line_t,
                   const int32_t *sample_first, const double *sample_t, int32_t *out_count, double *out_wind, double *out_wspd,
                   double *out_wspd_std, double *out_steadiness, double *out_longitude, double *out_latitude, double *out_u, double *out_v);

/* The same for a real raster x (dtype XSW_F32 or XSW_F64): count, mean and std per cell. */
int xsw_raster_cells(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t dtype, const void *x, const uint8_t *keep,
                     int32_t cell_lines, int32_t cell_samples, int32_t *out_count, double *out_mean, double *out_std);

/* ---- wind on a regular longitude / latitude grid (xsarsea_amd.grid): order-free binning in fixed point, the building block of
 * maps, mosaics of several scenes and tiled or multi-GPU reductions.  Additive to XSW_VERSION 4; conventions as above.
 *
 * Every pixel of the lines x samples source (src_kind, src, keep: the kinds, the validity rule and the keep rule of
 * xsw_wind_cells) is geolocated from the scene's tie points (REQUIRED here: the four grids, and the PER-PIXEL brackets
 * line_first / line_t [lines], sample_first / sample_t [samples], prepared exactly as for xsw_ancillary_model) and adds five
 * 64-bit integers to the bin of the grid it falls into.  The grid: n_lon x n_lat bins, bin (j, i) covering
 * [lon0 + i * dlon, lon0 + (i + 1) * dlon) x the latitudes between lat0 + j * dlat and lat0 + (j + 1) * dlat; lon0 and lat0 are
 * the EDGES of bin 0, not nodes; dlon > 0; dlat finite, non-zero and signed (a descending axis: dlat < 0); n_lon, n_lat >= 1 and
 * n_lon * n_lat fits int32; periodic is 0 or 1.  sums: int64 [5][n_lat][n_lon], the planes n, Su, Sv, Ss, Sq.  The entry ADDS
 * into sums; the caller zeroes them (XSW_MEM_HOST: sums is copied up, added to and copied down).
 *
 * Per pixel, every operation float64 and rounded once, in this order:
 *   1. (lon, lat, ch, sh): steps 1-2 of xsw_ancillary_model, unchanged (the same device code)
 *   2. re, im widened to float64;  q = re * re + im * im,  sp = sqrt(q),  u = -(re * ch + im * sh),  v = -(im * ch - re * sh)
 *      (the cells' expressions, per pixel and with the pixel's own heading)
 *   3. x = (lon - lon0) / dlon,  y = (lat - lat0) / dlat
 *      periodic != 0 (n_lon * dlon is 360):  x = x - floor(x / n_lon) * n_lon, and 0 where that is not inside [0, n_lon)  (the
 *        rule of xsw_ancillary_model);  otherwise, and always for y:  the pixel is dropped unless 0 <= x < n: the upper edge is
 *        outside;  i = floor(x), j = floor(y)
 *   4. the pixel is dropped unless the source is valid, keep is non-zero, u and v are not NaN (cancelling headings give NaN) and
 *      q < 65536 (a speed below 256 m/s)
 *   5. bin (j, i):  n += 1,  Su += Q24(u),  Sv += Q24(v),  Ss += Q24(sp),  Sq += Q16(q)
 *      with Q24(a) = llrint(a * 16777216.0), Q16(a) = llrint(a * 65536.0), rounding half to even
 * Integer addition has no order: any launch geometry, any pre-aggregation, any split of a scene into tiles, any order of scenes
 * and any number of devices whose planes are added afterwards give the same bits.  tests/grid_ref.py restates the entry in numpy.
 *
 * Overflow.  Every addend is below 2**32 * (1 + 2**-50) in magnitude (step 4's last condition makes this unconditional), so a
 * bin is exact up to 2**30 pixels over all accumulated calls (a 20000 x 20000 scene has 2**28.6 pixels in all).  This is not
 * checked at run time.
 *
 * Finish (not part of the entry: elementwise on the grid, in the caller's float64), with nd = (double)n:
 *   u = ((double)Su / nd) * 2**-24, v and wspd (from Ss) likewise;  s1 = (double)Ss * 2**-24,  s2 = (double)Sq * 2**-16,
 *   var = (s2 - (s1 * s1) / nd) / (nd - 1),  wspd_std = NaN for n < 2, else sqrt(var < 0 ? 0 : var),
 *   steadiness = sqrt(u * u + v * v) / wspd;  n == 0 gives NaN everywhere.
 * A mean differs from the exact mean of the per-pixel values by at most 2**-25 (the quantisation) + the division's rounding.
 *
 * Environment XSW_GRID_PATH = direct | lds, read at every call (any other value is refused): `direct` sends every pixel's five
 * adds straight to global memory, `lds` (the default) pre-aggregates per thread and per workgroup first.  Both give the same bits. */
int xsw_wind_grid(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                  int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                  const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                  const double *sample_t, double lon0, double dlon, int32_t n_lon, int32_t periodic, double lat0, double dlat,
                  int32_t n_lat, int64_t *sums);

/* ---- wind around a given centre (xsarsea_amd.polar): the storm-centred description of a cyclone scene -- azimuthal means, the
 * largest speed, the radial and tangential components -- binned in rings and sectors, order-free in fixed point as
 * xsw_wind_grid.  Additive to XSW_VERSION 4; conventions as above.
 *
 * Source, keep, tie points and per-pixel brackets: exactly as xsw_wind_grid.  The bins: n_r rings of width dr_km (> 0) around
 * the centre (lon_c, lat_c: finite, |lat_c| <= 89), ring k covering [k * dr_km, (k + 1) * dr_km); each ring has n_theta sectors
 * counted clockwise from north, sector 0 starting at north; n_theta is a multiple of 4 from 4 to 360, so that the quadrant
 * borders are sector borders; n_r >= 1 and n_r * n_theta fits int32.  cos_lat_c, sin_lat_c: cos and sin of lat_c, by the caller.
 * sector_sin, sector_cos [n_theta / 4 + 1]: sin and cos of j * 90 / (n_theta / 4) degrees, j = 0 .. n_theta / 4, by the caller:
 * the device calls no trigonometric function.  sums: int64 [6][n_r][n_theta], the planes n, Ss, Sq, Sr, St, Mx.  The entry
 * ACCUMULATES into sums: the first five planes are added to, Mx is raised to the maximum (unsigned 64-bit; the value is never
 * negative); the caller zeroes them (XSW_MEM_HOST: sums is copied up, accumulated into and copied down).
 *
 * Per pixel, every operation float64 and rounded once, in this order, with R = 6371.0088 (km), D = 0.017453292519943295
 * (pi / 180) and K = R * D (one rounding):
 *   0. once per call:  lon_c = lon_c - 360 * rint(lon_c / 360)   (a centre given as -179.6 or as 180.4 is the same centre)
 *   1. (lon, lat, ch, sh): steps 1-2 of xsw_ancillary_model, unchanged (the same device code)
 *   2. q, sp, u, v: step 2 of xsw_wind_grid, unchanged
 *   3. dl = lon - lon_c;  dl = dl - 360 * rint(dl / 360)  (halves to even);  dy = (lat - lat_c) * D;  h = 0.5 * dy
 *      m = (cos_lat_c - sin_lat_c * h) - (0.5 * cos_lat_c) * (h * h)      (cos of the mid-latitude to second order)
 *      x = (K * dl) * m  (east, km);   y = R * dy  (north, km)
 *   4. rr = x * x + y * y,  r = sqrt(rr),  kr = floor(r / dr_km);  the pixel is dropped unless kr < n_r
 *   5. the quadrant Q and the pair (a, b), from signs alone:
 *        Q = 0 if x >= 0 and y > 0:  (a, b) = (x, y)         Q = 1 if x > 0 and y <= 0:  (a, b) = (-y, x)
 *        Q = 2 if x <= 0 and y < 0:  (a, b) = (-x, -y)       Q = 3 if x < 0 and y >= 0:  (a, b) = (y, -x)
 *        x = y = 0:  Q = 0 and sector 0
 *      with mq = n_theta / 4:  lo = 0, hi = mq;  while hi - lo > 1:  mid = (lo + hi) >> 1;
 *        if a * sector_cos[mid] >= b * sector_sin[mid]:  lo = mid  else  hi = mid
 *      sector = Q * mq + lo
 *   6. vr = (u * x + v * y) / r  (outward),  vt = (v * x - u * y) / r  (positive counter-clockwise);  both 0 where r == 0
 *   7. the pixel is dropped unless the source is valid, keep is non-zero, u and v are not NaN and q < 65536
 *   8. bin (kr, sector):  n += 1,  Ss += Q24(sp),  Sq += Q16(q),  Sr += Q24(vr),  St += Q24(vt),  Mx = max(Mx, Q24(sp))
 *      with Q24 and Q16 as in xsw_wind_grid
 * Integer addition and the maximum have no order: what xsw_wind_grid says of launches, tiles, scenes and devices holds here,
 * with "planes 0-4 added, plane 5 the maximum" as the merge.  tests/polar_ref.py restates the entry in numpy.
 *
 * The chart.  (x, y) is the equirectangular chart at the mid-latitude, its cosine expanded to second order around lat_c; against
 * the great-circle distance and initial bearing it is off by less than 2e-4 of the distance and 1.5 degrees of bearing out to
 * 300 km for |lat_c| <= 35 (tests/test_polar_cpu.py measures it; DESIGN has the figures).
 *
 * Overflow.  |vr|, |vt| <= sp up to rounding, so every addend is below 2**33 in magnitude (step 7's last condition makes this
 * unconditional) and a bin is exact up to 2**30 pixels over all accumulated calls, as in xsw_wind_grid.  Not checked at run time.
 *
 * Finish (not part of the entry: elementwise on the bins, in the caller's float64), with nd = (double)n:
 *   wspd = ((double)Ss / nd) * 2**-24, vr and vt (from Sr, St) likewise;  wspd_std from Ss and Sq as in xsw_wind_grid;
 *   vmax = (double)Mx * 2**-24;  n == 0 gives NaN everywhere.
 *
 * Environment XSW_GRID_PATH = direct | lds, read at every call (any other value is refused), with the meaning it has for
 * xsw_wind_grid.  Both give the same bits. */
int xsw_wind_polar(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                   int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                   const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                   const double *sample_t, double lon_c, double lat_c, double cos_lat_c, double sin_lat_c, double dr_km, int32_t n_r,
                   int32_t n_theta, const double *sector_sin, const double *sector_cos, int64_t *sums);

/* ---- the cyclone centre from the wind field (xsarsea_amd.centre): the annulus sums of xsw_wind_polar around every node of a
 * lattice of candidate centres, in one pass over the raster: what a search for the circulation centre (the largest mean
 * tangential wind in an annulus near the radius of maximum wind), the calmest disc, the highest or the most uniform annulus
 * speed scores its candidates with.  Additive to XSW_VERSION 4; conventions as above.
 *
 * Source, keep, tie points and per-pixel brackets: exactly as xsw_wind_grid.  (lon_g, lat_g): the first guess, finite,
 * |lat_g| <= 89, the centre of the chart; cos_lat_g, sin_lat_g: cos and sin of lat_g, by the caller.  The candidates: an
 * n_c x n_c lattice on that chart, n_c odd, 1 <= n_c <= 31, spaced step_km (finite, > 0; with n_c == 1 step_km is not read and
 * the one candidate is the first guess).  The annulus: r_in_km <= r < r_out_km around each candidate, both finite,
 * 0 <= r_in_km < r_out_km.  sums: int64 [5][n_c][n_c], the planes n, Ss, Sq, Sr, St: planes 0-4 of xsw_wind_polar, in its
 * units.  The entry ADDS into sums; the caller zeroes them (XSW_MEM_HOST: sums is copied up, added to and copied down).
 *
 * Per pixel, every operation float64 and rounded once:
 *   0. once per call:  lon_g = lon_g - 360 * rint(lon_g / 360)
 *   1.-3. (lon, lat, ch, sh), then q, sp, u, v, then (x, y) in km: steps 1-3 of xsw_wind_polar with (lon_g, lat_g, cos_lat_g,
 *      sin_lat_g) as its centre, unchanged
 *   4. the pixel is dropped unless the source is valid, keep is non-zero, u and v are not NaN and q < 65536
 * Per pixel and candidate (i, j), with h = (n_c - 1) / 2:
 *   5. cy = (double)(i - h) * step_km  (row i runs south to north),  cx = (double)(j - h) * step_km  (both 0 for n_c == 1)
 *   6. dx = x - cx,  dy = y - cy,  r = sqrt(dx * dx + dy * dy);  the pixel counts iff r_in_km <= r && r < r_out_km (a NaN fails)
 *   7. vr = (u * dx + v * dy) / r,  vt = (v * dx - u * dy) / r;  both 0 where r == 0
 *   8. sums[:, i, j]:  n += 1,  Ss += Q24(sp),  Sq += Q16(q),  Sr += Q24(vr),  St += Q24(vt), Q24 and Q16 as in xsw_wind_grid
 * With n_c == 1 and r_in_km == 0 the sums are those of xsw_wind_polar with one ring of r_out_km, added over its sectors.
 * Integer addition has no order: what xsw_wind_grid says of launches, tiles, scenes and devices holds here, and so does its
 * overflow statement: a candidate is exact up to 2**30 pixels over all accumulated calls.  tests/centre_ref.py restates the
 * entry in numpy.  Finish: wspd, wspd_std, vr, vt as in xsw_wind_polar.
 *
 * XSW_EINVAL, before any launch: a NULL source, sums or tie table, a bad src_kind or mem, n_c even or outside 1 .. 31, step_km
 * not finite or not positive with n_c > 1, radii that are not finite or not ordered, a first guess that is not finite or lies
 * beyond 89 degrees of latitude.
 *
 * Environment XSW_CENTRE_PATH = direct, read at every call (any other value is refused): every pixel meets every candidate in a
 * plain loop and sends each hit's five adds straight to global memory.  Unset (the default): the pixels near the lattice are
 * staged in LDS and every thread keeps its candidates' sums in registers.  Both give the same bits. */
int xsw_wind_centre(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t src_kind, const void *src, const uint8_t *keep,
                    int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon, const double *tie_lat, const double *tie_cos,
                    const double *tie_sin, const int32_t *line_first, const double *line_t, const int32_t *sample_first,
                    const double *sample_t, double lon_g, double lat_g, double cos_lat_g, double sin_lat_g, double step_km, int32_t n_c,
                    double r_in_km, double r_out_km, int64_t *sums);

/* ---- calibration: sigma0, NESZ, incidence and a validity mask from a product's digital numbers (xsarsea_amd.calibrate), the way
 * IN to device memory: 2 bytes per pixel and a few kilobytes of annotation instead of 4 bytes per pixel and raster.  Additive to
 * XSW_VERSION 4; conventions as above.
 *
 * A table is an annotation grid values[n_lines][n_samples] (float64) with the bracket of every raster line and sample between its
 * nodes, prepared by the caller exactly as for xsw_ancillary_model: i0 = line_first[l], i1 = min(i0 + 1, n_lines - 1), weights
 * wl = (1 - line_t[l], line_t[l]); j0, j1, ws likewise from sample_first / sample_t (indices are clamped into range, never
 * trusted).  Every table has its OWN brackets.  A NULL table pointer, or one whose `values` is NULL, means the table is absent.
 * Its value at pixel (l, s), every operation float64 and rounded once:
 *   f(l, s) = wl0 * (ws0 * f[i0][j0] + ws1 * f[i0][j1]) + wl1 * (ws0 * f[i1][j0] + ws1 * f[i1][j1])
 * (two nodes at neighbouring integer coordinates s, s + 1 therefore state a jump exactly: pixel s reads node s alone, pixel
 * s + 1 the next one).
 *
 * dn: the lines x samples digital numbers, uint16 (XSW_DN_U16) or float32 (XSW_DN_F32).  Per pixel, every operation float64 and
 * rounded once, in this order:
 *   1. A from sigma0_lut and, where given, Nr from noise_range, Na from noise_azimuth, inc from incidence, each by f above
 *   2. N = Nr * Na;  Nr or Na alone when only one is given;  0.0 when neither is
 *   3. d = (double)dn,  q = d * d,  g = 1.0 / (A * A)
 *   4. nesz = N * g,  sigma0 = (q - N) * g          (one division per pixel; DN**2 / A**2 - N / A**2 in xsar's words)
 *   5. use_fill != 0 and dn == fill (uint16: as integers, fill a whole number in 0 .. 65535; float32: compared as float32
 *      against (float)fill):  sigma0 = NaN;  nesz and incidence are still written
 *   6. valid = 1 iff the pixel is not fill and sigma0 > 0, else 0   (uint8)
 *   7. sigma0, nesz, incidence rounded once to out_dtype (XSW_F32 or XSW_F64)
 * Every output pointer may be NULL: it is not computed and never written; out_incidence needs the incidence table.
 * dn == NULL with the incidence table alone and out_incidence alone is the table at every pixel (any annotation grid: incidence,
 * elevation, ground heading).  Any other combination with dn == NULL, and dn without sigma0_lut, is XSW_EINVAL, as are a bad
 * dtype, mem or fill and a present table with a NULL bracket or an empty axis; a refused call writes no output.
 * One streaming pass (k_calibrate): 2 B (4 B) read per pixel, 4 B (8 B) written per float raster, the tables stay in cache. */
enum { XSW_DN_U16 = 0, XSW_DN_F32 = 1 };
typedef struct xsw_table {
    int32_t n_lines, n_samples;
    const double *values;        /* [n_lines][n_samples]; NULL: the table is absent */
    const int32_t *line_first;   /* [lines] */
    const double *line_t;        /* [lines] */
    const int32_t *sample_first; /* [samples] */
    const double *sample_t;      /* [samples] */
} xsw_table;
int xsw_calibrate(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t dn_dtype, int32_t out_dtype, const void *dn,
                  const xsw_table *sigma0_lut, const xsw_table *noise_range, const xsw_table *noise_azimuth, const xsw_table *incidence,
                  int32_t use_fill, double fill, void *out_sigma0, void *out_nesz, void *out_incidence, uint8_t *out_valid);

/* ---- sea / land keep mask from coastline edges (xsarsea_amd.landmask): the one byte raster of the chain that comes from
 * geography, made where the others are, from a few thousand edges and the scene's tie points.  Additive to XSW_VERSION 4;
 * conventions as above.
 *
 * out: uint8 lines x samples, 1 = water (keep), 0 = land; invert = 1 swaps them; and_with (nullable, uint8 of the same shape; a
 * non-zero byte counts as 1) is AND-ed in after the inversion.  The tie grids and the brackets are those of xsw_ancillary_model
 * (tie_cos / tie_sin are not needed).  edges: float64 [n_edges][4] = x1, y1, x2, y2 in degrees, longitudes continuous with the
 * tie longitudes (the caller adds the whole turns); n_edges = 0 (edges may be NULL) gives all water.
 *
 * Per pixel (l, s): (lon, lat) by step 1 of xsw_ancillary_model for f = lon, lat alone (the same device code, csrc/xsw_tie.hpp);
 * px = lon, py = lat.  Per edge, every operation float64 and rounded once:
 *   s    = (y1 > py) != (y2 > py)                       half-open in latitude: a vertex belongs to the edge above it
 *   xmin = min(x1, x2), xmax = max(x1, x2)
 *   east = px < xmin
 *   a = (px - x1) * (y2 - y1),  b = (py - y1) * (x2 - x1)
 *   mid  = !east && px <= xmax && (y2 > y1 ? a < b : a > b)
 *   hit  = s && (east || mid)
 *   land = parity of the number of hits over all edges
 * The two x-range clauses belong to the definition: an edge wholly west of the pixel never counts and one wholly east of it
 * always does, whatever a and b round to, so skipping the one and counting the other unseen are exact.  An edge with y1 == y2
 * never counts.  No division and no library call: tests/landmask_ref.py restates it in numpy and asks for equal bytes.
 *
 * Bands (n_bands >= 1): band_start [n_bands + 1] ascending from >= 0 to <= n_list, band_edges [n_list] with entries in
 * [0, n_edges): the edges a pixel of band clamp(floor((lat - lat0) / h), 0, n_bands - 1) is tested against, h finite and > 0.
 * The list of a band must hold every edge that can hit a pixel the kernel puts into it (the index may be off by one through
 * rounding, so a caller lists an edge one band beyond its latitude range on either side) and be ordered by descending xmax: the
 * walk stops at the first edge with xmax < px.  A band is never part of the result; a list that is too long costs time only.
 * n_bands = 0 (band_start, band_edges NULL): every pixel against every edge, the direct kernel.  Environment XSW_LAND_PATH =
 * direct | bands (default bands), read at every call (any other value is refused): `direct` ignores the bands of the call.
 * With XSW_MEM_HOST the band arrays are checked (XSW_EINVAL for a descending band_start or an entry outside the edges); with
 * XSW_MEM_DEVICE they cannot be read here, and the kernel clamps every index into range, as it always does.
 * XSW_EINVAL also for a bad mem or invert, n_edges < 0, n_bands outside 0 .. 65536; a refused call writes nothing.
 * lines == 0 or samples == 0 is XSW_OK and launches nothing.  1 B written per pixel (and 1 B read with and_with); the time goes
 * into the edge walk and the float64 geolocation. */
int xsw_land_mask(xsw_ctx *ctx, int64_t lines, int64_t samples, int32_t mem, int32_t n_tie_lines, int32_t n_tie_samples, const double *tie_lon,
                  const double *tie_lat, const int32_t *line_first, const double *line_t, const int32_t *sample_first, const double *sample_t,
                  int32_t n_edges, const double *edges, int32_t n_bands, const int32_t *band_start, int32_t n_list, const int32_t *band_edges,
                  double lat0, double h, const uint8_t *and_with, int32_t invert, uint8_t *out);
/* Edges of one staging chunk of the two kernels (a band with more of them is staged in several rounds). */
int32_t xsw_land_chunk_edges(void);

#ifdef __cplusplus
}
#endif
#endif /* XSW_H */
