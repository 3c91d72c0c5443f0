// The cross-pol step of a dual-pol inversion on its own (xsw.h: xsw_cross_from_codes): k_cross_from_codes takes the co-pol
// answer as the 4-byte grid codes xsw_invert wrote (out_code_co) and runs windspeed.py:252-278 and the select :426-428 for
// every pixel -- what the fused kernels do after their co-pol search, without the search.  A change on the cross-pol side
// (another GMF, another dsig_cr) then costs this kernel, not the co-pol search again.
//
// One pixel per lane, 16 B read per pixel (code, incidence, sigma0_cr, dsig_cr as float32 rasters), 4 B (or a complex)
// written.  Everything the cross-pol step needs of the co-pol search is in the code and the context's tables: whether it ran
// (XSW_CODE_NAN: it did not), whether the pixel was an early NaN (XSW_CODE_NAN_RE: incidence or ancillary wind NaN),
// |wind_co| (abs_co[flat]) and its direction (dual_dir[sign][flat]).  The searches are those of invert_strip (xsw_device.hpp),
// selected by the same conditions, so the winning index is the reference's first arg-min on every route; the winds are formed
// in store_pixel's operation order, the co-pol wind a select picks is read from `sol` (what k_expand reads).
//
// A code that is no code of the context's co-pol LUT (bit 31 set and not one of the two NaN codes, or a flat index at or
// beyond n_wspd * n_phi: codes of another LUT, stale memory) reads no table: the pixel is handled as XSW_CODE_NAN_RE.
#pragma once
#include "xsw_device.hpp"  // DevTables, to_db, nearest_index, the search_cr_* and exact_scan_cr of invert_strip, Cx
#include "xsw_host.hpp"    // CrossArgs

namespace xsw {

// 64 VGPRs = 8 waves per SIMD: nothing of a co-pol search is alive here (the fused dual-pol k_invert_band holds 7).
template <typename T, typename TO>
__global__ __launch_bounds__(256, 8) void k_cross_from_codes(DevTables L, CrossArgs A)
{
    const double nan = __builtin_nan("");
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i - lane >= A.n) return;  // wave-uniform: the cooperative scan below needs whole waves
    const bool in = i < A.n;
    const long long il = in ? i : A.n - 1;

    // ---- load_pixel's cross-pol half (windspeed.py:198-209, :252-254), the co-pol half replaced by the code
    const double inc = ld<T>(A.inc, il);
    const CoCode code = co_decode(A.code_co ? A.code_co[il] : XSW_CODE_NAN, (unsigned)(L.n_w * L.n_phi));
    const T x = ((const T *)A.s_cr)[il];
    const double s_cr = to_db(x, A.is_db);
    const double dsig = dsig_cr_at<T>(A.dsig_cr, il, x, A.dsig_cr_scalar);
    const bool grid = code.grid();
    const bool early = inc != inc || (code.code != XSW_CODE_NAN && !grid);  // XSW_CODE_NAN_RE, or no code of this LUT
    const bool have_co = !early && grid;
    const bool need = in && !early && s_cr == s_cr && dsig == dsig;
    int i_inc_cr = 0;
    if (need) i_inc_cr = nearest_index(L.inc_cr, L.n_inc_cr, inc, L.inc_cr_uniform != 0, L.inc_cr0, L.inv_inccrstep);
    const double aco = have_co ? L.abs_co[code.flat()] : nan;  // np.abs(wind_co)

    // ---- the search of invert_strip (windspeed.py:255-269): one pixel per lane, the undecided ones cooperatively
    int icr = 0;
    bool undecided = need;
    {
        bool done = false;
        if (L.cr_monotone && L.inv_cr) done = search_cr_scan(L, need, i_inc_cr, s_cr, dsig, have_co, aco, icr, undecided);
        else if (L.cr_monotone) done = search_cr_interval(L, need, i_inc_cr, s_cr, dsig, have_co, aco, icr, undecided);
        if (!done) search_cr_lanes(L, need, i_inc_cr, s_cr, dsig, have_co, aco, icr, undecided);
    }
    unsigned long long und = __ballot(undecided);
    while (und) {
        const int p = __ffsll((long long)und) - 1;
        und &= und - 1;
        const int k = exact_scan_cr(L, rd_lane_i(i_inc_cr, p), rd_lane_d(s_cr, p), rd_lane_d(dsig, p), rd_lane_i((int)have_co, p) != 0,
                                    rd_lane_d(aco, p), lane);
        if (lane == p) icr = k;
    }
    if (!in) return;

    // ---- store_pixel's cross-pol half (windspeed.py:269-278, select :426-428)
    const size_t k_co = (size_t)code.k();  // [sign][i_wspd][i_phi] of dual_dir and sol
    double cr_re = nan, cr_im = early ? 0.0 : nan;
    if (need) {
        const double wd = L.wcr[icr];
        if (have_co) {
            const double2 u = ((const double2 *)L.dual_dir)[k_co];
            cr_re = wd * u.x;
            cr_im = wd * u.y + 0.0 * u.x;
        } else {
            cr_re = wd; cr_im = 0.0;  // exp(1j*0)
        }
    }
    bool picked_co = false;
    if (A.dual_select) {
        bool dual_small = false;
        if (need) {
            const double wd = L.wcr[icr];
            dual_small = wd < 5.0 - 1e-9 ? true : (wd > 5.0 + 1e-9 ? false : hypot_glibc(cr_re, cr_im) < 5.0);
        }
        if (aco < 5.0 || dual_small) {  // (aco is NaN without a co-pol wind: never < 5)
            picked_co = true;
            cr_re = nan; cr_im = nan;  // wind_co of a cross-only pixel (dual_small alone picked it)
            if (have_co) { const double2 z = ((const double2 *)L.sol)[k_co]; cr_re = z.x; cr_im = z.y; }
        }
    }
    if (A.out_cr) {
        typedef typename Cx<TO>::type cx_t;
        cx_t z; z.x = (TO)cr_re; z.y = (TO)cr_im;
        ((cx_t *)A.out_cr)[i] = z;
    }
    if (A.code_cr) A.code_cr[i] = early ? XSW_CODE_NAN_RE : cr_encode(need ? (unsigned)icr : XSW_CODE_NO_INDEX, picked_co);
}

}  // namespace xsw
