// The search kernels of ONE (input dtype, output dtype) pair and their launch logic (-DXSW_PAIR=0..3; xsarsea_amd/_build.py
// compiles the four side by side and links them with xsw.hip into libxsw.so).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "xsw_host.hpp"
#include "xsw_band.hpp"
#include "xsw_band2.hpp"
#include "xsw_blocks.hpp"
#include "xsw_exhaustive.hpp"
#include "xsw_cross.hpp"
#include "xsw_cost.hpp"
#include "xsw_uncertainty.hpp"
#include "xsw_forward.hpp"
#include "xsw_solve.hpp"
#include "xsw_dirsolve.hpp"
#include "xsw_joint.hpp"
#include "xsw_uncertainty_joint.hpp"

using namespace xsw;

// f(std::true_type) for a dual-pol launch, f(std::false_type) for a mono one: the kernels' CR instantiation, chosen once
template <typename F>
static void with_pol(bool dual, F &&f)
{
    if (dual) f(std::true_type{});
    else f(std::false_type{});
}

// Every routing decision is ChainPlan's (xsw_plan.hpp: which kernels, which thresholds, which grids); here it is carried out.
template <typename T, typename TO>
static int launch_invert(xsw_ctx *c, const KArgs &A_in, int algo, const LaunchCtl &lc, std::string &err)
{
    const RouteFacts f = route_facts(c->T, A_in, algo, lc);
    const ChainPlan p(route_knobs(), f, ChainWaves{XSW_BAND_WG_WAVES, XSW_BAND2_WAVES, XSW_BLOCKS_WAVES, XSW_BAND_POOL ? kBandCsCap : 0});
    if (p.route == ChainPlan::TOO_LARGE) return seterr(err, XSW_EINVAL, "raster too large for one launch");
    if (p.route == ChainPlan::EXHAUSTIVE)
        return launch_exhaustive<T, TO>(c->T, A_in, lc.stream, algo == XSW_ALGO_EXHAUSTIVE) == hipSuccess
                   ? XSW_OK : seterr(err, XSW_EHIP, "exhaustive launch failed: %s", hipGetErrorString(hipGetLastError()));
    KArgs A = A_in;
    A.block_min = p.block_min;
    if (p.route == ChainPlan::CHAIN) {
        KArgs B = A;
        const WorkLists &wl = lc.lists;
        B.list_count = wl.count(WorkLists::G); B.list = wl.entries(WorkLists::G); B.list_cap = wl.cap(WorkLists::G);
        if (p.band2) { B.list_b_count = wl.count(WorkLists::B); B.list_b = wl.entries(WorkLists::B); B.list_b_cap = wl.cap(WorkLists::B); }
        static_assert(sizeof(BandRec) == XSW_REC_BYTES, "XSW_REC_BYTES (xsw_plan.hpp) is sizeof(BandRec)");
        B.rec_b = p.records ? wl.records() : nullptr;
        if (p.blocks3) { B.list_c_count = wl.count(WorkLists::C); B.list_c = wl.entries(WorkLists::C); B.list_c_cap = wl.cap(WorkLists::C); }
        B.long_run = p.long_run; B.area_max = p.area_max; B.b2_crowd = p.b2_crowd; B.area_crowd_max = p.area_crowd_max;
        B.wide_min = p.wide_min; B.arc_min = p.arc_min; B.arc_crowd = p.arc_crowd; B.b2_refine_min = p.b2_refine_min;
        B.b2_rows_max = p.b2_rows_max; B.tail_max = p.tail_max;
        if (p.masks) {
            B.mask_g = wl.masks(); B.mask_b = wl.masks() + p.nstrips;  // side by side: one reset (0.25 B per pixel)
            if (hipMemsetAsync(wl.masks(), 0, 2 * p.nstrips * sizeof(unsigned long long), lc.stream) != hipSuccess) return seterr(err, XSW_EHIP, "strip-mask reset failed");
        }
        if (hipMemsetAsync(wl.count(WorkLists::G), 0, 3 * sizeof(unsigned), lc.stream) != hipSuccess) return seterr(err, XSW_EHIP, "work-list reset failed");
        const dim3 band_grid(p.band_grid_x, p.band_grid_y), band_block(64 * XSW_BAND_WG_WAVES);
        with_pol(!f.mono, [&](auto cr) {
            constexpr bool CR = decltype(cr)::value;
            if (lc.timing) timing_mark(c);
            // (p.cs_lds: the LUT's directions fit k_invert_band's LDS copy of the cos / sin table)
            auto band = [&](auto lds) {
                constexpr bool CSLDS = decltype(lds)::value;
                if (p.count_inst) hipLaunchKernelGGL((k_invert_band<T, TO, CR, true, 0, CSLDS>), band_grid, band_block, 0, lc.stream, c->T, B);  // (counts the scored candidates)
                else if (p.band2) hipLaunchKernelGGL((k_invert_band<T, TO, CR, false, 1, CSLDS>), band_grid, band_block, 0, lc.stream, c->T, B);
                else hipLaunchKernelGGL((k_invert_band<T, TO, CR, false, 0, CSLDS>), band_grid, band_block, 0, lc.stream, c->T, B);
            };
#if XSW_BAND_POOL
            if (p.cs_lds) band(std::true_type{});
            else
#endif
                band(std::false_type{});
            if (lc.timing) timing_mark(c);
#if defined(XSW_BAND_PASS_STATS) || defined(XSW_BAND_DETOUR_STATS)
            B.stats = nullptr;  // counter builds: the statistics buffer holds k_invert_band's own counts (band_wave), nothing else
#endif
            if (p.band2) hipLaunchKernelGGL((k_invert_band2<T, TO, CR>), dim3(p.band2_blocks), band_block, 0, lc.stream, c->T, B);
            if (lc.timing) timing_mark(c);
            if (p.blocks3) hipLaunchKernelGGL((k_invert_blocks<T, TO, CR>), dim3(p.blocks3_blocks), dim3(256), 0, lc.stream, c->T, B);
            if (lc.timing) timing_mark(c);
            hipLaunchKernelGGL((k_invert_list<T, TO, CR>), dim3(p.list_blocks), dim3(256), 0, lc.stream, c->T, B);
            if (lc.timing) timing_mark(c);
        });
    } else if (p.route == ChainPlan::ONE_PRUNED) {
        with_pol(!f.mono, [&](auto cr) {
            hipLaunchKernelGGL((k_invert<T, TO, 1, decltype(cr)::value>), dim3((unsigned)p.nblocks), dim3(256), 0, lc.stream, c->T, A);
        });
    } else {
        hipLaunchKernelGGL((k_invert<T, TO, 3>), dim3((unsigned)p.nblocks), dim3(256), 0, lc.stream, c->T, A);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(err, XSW_EHIP, "launch failed: %s", hipGetErrorString(e));
    return XSW_OK;
}


#ifndef XSW_PAIR
#error "compile with -DXSW_PAIR=0..3"
#endif
#define XSW_PAIR_NAME_(k) xsw_pair_##k
#define XSW_PAIR_NAME(k) XSW_PAIR_NAME_(k)
using TIn = std::conditional_t<(XSW_PAIR & 2) != 0, double, float>;
using TOut = std::conditional_t<(XSW_PAIR & 1) != 0, double, float>;
const PairLaunch &XSW_PAIR_NAME(XSW_PAIR)()
{
    static const PairLaunch pair = {
        launch_invert<TIn, TOut>,
        [](xsw_ctx *c, const CrossArgs &A, hipStream_t s, std::string &e) { return launch_pixels(k_cross_from_codes<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const CostArgs &A, bool cr, hipStream_t s, std::string &e) { return launch_pixels(cr ? k_cost_cr<TIn, TOut> : k_cost_co<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const UncArgs &A, bool cr, hipStream_t s, std::string &e) { return launch_pixels(cr ? k_unc_cr<TIn, TOut> : k_unc_co<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const FwdArgs &A, bool cr, hipStream_t s, std::string &e) { return launch_pixels(cr ? k_lut_eval_cr<TIn, TOut> : k_lut_eval_co<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const SolveArgs &A, bool cr, hipStream_t s, std::string &e) { return launch_pixels(cr ? k_wspd_solve_cr<TIn, TOut> : k_wspd_solve_co<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const DirArgs &A, hipStream_t s, std::string &e) { return launch_pixels(k_dir_solve_co<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const JointArgs &A, hipStream_t s, std::string &e) { return launch_pixels(k_joint_from_codes<TIn, TOut>, c->T, A, A.n, s, e); },
        [](xsw_ctx *c, const UncJointArgs &A, hipStream_t s, std::string &e) { return launch_pixels(k_unc_joint<TIn, TOut>, c->T, A, A.n, s, e); }};
    return pair;
}
