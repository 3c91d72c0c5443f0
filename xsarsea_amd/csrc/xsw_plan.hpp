// The host side's pure arithmetic: the layout of a launch's work lists, the plan that cuts a raster into chunks, the strip grid
// of the line-block kernels, the route of an inversion launch.  No HIP type or call in here, so a host compiler builds it alone
// (tests/test_host_plan.py, tests/test_host_route_plan.py).
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>

// Work lists of one launch, side by side in one allocation: [0..15] counters, then list G (k_invert_list) of list_cap entries,
// list B (k_invert_band2) of XSW_LIST_B_SHARE times as many and list C (k_invert_blocks) of XSW_LIST_C_SHARE times as
// many: on the scenes whose a-priori wind is far from the sigma0 contour HALF the pixels are k_invert_band2's (an overflowing
// list B sends the rest through the strip mask, where stage 1 is redone for them).  With list_cap = an eighth of the raster the
// lists take 4.5 B and list B's records 24 B per pixel of the largest raster seen.
#ifndef XSW_LIST_B_SHARE
#define XSW_LIST_B_SHARE 4
#endif
#ifndef XSW_LIST_C_SHARE
#define XSW_LIST_C_SHARE 4
#endif
#define XSW_LISTS_TOTAL (1 + XSW_LIST_B_SHARE + XSW_LIST_C_SHARE)
#define XSW_REC_BYTES 48  // sizeof(BandRec) (xsw_band.hpp; static_assert in xsw_invert_tu.hip)

static inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// [16 counters | list G | list B | list C | pad to 256 B | mask G, mask B: mask_strips words each | list B's records].
// `base` is the allocation (nullptr: no lists, the one-kernel path); everything a launch needs is carved from it here and
// nowhere else.  The padding keeps the masks and the records 16-byte aligned whatever list_cap is.
struct WorkLists {
    enum List { G = 0, B = 1, C = 2 };
    unsigned *base = nullptr;
    size_t list_cap = 0;     // entries of list G
    size_t mask_strips = 0;  // 64-bit words of each strip mask (one per strip of 64 samples)

    static size_t share(List l) { return l == G ? 1 : l == B ? XSW_LIST_B_SHARE : XSW_LIST_C_SHARE; }
    static size_t lists_bytes(size_t cap) { return pad256((XSW_LISTS_TOTAL * cap + 16) * sizeof(unsigned)); }
    size_t bytes() const  // of the whole allocation
    {
        return lists_bytes(list_cap) + 2 * mask_strips * sizeof(unsigned long long) + (size_t)XSW_LIST_B_SHARE * list_cap * XSW_REC_BYTES;
    }

    unsigned *count(List l) const { return base + l; }  // side by side: count(G) .. count(C) are one reset, one read
    unsigned *entries(List l) const { return base + 16 + (l == G ? 0 : l == B ? 1 : 1 + XSW_LIST_B_SHARE) * list_cap; }
    unsigned cap(List l) const { return (unsigned)std::min<size_t>(share(l) * list_cap, 0xfffffff0u); }
    // the masks of a raster of nstrips <= mask_strips strips: masks() and masks() + nstrips, side by side (one reset)
    unsigned long long *masks() const { return (unsigned long long *)((char *)base + lists_bytes(list_cap)); }
    void *records() const { return masks() + 2 * mask_strips; }  // XSW_LIST_B_SHARE * list_cap of XSW_REC_BYTES
};

// strips of 64 samples a raster of n pixels in `lines` lines can have, however it is cut (as given, or into lines of 4096)
static inline size_t strips_for(long long n, long long lines) { return (size_t)(n / 64 + std::max<long long>(lines, n / 4096) + 64); }

// Capacity of list G.  The context's list (device rasters): an eighth of the raster's pixels (the benchmark scene leaves
// 0.06 %; a scene that leaves more than an eighth overflows it, see k_invert_list), or `test_cap` when that is set
// (XSW_LIST_CAP_TEST), rounded up to even.  A worker's list (one chunk of at most max_px pixels) has a smaller floor and no
// test override.
static inline size_t context_list_cap(long long n, long long test_cap)
{
    return ((size_t)(test_cap ? test_cap : std::max<long long>(n / 8, 1 << 16)) + 1) & ~(size_t)1;
}
static inline size_t worker_list_cap(size_t max_px) { return std::max<size_t>(max_px / 8, 1 << 14) & ~(size_t)1; }

// How a raster of lines x samples pixels is cut into the chunks that are launched one by one.
//   recut_flat: a flat raster (a long vector of pixels: the core dimension is only a loop, windspeed.py:190; 1-D inputs arrive
//     as one line) is re-cut into lines of 4096 samples + a tail chunk of one short line: pixels are independent, and whole
//     4-line tiles keep the workgroups full (a one-line raster leaves three of a workgroup's four waves idle).
//   cap_px: chunks of about n / 16 pixels, at least 1 << 16 and at most cap_px; 0: the whole (re-cut) raster is one chunk.
//   tile_rows: a chunk is whole rows of tiles this many lines high (1: any number of lines).
struct ChunkPlan {
    long long lines, samples;  // the raster as cut
    long long lines_per_chunk, nmain, tail_px, nchunks;
    size_t max_px;  // the largest chunk

    struct Chunk {
        size_t px0, npx;
        long long lines, samples;
    };

    ChunkPlan(long long lines_in, long long samples_in, long long cap_px, long long tile_rows, bool recut_flat)
        : lines(lines_in), samples(samples_in), tail_px(0)
    {
        const long long n = lines * samples;
        if (recut_flat && lines < 16 && n >= (1LL << 16)) { samples = 4096; lines = n / samples; tail_px = n - lines * samples; }
        lines_per_chunk = lines;
        if (cap_px > 0) {
            const long long target_px = std::min<long long>(cap_px, std::max<long long>(1LL << 16, n / 16));
            lines_per_chunk = samples > 0 ? (target_px + samples - 1) / samples : lines;
            lines_per_chunk = (std::max(lines_per_chunk, tile_rows) + tile_rows - 1) / tile_rows * tile_rows;
        }
        nmain = (lines + lines_per_chunk - 1) / lines_per_chunk;
        nchunks = nmain + (tail_px ? 1 : 0);
        max_px = (size_t)std::max<long long>(std::min(lines_per_chunk, lines) * samples, tail_px);
    }

    Chunk chunk(long long k) const  // k in [0, nchunks); the last pixels of a re-cut flat raster come last, as one short line
    {
        if (k >= nmain) return Chunk{(size_t)(lines * samples), (size_t)tail_px, 1, tail_px};
        const long long l0 = k * lines_per_chunk, l1 = std::min(lines, l0 + lines_per_chunk);
        return Chunk{(size_t)(l0 * samples), (size_t)((l1 - l0) * samples), l1 - l0, samples};
    }
};

// Staging of one chunk of an inversion (the same offsets in a worker's page-locked and device buffer): the input rasters that
// travel, each padded to 256 B, then the grid codes that come back; [o_cc, o_end) is one download.  The worker's work lists
// follow at o_end in the device buffer.  es: bytes of an input element (anc: two per pixel).
struct ChunkStaging {
    size_t o_inc, o_co, o_cr, o_dsig, o_anc, o_cc, o_ccr, o_end;
    ChunkStaging(size_t max_px, size_t es, bool inc, bool co, bool cr, bool dsig, bool anc, bool code_co, bool code_cr)
    {
        size_t o = 0;
        auto take = [&o](bool on, size_t bytes) { const size_t at = o; if (on) o += pad256(bytes); return at; };
        o_inc = take(inc, max_px * es); o_co = take(co, max_px * es); o_cr = take(cr, max_px * es);
        o_dsig = take(dsig, max_px * es); o_anc = take(anc, max_px * es * 2);
        o_cc = take(code_co, max_px * 4); o_ccr = take(code_cr, max_px * 4);
        o_end = o;
    }
};

// The grid of k_detrend and its like for a raster of rows x cols units: about wg_per_cu workgroups per CU, each a strip of
// 256 columns by a block of rows.
struct Strips {
    long long gx, gy, rows_per_block;
};
static inline Strips strip_grid(long long rows, long long cols, long long wg_per_cu = 16)
{
    Strips s;
    s.gx = (cols + 255) / 256;
    s.gy = (256LL * wg_per_cu + s.gx - 1) / s.gx;
    s.gy = std::max<long long>(1, std::min<long long>(std::min<long long>(s.gy, rows), 65535));
    s.rows_per_block = (rows + s.gy - 1) / s.gy;
    s.gy = (rows + s.rows_per_block - 1) / s.rows_per_block;
    return s;
}

// ---- The route of one inversion launch (launch_invert, xsw_invert_tu.hip): which kernels run, with which hand-over thresholds
// and on which grids.  RouteKnobs: the environment switches; RouteFacts: what the installed tables and the call are; ChainPlan:
// everything that follows from the two.  Results never depend on the route.
#ifndef XSW_B2_AREA
#define XSW_B2_AREA 2048  // measured with list C at half the raster (profiles/sweep_b2_area.sh, Mpx/s at 1e6 / 8192 / 4096 / 2048 / 1024 / 512): outliers 5 % 727 / 2486 / 2675 / 2711 / 2624 / 2694, a-priori x 0.3 424 / 440 / 512 / 591 / 643 / 620, x 2.5 460 / 459 / 480 / 520 / 508 / 489, x 0.6 1148 / 1147 / 1161 / 1176 / 1128 / 910
#endif
// list B (k_invert_band -> k_invert_band2): a pixel whose band holds XSW_LONG_RUN (5) or more rows along the a-priori direction
// is handed to k_invert_band2 -- one such pixel holds up every pixel of its pass in k_invert_band, and where the a-priori wind is
// far from the sigma0 contour most pixels are such.  XSW_LONG_RUN=0: never (k_invert_band sweeps every window: A/B
// measurements); the statistics instantiation sweeps every window in k_invert_band as well.
// (5 since round 5: with the stage-1 live arc and the cheaper k_invert_band2 re-measured on the hard scenes, 4 / 5 / 6 / 8 rows: cyclone band
// 7669 / 8052 / 7971 / 7489 Mpx/s, outliers 5 % 3640 / 3885 / 3955 / 3860, a-priori x 0.6 1925 / 2073 / 2081 / 1908, x 1.6 1586 / 1610 /
// 1571 / 1480, inc 17-33 x 1.6 979 / 1009 / 1030 / 990; the 20000 x 20000 benchmark scene 37.31 / 37.44 / 37.77 ms: within its noise for 4 / 5)
#ifndef XSW_LONG_RUN_DEFAULT
#define XSW_LONG_RUN_DEFAULT 5
#endif
#ifndef XSW_ARC_MIN
#define XSW_ARC_MIN 32    // directions from which a window is narrowed to its live arc in stage 1 of k_invert_band (environment XSW_ARC_MIN; 0: never).  48 / 40 / 32 / 24 at 48 pixels per wave: a-priori x 1.6 1651 / 1663 / 1711 / 1736 Mpx/s, inc 17-33 x 1.6 1012 / 1059 / 1081 / 1071, cyclone band 7816 / 7885 / 7865 / 7637
#endif
#ifndef XSW_ARC_CROWD
#define XSW_ARC_CROWD 48  // ... when this many of the wave's 64 pixels are such (environment XSW_ARC_CROWD)
#endif
#ifndef XSW_B2_CROWD
#define XSW_B2_CROWD 24  // pixels beyond XSW_B2_AREA a wave of k_invert_band must hold (of 64) for them to stay k_invert_band2's (environment XSW_B2_CROWD; 65: never)
#endif
#ifndef XSW_B2_WIDE
#define XSW_B2_WIDE 0  // directions from which a window is k_invert_band2's whatever its run (0: never)
#endif
#ifndef XSW_B2_REFINE_MIN
#define XSW_B2_REFINE_MIN 16  // records marked for the refinement a wave of k_invert_band2 must hold to run it (environment XSW_B2_REFINE_MIN)
#endif
#ifndef XSW_B2_ROWS_MAX
#define XSW_B2_ROWS_MAX 4096  // rows (candidates) the live arc may hold after step B: beyond, the pixel is k_invert_blocks's (environment XSW_B2_ROWS_MAX)
#endif
#ifndef XSW_TAIL_SWEEP
#define XSW_TAIL_SWEEP 256  // rows past the monotone ones a window may hold for k_invert_band2's tail sweep (KArgs::tail_max; 0: off;
                            // environment XSW_TAIL_SWEEP).  Measured (Mpx/s, 0 / 96 / 192 / 400 rows): a-priori x 1.6 1107 / 1186 / 1193 / 1191,
                            // x 2.5 252 / 331 / 394 / 396, incidence 17..33 deg x 1.6 421 / 473 / 570 / 560, 17..25 deg 2460 / 2654 / 2612 / 2651
#endif
#ifndef XSW_BLOCK_MIN
#define XSW_BLOCK_MIN 1024
#endif

// Environment knobs (experiments, A/B measurements, the tests' forced routes).  env_int: the variable's integer clamped to
// [lo, hi], or dflt when it is unset.
static inline long long env_int(const char *name, long long dflt, long long lo = LLONG_MIN, long long hi = LLONG_MAX)
{
    const char *v = getenv(name);
    return v ? std::min(std::max(atoll(v), lo), hi) : dflt;
}
static inline bool env_flag(const char *name) { return getenv(name) != nullptr; }

// Every switch that shapes an inversion (INTEGRATION.md has the table).  A process reads them once: route_knobs(), xsw_host.hpp.
struct RouteKnobs {
    int block_min = XSW_BLOCK_MIN;       // windows of at least this many candidates: block pyramid (general kernel)
    bool no_band = false;                // experiments / A-B measurements only
    int long_run = XSW_LONG_RUN_DEFAULT;
    bool no_records = false;             // A/B measurements and the tests of the index-list route
    bool no_blocks_kernel = false;       // list C's pixels stay on list G, i.e. with k_invert_list (A/B measurements and the tests of that route)
    int b2_area = XSW_B2_AREA, b2_crowd = XSW_B2_CROWD /* (65: never) */, b2_wide = XSW_B2_WIDE;
    int arc_min = XSW_ARC_MIN, arc_crowd = XSW_ARC_CROWD;
    int b2_refine_min = XSW_B2_REFINE_MIN, b2_rows_max = XSW_B2_ROWS_MAX, tail_sweep = XSW_TAIL_SWEEP;
    bool no_strip_masks = false;         // A/B measurements and the tests of the old route
    long long list_cap_test = 0;         // ensure_list (xsw.hip); tests: a tiny capacity, so that the overflow route runs
    bool fail_list_alloc = false;        // ensure_list; tests: the allocation-failure route

    static RouteKnobs from_env()
    {
        RouteKnobs k;
        k.block_min = (int)env_int("XSW_BLOCK_MIN", XSW_BLOCK_MIN, 0);
        k.no_band = env_flag("XSW_NO_BAND");
        k.long_run = (int)env_int("XSW_LONG_RUN", XSW_LONG_RUN_DEFAULT, 0);
        k.no_records = env_flag("XSW_NO_RECORDS");
        k.no_blocks_kernel = env_flag("XSW_NO_BLOCKS_KERNEL");
        k.b2_area = (int)env_int("XSW_B2_AREA", XSW_B2_AREA, 1);
        k.b2_crowd = (int)env_int("XSW_B2_CROWD", XSW_B2_CROWD, 1);
        k.b2_wide = (int)env_int("XSW_B2_WIDE", XSW_B2_WIDE, 0);
        k.arc_min = (int)env_int("XSW_ARC_MIN", XSW_ARC_MIN);
        k.arc_crowd = (int)env_int("XSW_ARC_CROWD", XSW_ARC_CROWD, 1);
        k.b2_refine_min = (int)env_int("XSW_B2_REFINE_MIN", XSW_B2_REFINE_MIN, 0);
        k.b2_rows_max = (int)env_int("XSW_B2_ROWS_MAX", XSW_B2_ROWS_MAX, 1);
        k.tail_sweep = (int)env_int("XSW_TAIL_SWEEP", XSW_TAIL_SWEEP, 0, 30000);
        k.no_strip_masks = env_flag("XSW_NO_STRIP_MASKS");
        k.list_cap_test = env_int("XSW_LIST_CAP_TEST", 0, 16);
        k.fail_list_alloc = env_flag("XSW_FAIL_LIST_ALLOC");
        return k;
    }
};

// What the route decision reads: of the installed tables (DevTables) and of the call (KArgs, LaunchCtl); route_facts(),
// xsw_host.hpp, fills it.
struct RouteFacts {
    enum Algo { PRUNED = 1, EXHAUSTIVE = 2, EXACT = 3, EXHAUSTIVE_F64 = 4 };  // XSW_ALGO_* of xsw.h (static_assert in xsw_host.hpp)
    // tables
    bool prunable, co_off32, band_mul24, cr_monotone, blk_span_ok;
    bool mono_rows, inv_rows, blk, csphi32, tail_min;  // the table is there
    int n_w, n_phi;
    // call
    long long lines, samples, n;
    int algo;         // resolved: never XSW_ALGO_AUTO
    bool s_co, s_cr;  // the raster is given
    bool mono;        // no cross-pol raster in or out
    bool stats, stats_chain;
    bool lists;               // the launch has work lists
    size_t mask_strips;       // ... and their strip masks hold this many words each
};

// The kernels' own compile-time figures (xsw_band.hpp, xsw_blocks.hpp): XSW_BAND_WG_WAVES, XSW_BAND2_WAVES, XSW_BLOCKS_WAVES;
// band_cs_cap: directions k_invert_band's LDS copy of the cos / sin table holds (kBandCsCap; 0: the build has none).
struct ChainWaves {
    int band_wg, band2, blocks;
    int band_cs_cap = 0;
};

struct ChainPlan {
    enum Route { EXHAUSTIVE, CHAIN, ONE_PRUNED, ONE_EXACT, TOO_LARGE };
    enum Limit { NONE, NBLOCKS, BAND_GROUPS, BAND_COLS };  // TOO_LARGE: the grid dimension that does not fit one launch
    Route route;
    Limit limit = NONE;
    long long nblocks;  // k_invert grid: 8 XCD lanes x ceil(columns/8) tile columns x line groups (see the kernel)
    int block_min;      // KArgs::block_min of the branch-and-bound routes
    // ---- CHAIN only.  Two-kernel fast path: k_invert_band finishes every pixel the band rule decides (monotone LUT rows, finite
    // inputs, unique minimum; cross-pol by the interval rule) and appends the rest to a work list; k_invert_list inverts those
    // (all tiles, should the list overflow).
    bool count_inst = false;  // the statistics instantiation: k_invert_band sweeps every window itself and counts
    bool band2 = false;       // k_invert_band2 runs (list B)
    bool records = false;     // ... on list B's records (BandRec), not on pixel indices
    bool blocks3 = false;     // k_invert_blocks runs (list C: the finite pixels the band rule is not for)
    bool cs_lds = false;      // k_invert_band's passes read cos / sin from the workgroup's LDS copy of the table (it holds the LUT's directions)
    bool masks = false;       // strip masks: what the consumers walk when a list overflows (only the marked pixels instead of the whole raster)
    size_t nstrips = 0;       // 64-bit words of each mask for this raster
    // the KArgs thresholds of the same names
    int long_run = 0, area_max = 0, b2_crowd = 0, area_crowd_max = 0, wide_min = 0, arc_min = 0, arc_crowd = 0, b2_refine_min = 0,
        b2_rows_max = 0, tail_max = 0;
    // grids.  k_invert_band: x = XCD lane + 8 * line group, y = tile column inside the XCD's range (see the kernel); the others
    // walk their lists with a capped number of workgroups
    unsigned band_grid_x = 0, band_grid_y = 0, band2_blocks = 0, blocks3_blocks = 0, list_blocks = 0;

    ChainPlan(const RouteKnobs &k, const RouteFacts &f, const ChainWaves &w) : block_min(k.block_min)
    {
        const long long strips_per_line = (f.samples + 63) / 64, line_groups = (f.lines + 3) / 4;
        nblocks = 8 * ((strips_per_line + 7) / 8) * line_groups;
        if (nblocks > 0x7fffffffLL) { route = TOO_LARGE; limit = NBLOCKS; return; }
        if (f.algo == RouteFacts::EXHAUSTIVE || f.algo == RouteFacts::EXHAUSTIVE_F64) { route = EXHAUSTIVE; return; }
        if (!(f.algo == RouteFacts::PRUNED && !k.no_band && f.lists && f.s_co && f.prunable && f.mono_rows && f.inv_rows && f.co_off32 &&
              f.band_mul24 && (!f.s_cr || f.cr_monotone) && f.n < (1LL << 32))) {
            route = f.algo == RouteFacts::PRUNED ? ONE_PRUNED : ONE_EXACT;
            return;
        }
        const long long cols_per_xcd = (strips_per_line + 7) / 8;
        const long long band_groups = (f.lines + w.band_wg - 1) / w.band_wg;
        if (8 * band_groups > 0x7fffffffLL) { route = TOO_LARGE; limit = BAND_GROUPS; return; }
        if (cols_per_xcd > 65535) { route = TOO_LARGE; limit = BAND_COLS; return; }
        route = CHAIN;
        count_inst = f.stats && !f.stats_chain;
        band2 = k.long_run > 0 && !count_inst;
        records = band2 && !k.no_records;
        cs_lds = f.n_phi >= 1 && f.n_phi <= w.band_cs_cap;  // (more directions: the instantiation that reads global memory)
        blocks3 = f.blk && f.blk_span_ok && !k.no_blocks_kernel && f.n_w < 32768 && f.n_phi < 32768;
        long_run = k.long_run;
        area_max = f.blk ? k.b2_area : 0x7fffffff;  // (without the block tables the general kernel has nothing better to offer)
        b2_crowd = k.b2_crowd;
        area_crowd_max = 1 << 20;
        wide_min = k.b2_wide > 0 ? k.b2_wide : 0x7fffffff;
        arc_min = (k.arc_min > 0 && f.csphi32) ? k.arc_min : 0x7fffffff;
        arc_crowd = k.arc_crowd;
        b2_refine_min = k.b2_refine_min;
        b2_rows_max = k.b2_rows_max;
        tail_max = (band2 && f.tail_min) ? k.tail_sweep : 0;  // (the tail rows are k_invert_band2's to sweep)
        nstrips = (size_t)(strips_per_line * f.lines);
        masks = nstrips <= f.mask_strips && !k.no_strip_masks;
        band_grid_x = (unsigned)(8 * band_groups);
        band_grid_y = (unsigned)cols_per_xcd;
        band2_blocks = (unsigned)std::min<long long>(nblocks, 256 * w.band2);  // XSW_BAND2_WAVES waves per SIMD, 4-wave workgroups
        blocks3_blocks = (unsigned)std::min<long long>(nblocks, 256 * w.blocks);
        list_blocks = (unsigned)std::min<long long>(nblocks, 256 * 8);  // 8 waves per SIMD
    }
};
