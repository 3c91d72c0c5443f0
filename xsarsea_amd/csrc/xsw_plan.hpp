// The host side's pure arithmetic: the layout of a launch's work lists, the plan that cuts a raster into chunks, the strip grid
// of the line-block kernels.  No HIP type or call in here, so a host compiler builds it alone (tests/test_host_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>

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
