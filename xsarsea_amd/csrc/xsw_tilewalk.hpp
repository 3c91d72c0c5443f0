// The inversion kernels' tile walk: which raster tile (tile column, line group) a workgroup takes.  One statement of it for
// k_invert_band, k_invert, k_invert_list's two overflow walks and the two exhaustive kernels; plain integer code that a host
// compiler takes as well (tests/tile_walk_c builds a stand-alone program from it).
//
// A raster of `strips` tile columns (64 samples each) and `lg` line groups is walked by 8 * C * lg workgroup slots,
// C = ceil(strips / 8): slot (xcd, y, g) with xcd in [0, 8), y in [0, C), g in [0, lg).  Workgroups are dealt to the 8 XCDs
// round-robin, so `xcd` is the XCD a slot lands on -- observed placement, used for speed only: the map below is a bijection
// onto the strips * lg tiles whatever XCD runs a slot.
//
// With base = strips / 8 and R = strips % 8:
//   * y < base: tile column xcd * base + y, line group g.  Every XCD owns a contiguous block of `base` columns and walks it
//     line groups fastest, so the waves resident on one XCD work in the same few LUT slices and its L2 keeps them.
//   * y == base (there only when R > 0): the R * lg tiles of the leftover columns [8 * base, strips), numbered
//     t = (column - 8 * base) * lg + line group, are cut into eight contiguous shares of q = ceil(R * lg / 8).  XCD `xcd`
//     takes t = xcd * q + g for g < q and t < R * lg; the other slots of the row have no tile.
// No XCD takes more than base * lg + q tiles (the leftover columns used to be the first R XCDs' alone: lg tiles each).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XSW_TILEWALK_HD __host__ __device__
#else
#define XSW_TILEWALK_HD
#endif

namespace xsw {

// Slot (xcd, y, g) -> its tile (col, group); false: the slot has no tile (col and group are then not to be used).  All the
// arguments are workgroup-uniform in the kernels, and so is everything computed here: the scalar unit's work.
XSW_TILEWALK_HD inline bool tile_walk(long long strips, long long lg, long long xcd, long long y, long long g, long long &col,
                                      long long &group)
{
    const long long base = strips >> 3, rem = strips & 7;
    col = xcd * base + y;
    group = g;
    if (y < base) return true;
    if (y > base || rem == 0) return false;
    const long long left = rem * lg, q = (left + 7) >> 3;
    long long t = xcd * q + g;
    if (g >= q || t >= left) return false;
    col = 8 * base;
    while (t >= lg) {  // t / lg < rem: at most 6 steps, no division
        t -= lg;
        ++col;
    }
    group = t;
    return true;
}

// The same for a linear slot number b in [0, 8 * C * lg) (k_invert's grid and the grid-stride walks): xcd = b % 8 as the
// workgroups are dealt, then tile-column slots outer, line groups inner.
XSW_TILEWALK_HD inline bool tile_walk_linear(long long strips, long long lg, long long b, long long &col, long long &group)
{
    const long long j = b >> 3;
    return tile_walk(strips, lg, b & 7, j / lg, j % lg, col, group);
}

}  // namespace xsw
