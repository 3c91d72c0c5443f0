// Stand-alone host program around csrc/xsw_tilewalk.hpp (tests/test_tile_walk_cpu.py builds it with the host compiler and
// compares it with tests/tile_walk_ref.py).  Arguments: pairs "strips line_groups".  For every pair it writes the whole map to
// stdout as int32 pairs (tile column, line group), (-1, -1) for a slot without a tile, in the order xcd, y, g (g fastest) --
// once through tile_walk and once more through tile_walk_linear, in the order of the linear slot number b.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xsw_tilewalk.hpp"

int main(int argc, char **argv)
{
    if (argc < 3 || (argc - 1) % 2 != 0) {
        std::fprintf(stderr, "usage: %s strips line_groups [strips line_groups ...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 1 < argc; a += 2) {
        const long long strips = std::atoll(argv[a]), lg = std::atoll(argv[a + 1]);
        if (strips < 1 || lg < 1) return 2;
        const long long C = (strips + 7) / 8;
        std::vector<int32_t> out((size_t)(8 * C * lg * 2));
        size_t k = 0;
        for (long long xcd = 0; xcd < 8; ++xcd)
            for (long long y = 0; y < C; ++y)
                for (long long g = 0; g < lg; ++g) {
                    long long col = 0, group = 0;
                    const bool ok = xsw::tile_walk(strips, lg, xcd, y, g, col, group);
                    out[k++] = ok ? (int32_t)col : -1;
                    out[k++] = ok ? (int32_t)group : -1;
                }
        if (std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size()) return 1;
        k = 0;
        for (long long b = 0; b < 8 * C * lg; ++b) {
            long long col = 0, group = 0;
            const bool ok = xsw::tile_walk_linear(strips, lg, b, col, group);
            out[k++] = ok ? (int32_t)col : -1;
            out[k++] = ok ? (int32_t)group : -1;
        }
        if (std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size()) return 1;
    }
    return 0;
}
