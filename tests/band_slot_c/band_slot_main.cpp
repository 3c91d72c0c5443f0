// Stand-alone host program around csrc/xsw_bandslot.hpp (tests/test_band_slot_cpu.py builds it with the host compiler and
// compares it with the plain 64-bit formulas).  Arguments: quintuples "phi_pad n_w i_inc bin bin_hi".  For every quintuple it
// writes six uint32 to stdout: slice0, inv0, inv1 as stage 1 packs them into the slot, then what the pass makes of inv1 --
// 1 / 0: there is a row above the band, the offset it reads that row at -- and the reserved value itself.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xsw_bandslot.hpp"

int main(int argc, char **argv)
{
    if (argc < 6 || (argc - 1) % 5 != 0) {
        std::fprintf(stderr, "usage: %s phi_pad n_w i_inc bin bin_hi [...]\n", argv[0]);
        return 2;
    }
    std::vector<uint32_t> out;
    for (int a = 1; a + 4 < argc; a += 5) {
        const unsigned phi_pad = (unsigned)std::strtoul(argv[a], nullptr, 10), n_w = (unsigned)std::strtoul(argv[a + 1], nullptr, 10);
        const unsigned i_inc = (unsigned)std::strtoul(argv[a + 2], nullptr, 10), bin = (unsigned)std::strtoul(argv[a + 3], nullptr, 10);
        const int bin_hi = std::atoi(argv[a + 4]);
        const unsigned lo = xsw::band_inv_elems(phi_pad, i_inc, bin), hi = xsw::band_inv_elems(phi_pad, i_inc, (unsigned)bin_hi);
        const unsigned inv0 = xsw::band_inv0(lo), inv1 = xsw::band_inv1(hi, bin_hi);
        out.push_back(xsw::band_slice0(phi_pad, n_w, i_inc));
        out.push_back(inv0);
        out.push_back(inv1);
        out.push_back(xsw::band_inv1_capped(inv1) ? 1u : 0u);
        out.push_back(xsw::band_inv1_row(inv0, inv1));
        out.push_back(xsw::kBandInvNone);
    }
    return std::fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
