// The table offsets a pixel's slot carries through k_invert_band's passes (BandSlot, xsw_band.hpp): one statement of their packing
// for stage 1 (band_wave forms them once per pixel), the pass (co_band_pass adds a direction and loads) and the host
// (tests/band_slot_c builds a stand-alone program from this header).  Plain integer code.
//
//   slice0      byte offset of the pixel's incidence slice in the co-pol table L.co ([n_inc][n_w][phi_pad] doubles)
//   inv0, inv1  byte offsets of two rows of the inverse-row table L.inv_rows ([n_inc][XSW_INV_BINS][phi_pad], 2 bytes each):
//               the row of the largest threshold <= s - d and the row of the smallest threshold > s + d
//   inv1 == kBandInvNone: the grid has no threshold above s + d (the band may reach the window's last row).  A real offset is
//               even, the reserved value is odd: they cannot collide.
//
// All three are 32-bit: the band kernels run only on tables below 4 GB (LutGeometry::inv_ok, DevTables::co_off32) whose row
// numbers fit 24 bits (DevTables::band_mul24: n_inc * n_w, (n_inc + 1) * XSW_INV_BINS and phi_pad * 8 stay below 2^24), so every
// product below is one full-rate 24-bit multiply on the device.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XSW_BANDSLOT_HD __host__ __device__ __forceinline__
#else
#define XSW_BANDSLOT_HD inline
#endif
#ifndef XSW_INV_BINS
#define XSW_INV_BINS 2048  // thresholds per slice of the inverse-row table (xsw_lutplan.hpp)
#endif

namespace xsw {

constexpr unsigned kBandInvNone = 0xFFFFFFFFu;

// uniform * v, both below 2^24 (device: v_mul_u32_u24 with the wave-uniform factor in an SGPR, as mul24_sv of xsw_device.hpp)
XSW_BANDSLOT_HD unsigned band_mul24_uv(unsigned uniform, unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "s"(uniform), "v"(v));
    return r;
#else
    return (uniform & 0xFFFFFFu) * (v & 0xFFFFFFu);
#endif
}

// Row `bin` (0 .. XSW_INV_BINS; XSW_INV_BINS itself names no row: band_inv1 maps it to the reserved value) of slice i_inc of
// the inverse-row table, as an offset in ELEMENTS -- the product stage 1 also reads its run length through.
XSW_BANDSLOT_HD unsigned band_inv_elems(unsigned phi_pad, unsigned i_inc, unsigned bin)
{
    return band_mul24_uv(phi_pad, i_inc * (unsigned)XSW_INV_BINS + bin);
}
XSW_BANDSLOT_HD unsigned band_inv0(unsigned elems_lo) { return elems_lo * 2u; }
XSW_BANDSLOT_HD unsigned band_inv1(unsigned elems_hi, int bin_hi) { return bin_hi < XSW_INV_BINS ? elems_hi * 2u : kBandInvNone; }
XSW_BANDSLOT_HD unsigned band_slice0(unsigned phi_pad, unsigned n_w, unsigned i_inc) { return band_mul24_uv(phi_pad * 8u, band_mul24_uv(n_w, i_inc)); }

// The pass's side: is there a row above the band, and where to read it -- without one, the lower row's address (harmless: the
// lane loads it anyway, and the value is not used).
XSW_BANDSLOT_HD bool band_inv1_capped(unsigned inv1) { return inv1 != kBandInvNone; }
XSW_BANDSLOT_HD unsigned band_inv1_row(unsigned inv0, unsigned inv1) { return inv1 != kBandInvNone ? inv1 : inv0; }

}  // namespace xsw
