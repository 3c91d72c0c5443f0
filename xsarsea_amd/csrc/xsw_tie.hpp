// The scene's geolocation at a raster coordinate, from its tie-point grid: steps 1-2 of xsw_ancillary_model (include/xsw.h),
// stated once for the kernels that need them (k_ancillary_model per pixel, k_cells per cell centre).  Every operation is float64
// and rounded once, in the order written here; tests/ancillary_model_ref.py restates it.
//   f    = wl0 * (ws0 * f[i0][j0] + ws1 * f[i0][j1]) + wl1 * (ws0 * f[i1][j0] + ws1 * f[i1][j1])   for f = lon, lat, cos, sin
//   n    = hypot(cos, sin), ch = cos / n, sh = sin / n       (n == 0, the headings cancel: 0 / 0 = NaN)
#pragma once
#include <hip/hip_runtime.h>

#include "xsw_device.hpp"

namespace {

// One tie-grid field blended along the sample axis at the two tie lines of a line bracket.
struct TieRows {
    double lon0, lon1, lat0, lat1, c0, c1, s0, s1;
};

__device__ inline double along(const double *__restrict__ f, int i, int j0, int j1, int ns, double ws0, double ws1)
{
    return ws0 * f[(long long)i * ns + j0] + ws1 * f[(long long)i * ns + j1];
}

// The four fields at tie lines i0, i1 between tie columns j0, j1 (indices already clamped into the [.., ns] grids).
__device__ inline TieRows tie_rows(const double *__restrict__ tlon, const double *__restrict__ tlat, const double *__restrict__ tcos,
                                   const double *__restrict__ tsin, int i0, int i1, int j0, int j1, int ns, double ws0, double ws1)
{
    TieRows q;
    q.lon0 = along(tlon, i0, j0, j1, ns, ws0, ws1); q.lon1 = along(tlon, i1, j0, j1, ns, ws0, ws1);
    q.lat0 = along(tlat, i0, j0, j1, ns, ws0, ws1); q.lat1 = along(tlat, i1, j0, j1, ns, ws0, ws1);
    q.c0 = along(tcos, i0, j0, j1, ns, ws0, ws1); q.c1 = along(tcos, i1, j0, j1, ns, ws0, ws1);
    q.s0 = along(tsin, i0, j0, j1, ns, ws0, ws1); q.s1 = along(tsin, i1, j0, j1, ns, ws0, ws1);
    return q;
}

// Longitude, latitude and the renormalised heading vector (ch, sh) at line weights (wl0, wl1).
struct TiePoint {
    double lon, lat, ch, sh;
};

__device__ inline TiePoint tie_point(const TieRows &q, double wl0, double wl1)
{
    TiePoint p;
    p.lon = wl0 * q.lon0 + wl1 * q.lon1;
    p.lat = wl0 * q.lat0 + wl1 * q.lat1;
    const double c = wl0 * q.c0 + wl1 * q.c1, s = wl0 * q.s0 + wl1 * q.s1;
    const double nh = xsw::hypot_glibc(c, s);
    p.ch = c / nh;  // nh == 0 (the headings cancel): 0 / 0
    p.sh = s / nh;
    return p;
}

// Longitude and latitude alone (step 1 of xsw_ancillary_model restricted to its first two fields; xsw_land_mask): the same
// products and sums in the same order as tie_rows + tie_point, no hypot and no division.
struct TieLonLat {
    double lon, lat;
};

__device__ inline TieLonLat tie_lonlat(const double *__restrict__ tlon, const double *__restrict__ tlat, int i0, int i1, int j0, int j1, int ns,
                                       double ws0, double ws1, double wl0, double wl1)
{
    TieLonLat p;
    p.lon = wl0 * along(tlon, i0, j0, j1, ns, ws0, ws1) + wl1 * along(tlon, i1, j0, j1, ns, ws0, ws1);
    p.lat = wl0 * along(tlat, i0, j0, j1, ns, ws0, ws1) + wl1 * along(tlat, i1, j0, j1, ns, ws0, ws1);
    return p;
}

}  // namespace
