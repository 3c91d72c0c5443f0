// Host side of the one-launch raster entry points (xsw.hip, xsw_gradients.hip, xsw_streaks.hip): the argument checks they
// share (their launch grid, strip_grid, is xsw_plan.hpp's), and one call's buffers on the XSW_MEM_HOST and XSW_MEM_DEVICE routes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "xsw_host.hpp"

namespace {

// Host buffers of one call: uploaded to temporaries, the launch runs on the context's stream, outputs come back, all before
// the call returns.  Device buffers: the launch alone, asynchronous on the context's stream.  A buffer the caller left out
// has bytes == 0 and null pointers: its dev stays null on both routes.
struct Buf {
    const void *host_in;  // input: host pointer to upload (nullptr for outputs)
    void *host_out;       // output: host pointer to fill (nullptr for inputs)
    size_t bytes;
    void *dev = nullptr;
};
static inline Buf in_buf(const void *p, size_t bytes) { return {p, nullptr, p ? bytes : 0}; }  // nullable input
static inline Buf out_buf(void *p, size_t bytes) { return {nullptr, p, p ? bytes : 0}; }       // nullable output

// launch(b) queues the kernels on the context's stream.  It returns nothing, or an XSW_* code: with a non-zero one the
// message in c->err is the launch's own, and no output comes back.
template <size_t N, typename Launch>
static int launch_on(xsw_ctx *c, Buf (&b)[N], Launch &launch, const char *what)
{
    if constexpr (std::is_void_v<decltype(launch(b))>) launch(b);
    else if (const int rc = launch(b)) return rc;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? XSW_OK : fail(c, XSW_EHIP, "%s failed: %s", what, hipGetErrorString(e));
}

template <size_t N, typename Launch>
static int run(xsw_ctx *c, int32_t mem, Buf (&b)[N], Launch &&launch, const char *what)
{
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, XSW_EHIP, "%s: hipSetDevice failed", what);
    if (mem == XSW_MEM_DEVICE) {
        for (auto &x : b) x.dev = x.host_out ? x.host_out : (void *)x.host_in;
        return launch_on(c, b, launch, what);
    }
    CallTemps tmp(c->stream);
    for (auto &x : b)
        if (x.bytes) x.dev = tmp.alloc(x.bytes, x.host_in);
    int rc = tmp.ok() ? XSW_OK : tmp.refused ? fail(c, XSW_ENOMEM, "%s: hipMalloc failed (%s)", what, hipGetErrorString(tmp.err))
                                             : fail(c, XSW_EHIP, "%s: upload failed (%s)", what, hipGetErrorString(tmp.err));
    hipError_t e;
    if (!rc) rc = launch_on(c, b, launch, what);
    for (auto &x : b)
        if (!rc && x.host_out && x.bytes && (e = hipMemcpyAsync(x.host_out, x.dev, x.bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
            rc = fail(c, XSW_EHIP, "%s: download failed (%s)", what, hipGetErrorString(e));
    e = tmp.finish();  // the one synchronisation, also before freeing after a failure: queued work may still use the temporaries
    if (!rc && e != hipSuccess) rc = fail(c, XSW_EHIP, "%s: %s", what, hipGetErrorString(e));
    return rc;
}

static bool bad_mem(int32_t mem) { return mem != XSW_MEM_HOST && mem != XSW_MEM_DEVICE; }

// The refusals every one-pixel-per-lane raster entry opens with, in this order: shape, dtype pair, memory kind.
static int check_raster_call(xsw_ctx *c, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, int32_t mem)
{
    if (lines < 0 || samples < 0) return fail(c, XSW_EINVAL, "negative raster shape");
    if ((dtype != XSW_F32 && dtype != XSW_F64) || (out_dtype != XSW_F32 && out_dtype != XSW_F64))
        return fail(c, XSW_EINVAL, "dtype/out_dtype must be XSW_F32 or XSW_F64");
    if (bad_mem(mem)) return fail(c, XSW_EINVAL, "bad mem kind");
    return XSW_OK;
}

// The pixels of such a call and the bytes of an input element (es) and of a real output element (os); XSW_EINVAL for a raster
// beyond one launch of 256-pixel blocks (checked without forming an overflowing lines * samples).
static int pixel_count(xsw_ctx *c, const char *who, int64_t lines, int64_t samples, int32_t dtype, int32_t out_dtype, long long &n, size_t &es,
                       size_t &os)
{
    if (lines && samples > (int64_t)(0x7fffffffLL * 256) / lines) return fail(c, XSW_EINVAL, "%s: raster too large for one launch", who);
    n = (long long)lines * samples;
    es = dtype == XSW_F32 ? 4 : 8;
    os = out_dtype == XSW_F32 ? 4 : 8;
    return XSW_OK;
}

// The kernels index a raster's axes (and count windows) with int.
static bool fits_int(int64_t a, int64_t b = 0) { return a <= 0x7fffffffLL && b <= 0x7fffffffLL; }

// XSW_OK, or XSW_EINVAL with "<what>: raster too large" for a raster whose axes do not fit int.
static int check_dims(xsw_ctx *c, const char *what, int64_t lines, int64_t samples)
{
    return fits_int(lines, samples) ? XSW_OK : fail(c, XSW_EINVAL, "%s: raster too large", what);
}

// XSW_OK, or XSW_EINVAL when a 2-D grid of tiles has more rows than one launch takes.
static int check_grid(xsw_ctx *c, const char *what, const dim3 &grid)
{
    return grid.y <= 65535 ? XSW_OK : fail(c, XSW_EINVAL, "%s: raster too large for one launch", what);
}

}  // namespace
