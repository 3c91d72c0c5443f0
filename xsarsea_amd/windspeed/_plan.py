"""One `xsw_invert` call decided once, from metadata only: every argument is absent (None), a scalar, or a raster known by
(shape, dtype).  No tensor, no pointer: `_engine`'s numpy, device and coded paths materialise what `CallPlan` says."""
import numpy as np

from .. import _lib, options

DB_NUMPY, DB_TORCH, DB_KERNEL = "numpy", "torch", "kernel"  # who turns the linear sigma0 into dB
# what a call's `dsig_cr` becomes: nothing (the default 0.1), the scalar, the scalar rounded through float32, the raster
# `sigma0_cr * 0 + dsig_cr` formed from the LINEAR cross-pol sigma0 in its own dtype (windspeed.py:122-123), the caller's raster
DSIG_NONE, DSIG_SCALAR, DSIG_SCALAR_F32, DSIG_FILL, DSIG_RASTER = "none", "scalar", "scalar_f32", "fill", "raster"


def meta(a):
    """(shape, dtype) of a host raster, None for an absent one."""
    return None if a is None else (np.shape(a), np.asarray(a).dtype)


class CallPlan:
    """inc, sigma0_co, sigma0_cr, anc: None or (shape, dtype); dsig_cr: None, a scalar or (shape, dtype).  device: the rasters
    are in device memory (torch forms what the kernel cannot; `options.device_out_dtype` out), else numpy rasters (numpy forms
    it in the staging step; complex128 out).  coded: the host rasters of `invert_coded` (uploaded, not handed to `invert_host`)."""

    def __init__(self, inc, sigma0_co, sigma0_cr, dsig_cr, anc, *, device, coded=False, dual_select=False):
        scalar = dsig_cr is not None and np.isscalar(dsig_cr)
        rasters = [m for m in (inc, sigma0_co, sigma0_cr, None if scalar else dsig_cr) if m is not None]
        # the gufunc "(n),(n),(n),(n),(n)->(n),(n)" broadcasts its loop dimensions over ALL inputs (windspeed.py:307-322):
        # e.g. a 1-D incidence row with 2-D sigma0 gives (line, sample) outputs
        self.shape = tuple(np.broadcast_shapes(*(m[0] for m in rasters + ([] if anc is None else [anc]))))
        self.n = int(np.prod(self.shape, dtype=np.int64))
        self.lines, self.samples = _lib.lines_samples(self.shape)
        self.want_co, self.want_cr = sigma0_co is not None, sigma0_cr is not None
        # every real raster float32, the ancillary wind absent or complex64: the device reads them as such and widens in registers
        f32 = self.all_f32 = all(m[1] == np.float32 for m in rasters) and (anc is None or anc[1] == np.complex64)
        self.dtype, self.cdtype, self.code, self.item = (np.float32, np.complex64, _lib.XSW_F32, 4) if f32 else (np.float64, np.complex128, _lib.XSW_F64, 8)
        # the reference converts sigma0 to dB in sigma0's OWN dtype (windspeed.py:126-130) before anything is widened
        f32_sigma0 = any(m is not None and m[1] == np.float32 for m in (sigma0_co, sigma0_cr))
        if device:  # the kernel's fused conversion is that arithmetic unless a float32 sigma0 stands next to wider rasters
            self.db_by = DB_TORCH if (f32_sigma0 and not f32) else DB_KERNEL
        else:  # numpy's own float32 log10 is the only way to the reference's bits: "auto" keeps a float32 sigma0 on the host
            on_dev = options.db_on_device
            self.db_by = DB_KERNEL if (not f32_sigma0 if on_dev == "auto" else on_dev) else DB_NUMPY
        self.is_db = self.db_by != DB_KERNEL
        self.dsig_scalar, self.dsig_fill = 0.1, None
        if dsig_cr is None:
            self.dsig = DSIG_NONE
        elif not scalar:
            self.dsig = DSIG_RASTER
        elif not self.want_cr:  # no cross-pol search: never read (`invert_numpy` alone passes the scalar on as it is)
            self.dsig = DSIG_NONE if (device or coded) else DSIG_SCALAR
        elif self.is_db:  # the kernel derives the broadcast from linear sigma0; with dB rasters it is formed as the reference does
            self.dsig, self.dsig_fill = DSIG_FILL, dsig_cr
        else:
            self.dsig = DSIG_SCALAR_F32 if f32 else DSIG_SCALAR
        if self.dsig in (DSIG_SCALAR, DSIG_SCALAR_F32):
            self.dsig_scalar = float(np.float32(dsig_cr)) if self.dsig == DSIG_SCALAR_F32 else float(dsig_cr)
        self.out_dtype = np.complex64 if (device and options.device_out_dtype == "complex64") else np.complex128
        self.out_code, self.out_item = (_lib.XSW_F32, 8) if self.out_dtype == np.complex64 else (_lib.XSW_F64, 16)
        self.algo = _lib.algo_code(options.algo)
        self.fused_select = bool(dual_select and device and self.want_co and self.want_cr)


class ForwardPlan:
    """One `xsw_lut_eval` / `xsw_lut_eval_cr` call from metadata only: inc, wspd, phi (None for a cross-pol table) as (shape, dtype),
    all of one shape; `more`: further rasters of a call that reads four (`xsw_dir_solve`), None for an absent one.  Every raster
    float32: the kernel reads them as such and widens in registers; else everything is float64."""

    def __init__(self, inc, wspd, phi=None, *more):
        rasters = [m for m in (inc, wspd, phi) + more if m is not None]
        shapes = {tuple(m[0]) for m in rasters}
        if len(shapes) != 1:
            raise ValueError(f"inc, wspd and phi must have one shape, not {sorted(shapes)}")
        for m in rasters:
            if np.dtype(m[1]) not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise TypeError(f"rasters must be float32 or float64, not {np.dtype(m[1]).name}")
        self.shape = shapes.pop()
        self.n = int(np.prod(self.shape, dtype=np.int64))
        self.lines, self.samples = _lib.lines_samples(self.shape)
        f32 = all(np.dtype(m[1]) == np.float32 for m in rasters)
        self.dtype, self.code = (np.float32, _lib.XSW_F32) if f32 else (np.float64, _lib.XSW_F64)
