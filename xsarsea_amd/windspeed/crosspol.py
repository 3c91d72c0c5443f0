"""The dual-pol inversion in two steps: the co-pol search once, kept as 4-byte grid codes (`invert_copol_codes` ->
`CopolCodes`), then the cross-pol step (reference: windspeed/windspeed.py:252-278, select :426-428) as often as wanted --
another cross-pol GMF, another `dsig_cr` -- each time one pass of `xsw_cross_from_codes` instead of the whole inversion.

    cc = invert_copol_codes(inc, sigma0_vv, ancillary_wind=anc, model="gmf_cmod5n")
    wind_co = cc.wind()                                            # == invert_from_model(inc, sigma0_vv, ...) mono
    wind_dual = cc.dual(sigma0_vh, dsig_cr=dsig, model="gmf_s1_v2")  # == invert_from_model(inc, vv, vh, ...)[1]

numpy rasters (numpy out) and device rasters (torch CUDA tensors / `__cuda_array_interface__`; torch out, asynchronous on
torch's current stream) only: xarray / dask containers are not handled here.  The bit equality with the fused call holds for
cross-pol rasters of the co-pol rasters' dtype; a `sigma0_dual` / `dsig_cr` whose dtype would change how the fused call computes
its co-pol step (float32 rasters next to float64 ones: another kernel dtype or dB route, hence other co-pol codes for a few
pixels) is refused with `ValueError`.
"""
import numpy as np

from .. import _device
from . import _engine, _plan
from . import windspeed as _ws
from .models import get_model


def _refuse_containers(what, *arrays):
    for v in arrays:
        if v is not None and (_ws._is_xr(v) or _ws._is_dask(v)):
            raise TypeError(f"{what} takes numpy or device arrays only: xarray / dask containers are not supported here "
                            "(use invert_from_model, or pass `.values`)")


def _meta(a):
    """(shape, numpy dtype) of a numpy or device raster without touching the device, None for an absent one."""
    if a is None:
        return None
    if not _device.is_device_array(a):
        return _plan.meta(a)
    if hasattr(a, "is_cuda"):  # a torch tensor
        return _device.meta(a)
    cai = a.__cuda_array_interface__
    return tuple(cai["shape"]), np.dtype(cai["typestr"])


class CopolCodes:
    """The co-pol answer of `invert_copol_codes`: `codes` (uint32 numpy array, or int32 torch tensor holding the same bits:
    include/xsw.h, out_code_co), the incidence raster and the co-pol LUT they belong to.  sigma0_meta / ancillary_meta:
    (shape, dtype) of the co-pol call's sigma0 and ancillary wind (they decide, with the cross-pol rasters, the dtype the
    fused dual-pol call would compute in); by default those of a call whose rasters all have the incidence's dtype."""

    def __init__(self, inc, codes, lut_co, sigma0_meta=None, ancillary_meta=None):
        self.inc, self.codes, self.lut_co = inc, codes, lut_co
        self.on_device = _device.is_device_array(codes)
        self.shape = tuple(codes.shape)
        self.inc_meta = _meta(inc)
        self.sigma0_meta = sigma0_meta if sigma0_meta is not None else (self.shape, self.inc_meta[1])
        self.ancillary_meta = ancillary_meta

    def wind(self):
        """The co-pol wind: what `invert_from_model(inc, sigma0, ancillary_wind=..., model=co)` returns, bit for bit."""
        if self.on_device:
            return _engine.expand_device(self.lut_co, self.codes)
        return _engine.expand_codes(self.lut_co, None, self.codes, None)[0]

    def dual(self, sigma0_dual, dsig_cr=0.1, model=None, dual_select=True, codes=False, **kwargs):
        """`wind_dual`, the second element of `invert_from_model(inc, sigma0, sigma0_dual, model=(co, model), dsig_cr=...)`, bit
        for bit, from the stored co-pol codes.  model: the cross-pol model; **kwargs go to its `to_lut`.  dual_select=False:
        the cross-pol wind before the select of windspeed.py:426-428.  codes=True: the cross-pol grid codes instead
        (include/xsw.h, out_code_cr; the select, when asked for, is the kernel's and sets XSW_CODE_PICK_CO).  ValueError for a
        shape, container or dtype mismatch with the co-pol call (module docstring), before any device call."""
        scalar = np.isscalar(dsig_cr)
        _refuse_containers("CopolCodes.dual", sigma0_dual, None if scalar else dsig_cr)
        if sigma0_dual is None:
            raise ValueError("sigma0_dual is missing")
        for name, v in (("sigma0_dual", sigma0_dual), ("dsig_cr", None if scalar else dsig_cr)):
            if v is not None and _device.is_device_array(v) != self.on_device:
                raise ValueError(f"{name} is a {'device' if not self.on_device else 'host'} array but the co-pol codes are in "
                                 f"{'device' if self.on_device else 'host'} memory: one container kind per CopolCodes")
        plan = _engine.cross_plan(self.shape, self.inc_meta, self.sigma0_meta, self.ancillary_meta, _meta(sigma0_dual),
                                  dsig_cr if scalar else _meta(dsig_cr), device=self.on_device, dual_select=dual_select)
        mono = _plan.CallPlan(self.inc_meta, self.sigma0_meta, None, None, self.ancillary_meta, device=self.on_device)
        if (mono.dtype, mono.db_by) != (plan.dtype, plan.db_by):
            raise ValueError(f"the dtypes of sigma0_dual / dsig_cr would make the fused dual-pol call compute its co-pol step in "
                             f"{np.dtype(plan.dtype).name} with sigma0 in dB by {plan.db_by}, but the stored codes were computed in "
                             f"{np.dtype(mono.dtype).name} with dB by {mono.db_by}: pass cross-pol rasters of the co-pol rasters' dtype")
        m = get_model(model)
        if not m.iscrosspol:
            raise ValueError(f"model {m.name} ({m.pol}) is not a cross-pol model")
        lut_cr = _engine.lut_source(m, kwargs)
        if self.on_device:  # the select fused into the kernel, as `invert_device` does
            return _engine.cross_device(self.lut_co, lut_cr, plan, self.codes, self.inc, sigma0_dual, dsig_cr, dual_select=dual_select, codes=codes)
        if codes:
            return _engine.cross_numpy(self.lut_co, lut_cr, plan, self.codes, self.inc, sigma0_dual, dsig_cr, dual_select=dual_select)
        # numpy rasters: codes over PCIe, expanded on the host, the select with numpy's own abs (as `invert_from_model` does)
        codes_cr = _engine.cross_numpy(self.lut_co, lut_cr, plan, self.codes, self.inc, sigma0_dual, dsig_cr)
        ws_co, ws_cr = _engine.expand_codes(self.lut_co, lut_cr, self.codes, codes_cr)
        return _engine.dual_select(ws_co, ws_cr) if dual_select else ws_cr


def invert_copol_codes(inc, sigma0, /, ancillary_wind=None, dsig_co=0.1, model=None, **kwargs):
    """The co-pol inversion of `invert_from_model(inc, sigma0, ancillary_wind=..., dsig_co=..., model=...)` kept as grid codes:
    a `CopolCodes`, whose `wind()` is that call's return value and whose `dual(sigma0_dual, ...)` runs the cross-pol step of
    the dual-pol inversion from the codes.  numpy rasters give a numpy uint32 array; device rasters an int32 torch tensor on
    the same device, asynchronously on torch's current stream.  **kwargs go to `Model.to_lut`."""
    tile_any_valid = kwargs.pop("_xsw_tile", None)  # private, as in invert_from_model: the ancillary-wind precondition answered by the caller
    _refuse_containers("invert_copol_codes", inc, sigma0, ancillary_wind)
    m = get_model(model)
    if not m.iscopol:
        raise ValueError(f"model {m.name} ({m.pol}) is not a co-pol model")
    assert ancillary_wind is not None and (_ws._valid(ancillary_wind) if tile_any_valid is None else tile_any_valid), \
        "co-pol inversion needs a valid ancillary wind"
    lut_co = _engine.lut_source(m, kwargs)
    if _device.any_device_array(inc, sigma0, ancillary_wind):
        codes, _ = _engine.invert_device(lut_co, None, inc, sigma0, None, None, ancillary_wind, dsig_co=dsig_co, codes=True)
        if not _device.is_device_array(inc):  # (a host incidence next to device rasters: the cross-pol step reads it in HBM)
            inc = _device.as_tensor(inc, codes.device)
    else:
        inc, sigma0, ancillary_wind = np.asarray(inc), np.asarray(sigma0), np.asarray(ancillary_wind)
        codes, _ = _engine.invert_numpy(lut_co, None, inc, sigma0, None, None, ancillary_wind, dsig_co=dsig_co, codes=True)
    return CopolCodes(inc, codes, lut_co, sigma0_meta=_meta(sigma0), ancillary_meta=_meta(ancillary_wind))
