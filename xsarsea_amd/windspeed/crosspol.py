"""The dual-pol inversion in two steps: the co-pol search once, kept as 4-byte grid codes (`invert_copol_codes` ->
`CopolCodes`), then the cross-pol step (reference: windspeed/windspeed.py:252-278, select :426-428) as often as wanted --
another cross-pol GMF, another `dsig_cr` -- each time one pass of `xsw_cross_from_codes` instead of the whole inversion.

    cc = invert_copol_codes(inc, sigma0_vv, ancillary_wind=anc, model="gmf_cmod5n")
    wind_co = cc.wind()                                            # == invert_from_model(inc, sigma0_vv, ...) mono
    wind_dual = cc.dual(sigma0_vh, dsig_cr=dsig, model="gmf_s1_v2")  # == invert_from_model(inc, vv, vh, ...)[1]
    fit = cc.cost(sigma0_vv, anc)                                  # InversionCost: J at the minimum, its terms, the residual
    bars = cc.uncertainty(sigma0_vv, anc)                          # InversionUncertainty: wspd_std, dir_std, corr, flag
    best = cc.joint(sigma0_vv, anc, sigma0_vh, dsig_cr=dsig, model="gmf_s1_v2")  # CopolCodes of ONE cost over VV, VH, a-priori
    bars = best.uncertainty_joint(sigma0_vv, anc, sigma0_vh, dsig_cr=dsig, model="gmf_s1_v2")  # JointUncertainty: + u_std, v_std, corr_uv

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


def _codes_meta(a):
    """`_meta` for grid codes: a torch tensor's integer dtype by its name (`_device.meta` knows the raster dtypes only)."""
    if _device.is_device_array(a) and hasattr(a, "is_cuda"):
        try:
            return tuple(a.shape), np.dtype(str(a.dtype).rpartition(".")[2])
        except TypeError:
            return tuple(a.shape), np.dtype(np.void)
    return _meta(a)


class InversionCost:
    """Result of `CopolCodes.cost` / `.cost_dual`: the value of the minimum the search found and what it is made of, one real
    raster each (numpy arrays, or torch tensors for device rasters): J = Jsig + Jwind (cross-pol without a co-pol wind:
    J = Jsig, Jwind NaN), Jsig = ((lut_db - sigma0_db) / dsig)^2, Jwind the distance to the a-priori wind, residual_db =
    lut_db - sigma0_db at the solution.  NaN where no search ran.  With parts=False only J is computed: the others are None."""

    def __init__(self, J, Jsig=None, Jwind=None, residual_db=None):
        self.J, self.Jsig, self.Jwind, self.residual_db = J, Jsig, Jwind, residual_db

    def __getitem__(self, name):
        return getattr(self, name)


class InversionUncertainty:
    """Result of `CopolCodes.uncertainty` / `.uncertainty_dual`: how well the solution is DETERMINED (where `InversionCost` says
    how well it fits), from the curvature of the cost around the stored grid point (posterior ~ exp(-J / 2): covariance = 2 H^-1,
    H by second differences on the LUT axes' own spacings).  wspd_std in m/s, dir_std in degrees, corr their correlation (both
    None for the cross-pol search, which has one axis), flag a uint8 raster of bits (`FLAGS`): 1 no solution, 2 the solution
    lies on a border of the wind-speed axis, 4 on a border of the direction axis, 8 interior but the stencil is not convex
    (also: a NaN sigma0 / a-priori next to a valid code).  Any flag: the real rasters are NaN there.  Borders are not wrapped
    (0..360 axes) or mirrored (0..180 axes: the folded cost is not symmetric about 0 / 180 deg because of |Im(ancillary)|), so
    a solution on a border has no estimate."""
    FLAGS = {"no_solution": 1, "wspd_border": 2, "phi_border": 4, "not_convex": 8}

    def __init__(self, wspd_std, dir_std=None, corr=None, flag=None):
        self.wspd_std, self.dir_std, self.corr, self.flag = wspd_std, dir_std, corr, flag

    def __getitem__(self, name):
        return getattr(self, name)


class JointInversion:
    """Result of `CopolCodes.joint(..., details=True)`: `codes`, the `CopolCodes` of the grid wind that minimises the joint cost
    J = Jwind_co + Jsig_co + Jsig_cr, and one real raster each (numpy arrays, or torch tensors for device
    rasters) for J and its three terms at that wind.  NaN where there is no joint solution; Jsig_cr alone is NaN (and J = Jwind +
    Jsig_co) where the pixel has no cross-pol information and keeps its co-pol answer."""

    def __init__(self, codes, J, Jwind, Jsig_co, Jsig_cr):
        self.codes, self.J, self.Jwind, self.Jsig_co, self.Jsig_cr = codes, J, Jwind, Jsig_co, Jsig_cr

    def __getitem__(self, name):
        return getattr(self, name)


class JointUncertainty:
    """Result of `CopolCodes.uncertainty_joint`: the error bars of the joint dual-pol wind, from the curvature of the cost that wind
    minimises, J = Jwind_co + Jsig_co + Jsig_cr, around the stored grid point.  wspd_std (m/s), dir_std
    (degrees) and corr as in `InversionUncertainty`; u_std, v_std (m/s) and corr_uv are the same covariance in the components of
    the complex wind `.wind()` returns (u its real, v its imaginary part: antenna convention), the form a merge or an assimilation
    reads.  One real raster each (numpy arrays, or torch tensors for device rasters) and flag, a uint8 raster of bits (`FLAGS`):
    1, 2, 4, 8 as in `InversionUncertainty` -- any of them: NaN in all six real rasters -- and 16, no cross-pol information
    (NaN sigma0_dual or dsig_cr): the joint inversion kept the co-pol answer there and the rasters hold the co-pol error bars,
    those of `.uncertainty`; 16 alone does not mean NaN."""
    FLAGS = {"no_solution": 1, "wspd_border": 2, "phi_border": 4, "not_convex": 8, "no_crosspol": 16}

    def __init__(self, wspd_std, dir_std, corr, u_std, v_std, corr_uv, flag):
        self.wspd_std, self.dir_std, self.corr, self.u_std, self.v_std, self.corr_uv, self.flag = wspd_std, dir_std, corr, u_std, v_std, corr_uv, flag

    def __getitem__(self, name):
        return getattr(self, name)


def _real_dtype(out_dtype):
    dt = np.dtype(np.float64 if out_dtype is None else out_dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"out_dtype must be float32 or float64, not {dt}")
    return dt.type


class CopolCodes:
    """The co-pol answer of `invert_copol_codes`: `codes` (uint32 numpy array, or int32 torch tensor holding the same bits:
    include/xsw.h, out_code_co), the incidence raster and the co-pol LUT they belong to.  sigma0_meta / ancillary_meta:
    (shape, dtype) of the co-pol call's sigma0 and ancillary wind (they decide, with the cross-pol rasters, the dtype the
    fused dual-pol call would compute in); by default those of a call whose rasters all have the incidence's dtype.  dsig_co:
    the co-pol call's, what `cost` divides by when it is given none (None: 0.1, the default of that call)."""

    def __init__(self, inc, codes, lut_co, sigma0_meta=None, ancillary_meta=None, dsig_co=None):
        self.inc, self.codes, self.lut_co, self.dsig_co = inc, codes, lut_co, dsig_co
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

    def cells(self, cell, *, tie_points=None, line=None, sample=None, keep=None):
        """`xsarsea_amd.wind_cells(self.wind(), cell, ...)` from the stored codes: the co-pol wind on the product grid of
        `cell = (cell_lines, cell_samples)` pixels per cell (`WindCells`).  The pass reads the 4-byte codes and expands nothing;
        the result equals that of the complex128 expansion bit for bit.  Arguments and refusals as `wind_cells`."""
        from .. import cells as _cells
        return _cells.codes_cells(self.codes, self.lut_co, cell, tie_points=tie_points, line=line, sample=sample, keep=keep)

    def grid(self, tie_points, *, lon, lat, line=None, sample=None, keep=None, into=None):
        """`xsarsea_amd.wind_grid(self.wind(), tie_points, lon=..., lat=..., ...)` from the stored codes: the co-pol wind binned
        on a regular longitude / latitude grid (`WindGrid`).  The pass reads the 4-byte codes and expands nothing; the result
        equals that of the complex128 expansion bit for bit.  Arguments and refusals as `wind_grid`."""
        from .. import grid as _grid
        return _grid.codes_grid(self.codes, self.lut_co, tie_points, lon=lon, lat=lat, line=line, sample=sample, keep=keep, into=into)

    def polar(self, tie_points, *, centre, radius, sectors, line=None, sample=None, keep=None, into=None):
        """`xsarsea_amd.wind_polar(self.wind(), tie_points, centre=..., radius=..., sectors=..., ...)` from the stored codes: the
        co-pol wind in rings and sectors around a centre (`WindPolar`).  The pass reads the 4-byte codes and expands nothing; the
        result equals that of the complex128 expansion bit for bit.  Arguments and refusals as `wind_polar`."""
        from .. import polar as _polar
        return _polar.codes_polar(self.codes, self.lut_co, tie_points, centre=centre, radius=radius, sectors=sectors, line=line, sample=sample,
                                  keep=keep, into=into)

    def centre_scores(self, tie_points, *, first_guess, step_km, n, annulus, line=None, sample=None, keep=None, into=None):
        """`xsarsea_amd.wind_centre_scores(self.wind(), tie_points, first_guess=..., step_km=..., n=..., annulus=..., ...)` from the
        stored codes: the annulus sums of the co-pol wind around every candidate centre of a lattice (`CentreScores`).  The pass
        reads the 4-byte codes and expands nothing; the result equals that of the complex128 expansion bit for bit.  Arguments
        and refusals as `wind_centre_scores`."""
        from .. import centre as _centre
        return _centre.codes_centre_scores(self.codes, self.lut_co, tie_points, first_guess=first_guess, step_km=step_km, n=n, annulus=annulus,
                                           line=line, sample=sample, keep=keep, into=into)

    def find_centre(self, tie_points, *, annulus, first_guess=None, steps_km=(8.0, 2.0, 0.5), n=9, criterion="vt", keep=None, line=None, sample=None,
                    min_coverage=0.9, rotation=None):
        """`xsarsea_amd.find_centre(self.wind(), tie_points, annulus=..., ...)` from the stored codes: the cyclone's centre, coarse
        to fine, with nothing expanded (`CentreFix`).  Arguments and refusals as `find_centre`."""
        from .. import centre as _centre
        return _centre.codes_find_centre(self.codes, self.lut_co, tie_points, first_guess=first_guess, steps_km=steps_km, n=n, annulus=annulus,
                                         criterion=criterion, keep=keep, line=line, sample=sample, min_coverage=min_coverage, rotation=rotation)

    def dual(self, sigma0_dual, dsig_cr=0.1, model=None, dual_select=True, codes=False, **kwargs):
        """`wind_dual`, the second element of `invert_from_model(inc, sigma0, sigma0_dual, model=(co, model), dsig_cr=...)`, bit
        for bit, from the stored co-pol codes.  model: the cross-pol model; **kwargs go to its `to_lut`.  dual_select=False:
        the cross-pol wind before the select of windspeed.py:426-428.  codes=True: the cross-pol grid codes instead
        (include/xsw.h, out_code_cr; the select, when asked for, is the kernel's and sets XSW_CODE_PICK_CO).  ValueError for a
        shape, container or dtype mismatch with the co-pol call (module docstring), before any device call."""
        plan, lut_cr = self._cross_step("CopolCodes.dual", sigma0_dual, dsig_cr, model, kwargs, dual_select=dual_select)
        run = lambda **kw: _engine.cross_from_codes(self.lut_co, lut_cr, plan, self.codes, self.inc, sigma0_dual, dsig_cr, **kw)
        if self.on_device or codes:  # device rasters: the select fused into the kernel, as `invert_device` does
            return run(dual_select=dual_select, codes=codes)
        # numpy rasters: codes over PCIe, expanded on the host, the select with numpy's own abs (as `invert_from_model` does)
        ws_co, ws_cr = _engine.expand_codes(self.lut_co, lut_cr, self.codes, run(codes=True))
        return _engine.dual_select(ws_co, ws_cr) if dual_select else ws_cr

    def _same_kind(self, **arrays):
        for name, v in arrays.items():
            if v is not None and _device.is_device_array(v) != self.on_device:
                raise ValueError(f"{name} is a {'device' if not self.on_device else 'host'} array but the co-pol codes are in "
                                 f"{'device' if self.on_device else 'host'} memory: one container kind per CopolCodes")

    def _cross_step(self, who, sigma0_dual, dsig_cr, model, kwargs, dual_select=False, **codes):
        """(plan, lut_cr) of a cross-pol step from these codes, after every refusal `dual` and `cost_dual` share (**codes:
        `cost_dual`'s codes_cr, held to the co-pol codes' shape and container kind); nothing here touches the device."""
        dsig = None if np.isscalar(dsig_cr) else dsig_cr
        _refuse_containers(who, sigma0_dual, *codes.values(), dsig)
        if any(v is None for v in (sigma0_dual, *codes.values())):
            raise ValueError(" and ".join(["sigma0_dual", *codes]) + (" are both needed" if codes else " is missing"))
        self._same_kind(sigma0_dual=sigma0_dual, **codes, dsig_cr=dsig)
        for name, v in codes.items():
            cm = _codes_meta(v)
            if np.dtype(cm[1]) not in (np.dtype(np.uint32), np.dtype(np.int32)):
                raise TypeError(f"{name} must be uint32 or int32 grid codes, not {np.dtype(cm[1]).name}")
            if tuple(cm[0]) != self.shape:
                raise ValueError(f"{name} has shape {tuple(cm[0])}, the co-pol codes have shape {self.shape}")
        plan = _engine.cross_plan(self.shape, self.inc_meta, self.sigma0_meta, self.ancillary_meta, _meta(sigma0_dual),
                                  dsig_cr if dsig is None else _meta(dsig), device=self.on_device, dual_select=dual_select)
        mono = _plan.CallPlan(self.inc_meta, self.sigma0_meta, None, None, self.ancillary_meta, device=self.on_device)
        if (mono.dtype, mono.db_by) != (plan.dtype, plan.db_by):
            raise ValueError(f"the dtypes of sigma0_dual / dsig_cr would make the fused dual-pol call compute its co-pol step in "
                             f"{np.dtype(plan.dtype).name} with sigma0 in dB by {plan.db_by}, but the stored codes were computed in "
                             f"{np.dtype(mono.dtype).name} with dB by {mono.db_by}: pass cross-pol rasters of the co-pol rasters' dtype")
        m = get_model(model)
        if not m.iscrosspol:
            raise ValueError(f"model {m.name} ({m.pol}) is not a cross-pol model")
        return plan, _engine.lut_source(m, kwargs)

    def _co_step(self, who, sigma0, ancillary_wind, dsig_co):
        """(plan, dsig_co) of a pass over the co-pol rasters from these codes, after every refusal `cost` and `uncertainty` share;
        nothing here touches the device."""
        _refuse_containers(who, sigma0, ancillary_wind)
        if sigma0 is None or ancillary_wind is None:
            raise ValueError("sigma0 and ancillary_wind are both needed: the rasters the co-pol codes were computed from")
        self._same_kind(sigma0=sigma0, ancillary_wind=ancillary_wind)
        for name, v, stored in (("sigma0", sigma0, self.sigma0_meta), ("ancillary_wind", ancillary_wind, self.ancillary_meta)):
            m = _meta(v)
            if stored is not None and (tuple(m[0]), np.dtype(m[1])) != (tuple(stored[0]), np.dtype(stored[1])):
                raise ValueError(f"{name} has shape {tuple(m[0])} and dtype {np.dtype(m[1]).name}, the co-pol codes were computed from shape "
                                 f"{tuple(stored[0])} and dtype {np.dtype(stored[1]).name}: the cost would not be the one the search minimised")
        try:
            plan = _plan.CallPlan(self.inc_meta, _meta(sigma0), None, None, _meta(ancillary_wind), device=self.on_device)
        except ValueError as exc:
            raise ValueError(f"sigma0 / ancillary_wind do not broadcast against the co-pol codes of shape {self.shape}: {exc}") from None
        if plan.shape != self.shape:
            raise ValueError(f"sigma0 / ancillary_wind broadcast to shape {plan.shape}, the co-pol codes have shape {self.shape}")
        if dsig_co is None:
            dsig_co = 0.1 if self.dsig_co is None else self.dsig_co
        if not np.isscalar(dsig_co) or not float(dsig_co) == float(dsig_co) or float(dsig_co) == 0.0:
            raise ValueError(f"dsig_co must be a scalar other than 0 and NaN, not {dsig_co!r}")
        return plan, float(dsig_co)

    def cost(self, sigma0, ancillary_wind, dsig_co=None, parts=True, out_dtype=None):
        """The cost the co-pol search minimised, at its minimum: `InversionCost` with J = Jwind + Jsig of windspeed.py:216-225 at
        the stored grid point (bit for bit the minimum of the reference's dense J_co), its two terms and residual_db = lut_db -
        sigma0_db.  sigma0 / ancillary_wind: the rasters `invert_copol_codes` was given (a raster of another shape or dtype is
        refused: the cost would not be the one the search minimised).  dsig_co=None: the co-pol call's (else 0.1).
        parts=False: J alone.  out_dtype: float64 (default) or float32.  ValueError / TypeError before any device call."""
        plan, dsig_co = self._co_step("CopolCodes.cost", sigma0, ancillary_wind, dsig_co)
        return InversionCost(*_engine.cost_from_codes(self.lut_co, plan, self.codes, self.inc, sigma0, ancillary_wind, dsig_co=dsig_co,
                                                      parts=parts, out_dtype=_real_dtype(out_dtype)))

    def uncertainty(self, sigma0, ancillary_wind, dsig_co=None, out_dtype=None):
        """The error bars of the co-pol wind: `InversionUncertainty` with wspd_std (m/s), dir_std (degrees), their correlation
        and a uint8 flag raster, from the second differences of J_co (windspeed.py:216-225) over the 3 x 3 grid points around the
        stored one (include/xsw.h: xsw_uncertainty_from_codes).  Arguments and refusals as `cost`.  A solution on the first or
        last index of an axis has no estimate (flag 2 / 4): a 0..360 direction axis is not wrapped, a 0..180 one not mirrored.
        On codes returned by `.joint` this is the curvature of the co-pol cost only, not of the cost those codes minimise:
        `.uncertainty_joint` gives the error bars of the joint wind."""
        plan, dsig_co = self._co_step("CopolCodes.uncertainty", sigma0, ancillary_wind, dsig_co)
        return InversionUncertainty(*_engine.uncertainty_from_codes(self.lut_co, plan, self.codes, self.inc, sigma0, ancillary_wind,
                                                                    dsig_co=dsig_co, out_dtype=_real_dtype(out_dtype)))

    def joint(self, sigma0, ancillary_wind, sigma0_dual, dsig_cr=0.1, model=None, dsig_co=None, details=False, out_dtype=None, **kwargs):
        """The joint dual-pol inversion: a new `CopolCodes`, on the same tables, of the grid wind that minimises ONE cost over
        both observations and the a-priori wind, J = Jwind_co + Jsig_co + Jsig_cr, where Jsig_cr reads the cross-pol table at the
        co-pol speed -- instead of the two-step answer of `.dual` and its hard switch at 5 m/s.  `.wind()`,
        `.cost` and `.uncertainty` work on the result (`.uncertainty`: the co-pol curvature only).  sigma0 / ancillary_wind: the
        rasters `invert_copol_codes` was given; sigma0_dual, dsig_cr (scalar or raster, e.g. `dsig_from_nesz`), model (the
        cross-pol one; **kwargs to its `to_lut`) as `.dual`.  These codes serve as the upper bound that confines the search: the
        answer does not depend on them, the cost of the pass does.  A pixel without cross-pol information (NaN sigma0_dual or
        dsig_cr) keeps its co-pol answer.  details=True: `JointInversion(codes, J, Jwind, Jsig_co, Jsig_cr)` with real rasters of
        out_dtype (float64, or float32).  The refusals of `.cost` and `.dual`, before any device call."""
        _, dsig_co = self._co_step("CopolCodes.joint", sigma0, ancillary_wind, dsig_co)
        _, lut_cr = self._cross_step("CopolCodes.joint", sigma0_dual, dsig_cr, model, kwargs)
        dsig = None if np.isscalar(dsig_cr) else dsig_cr
        plan = _engine.cross_plan(self.shape, self.inc_meta, _meta(sigma0), _meta(ancillary_wind), _meta(sigma0_dual),
                                  dsig_cr if dsig is None else _meta(dsig), device=self.on_device)
        out = _engine.joint_from_codes(self.lut_co, lut_cr, plan, self.codes, self.inc, sigma0, ancillary_wind, sigma0_dual, dsig_cr,
                                       dsig_co=dsig_co, details=details, out_dtype=_real_dtype(out_dtype))
        codes = CopolCodes(self.inc, out[0], self.lut_co, sigma0_meta=self.sigma0_meta, ancillary_meta=self.ancillary_meta, dsig_co=dsig_co)
        return JointInversion(codes, *out[1:]) if details else codes

    def uncertainty_joint(self, sigma0, ancillary_wind, sigma0_dual, dsig_cr=0.1, model=None, dsig_co=None, out_dtype=None, **kwargs):
        """The error bars of the joint dual-pol wind: `JointUncertainty(wspd_std, dir_std, corr, u_std, v_std, corr_uv, flag)` from
        the second differences of the JOINT cost J = Jwind_co + Jsig_co + Jsig_cr over the 3 x 3 grid points around the stored one
        (include/xsw.h: xsw_uncertainty_joint_from_codes), with the covariance also in the (u, v) components
        of `.wind()`.  Meant for the codes `.joint` returned, with the arguments it was given; any grid codes of the same tables
        do.  A pixel without cross-pol information (NaN sigma0_dual or dsig_cr) gets the co-pol error bars of `.uncertainty` and
        flag bit 16.  out_dtype: float64 (default) or float32.  The refusals of `.joint`, before any device call."""
        _, dsig_co = self._co_step("CopolCodes.uncertainty_joint", sigma0, ancillary_wind, dsig_co)
        _, lut_cr = self._cross_step("CopolCodes.uncertainty_joint", sigma0_dual, dsig_cr, model, kwargs)
        dsig = None if np.isscalar(dsig_cr) else dsig_cr
        plan = _engine.cross_plan(self.shape, self.inc_meta, _meta(sigma0), _meta(ancillary_wind), _meta(sigma0_dual),
                                  dsig_cr if dsig is None else _meta(dsig), device=self.on_device)
        return JointUncertainty(*_engine.uncertainty_joint_from_codes(self.lut_co, lut_cr, plan, self.codes, self.inc, sigma0, ancillary_wind,
                                                                      sigma0_dual, dsig_cr, dsig_co=dsig_co, out_dtype=_real_dtype(out_dtype)))

    def cost_dual(self, sigma0_dual, codes_cr, dsig_cr=0.1, model=None, parts=True, out_dtype=None, **kwargs):
        """The cost the cross-pol search of `.dual(sigma0_dual, dsig_cr=..., model=..., **kwargs)` minimised, at its minimum:
        `InversionCost` with J = Jsig_cr [+ Jwind_cr] of windspeed.py:257-264 (Jwind NaN and J = Jsig where there is no co-pol
        wind).  codes_cr: what `.dual(..., codes=True)` returned, with or without dual_select (the select does not enter the
        cost).  The same refusals as `.dual`, before any device call."""
        plan, lut_cr = self._cross_step("CopolCodes.cost_dual", sigma0_dual, dsig_cr, model, kwargs, codes_cr=codes_cr)
        return InversionCost(*_engine.cost_cr_from_codes(self.lut_co, lut_cr, plan, self.codes, codes_cr, self.inc, sigma0_dual, dsig_cr,
                                                         parts=parts, out_dtype=_real_dtype(out_dtype)))

    def uncertainty_dual(self, sigma0_dual, codes_cr, dsig_cr=0.1, model=None, out_dtype=None, **kwargs):
        """The error bar of the cross-pol wind speed of `.dual(sigma0_dual, dsig_cr=..., model=..., **kwargs)`:
        `InversionUncertainty(wspd_std, None, None, flag)` from the second difference of J_cr (windspeed.py:257-264) over the three
        speeds around the stored one.  codes_cr and the refusals as `cost_dual`; the select does not enter."""
        plan, lut_cr = self._cross_step("CopolCodes.uncertainty_dual", sigma0_dual, dsig_cr, model, kwargs, codes_cr=codes_cr)
        std, flag = _engine.uncertainty_cr_from_codes(self.lut_co, lut_cr, plan, self.codes, codes_cr, self.inc, sigma0_dual, dsig_cr,
                                                      out_dtype=_real_dtype(out_dtype))
        return InversionUncertainty(std, None, None, flag)


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
    return CopolCodes(inc, codes, lut_co, sigma0_meta=_meta(sigma0), ancillary_meta=_meta(ancillary_wind), dsig_co=dsig_co)


def invert_joint(inc, sigma0, sigma0_dual, /, ancillary_wind=None, dsig_co=0.1, dsig_cr=0.1, model=None, details=False, **kwargs):
    """The dual-pol wind as the minimum of ONE cost over sigma0 (co-pol), sigma0_dual (cross-pol) and the a-priori wind (DESIGN.md
    section 19): `invert_copol_codes(inc, sigma0, ...)` followed by `.joint(sigma0, ancillary_wind, sigma0_dual, ...)`; returns its
    `.wind()` (complex, antenna convention) or, details=True, (wind, `JointInversion`).  model: (co-pol, cross-pol), as
    `invert_from_model` takes it for a dual-pol call; **kwargs go to both models' `to_lut`.  numpy or device rasters."""
    if not isinstance(model, (tuple, list)) or len(model) != 2:
        raise ValueError("invert_joint needs model=(co-pol model, cross-pol model)")
    cc = invert_copol_codes(inc, sigma0, ancillary_wind=ancillary_wind, dsig_co=dsig_co, model=model[0], **kwargs)
    res = cc.joint(sigma0, ancillary_wind, sigma0_dual, dsig_cr=dsig_cr, model=model[1], dsig_co=dsig_co, details=details, **kwargs)
    return (res.codes.wind(), res) if details else res.wind()
