"""Wind direction at a known speed, and the a-priori-free wind vector from dual-pol rasters.  A cross-pol GMF gives a speed that
needs no direction; at that speed the co-pol GMF gives the observed sigma0 at a small set of directions -- typically two on
0..180 degrees plus their mirror images -- and a reference direction (wind streaks, a model) picks one.

    phi1, phi2 = retrieve_dir(inc, sigma0_vv, wspd, model="gmf_cmod5n")                    # the first two solutions on the table's axis
    phi = retrieve_dir(inc, sigma0_vv, wspd, near=phi_ref, model="gmf_cmod5n")             # the solution nearest to phi_ref (degrees)
    phi = retrieve_dir(inc, sigma0_vv, wspd, wind=ancillary_from_streaks(...), model=...)   # only the angle of `wind` is used
    r = retrieve_dir(inc, sigma0_vv, wspd, near=phi_ref, model=..., details=True)          # RetrievedDir, nine rasters
    wind = retrieve_wind(inc, sigma0_vv, sigma0_vh, near=phi_ref, model=("gmf_cmod5n", "gmf_s1_v2"))   # complex, antenna convention

What is inverted is THE TABLE THE INVERSION SEARCHES, `model.to_lut(units="dB", **kwargs)`, along its direction axis at the pixel's
incidence and speed (include/xsw.h: xsw_dir_solve): `simulate_sigma0` of the result gives sigma0 back to
rounding.  No a-priori wind vector enters, unlike `invert_from_model`.

numpy rasters (numpy out) and device rasters (torch CUDA tensors / `__cuda_array_interface__`; torch out, asynchronous on
torch's current stream) only: xarray / dask containers are not handled here.
"""
import numpy as np

from .. import _device
from .._lib import DIR_ABOVE, DIR_BELOW, DIR_MORE, DIR_NAN  # noqa: F401 (the bits of RetrievedDir.flag)
from . import _engine, _plan
from .crosspol import _meta, _real_dtype, _refuse_containers
from .forward import _full_like, _is_scalar, _same_kind_shape
from .models import get_model
from .retrieve import _angle_deg, _to_db, retrieve_wspd


class RetrievedDir:
    """Result of `retrieve_dir(..., details=True)`, one raster each (numpy arrays, or torch tensors for device rasters).  Directions
    are degrees relative to the antenna, on the table's own direction axis (0..180 for the built-in GMFs):
    phi1, phi2: the first and second direction, in ascending order, at which the table gives the observed sigma0; NaN where there is
      none.  dphi1_dsigma0, dphi2_dsigma0: the inverse of the table's direction slope in their cells, degrees per dB (+-inf in a
      flat cell): |dphi_dsigma0| * dsig is the a-posteriori direction error of this retrieval.
    phi_near, dphi_near_dsigma0: with a reference direction, the solution nearest to it on the circle among ALL solutions and
      (fold_phi) their mirror images -phi, and its sensitivity (negated for a mirror image); NaN where the reference is NaN or there
      is no solution; None without a reference direction.
    phi_closest: the direction of the table node whose sigma0 is closest to the observed one: where there is no solution, the
      crosswind (sigma0 below the column's minimum) or the up- / downwind direction (above its maximum).
    count, uint8: the number of solutions on the table's axis (saturating at 255).
    flag, uint8: DIR_NAN (1: a NaN input, or incidence / speed outside the table), DIR_BELOW (2) / DIR_ABOVE (4): no solution, sigma0
      below / above what the table holds at that incidence and speed; DIR_MORE (8): more than two solutions, of which two are stored."""

    FIELDS = ("phi1", "phi2", "dphi1_dsigma0", "dphi2_dsigma0", "phi_near", "dphi_near_dsigma0", "phi_closest", "count", "flag")

    def __init__(self, phi1, phi2=None, dphi1_dsigma0=None, dphi2_dsigma0=None, phi_near=None, dphi_near_dsigma0=None, phi_closest=None,
                 count=None, flag=None):
        self.phi1, self.phi2, self.dphi1_dsigma0, self.dphi2_dsigma0 = phi1, phi2, dphi1_dsigma0, dphi2_dsigma0
        self.phi_near, self.dphi_near_dsigma0, self.phi_closest, self.count, self.flag = phi_near, dphi_near_dsigma0, phi_closest, count, flag

    def __getitem__(self, name):
        return getattr(self, name)


def _plan_of(who, **named):
    """The `_plan.ForwardPlan` of (inc, sigma0, wspd, near) after the refusals: one container kind, one shape, float32 / float64."""
    given = {k: v for k, v in named.items() if v is not None}
    kinds = {k: _device.is_device_array(v) for k, v in given.items()}
    if len(set(kinds.values())) > 1:
        raise ValueError(f"{who}: " + ", ".join(f"{k} is a {'device' if d else 'host'} array" for k, d in kinds.items()) +
                         ": one container kind per call")
    try:
        return _plan.ForwardPlan(*(None if v is None else _meta(v) for v in named.values()))
    except ValueError as exc:
        raise ValueError(f"{who}: {str(exc).replace('inc, wspd and phi', ', '.join(named))}") from None


def retrieve_dir(inc, sigma0, wspd, *, near=None, wind=None, model=None, units="linear", fold_phi=True, details=False, out_dtype=None,
                 **kwargs):
    """Wind directions (degrees relative to the antenna) at which `model` gives `sigma0` at incidence `inc` and wind speed `wspd`,
    per pixel: the inverse along the direction axis of the table the inversion searches, `model.to_lut(units="dB", **kwargs)`
    (`resolution="low"` and the step overrides pass through), interpolated linearly in incidence, then speed.

    Returns, without a reference direction, the pair (phi1, phi2): the first two solutions in ascending order on the table's own
    axis (NaN where there is none); with one, phi_near: the solution nearest to it; details=True: `RetrievedDir`.

    sigma0: linear by default, as in `invert_from_model`: 10 * log10(sigma0 + 1e-15) in its own dtype first.  units="dB": taken as
      it is.
    wspd: a raster of inc's shape or a Python scalar, m/s: `retrieve_wspd(inc, sigma0_vh, model="gmf_s1_v2")`, say.
    near: the reference direction, a raster of inc's shape or a Python scalar, degrees in the convention of `simulate_sigma0`,
      any range.
    wind: instead of near, a complex raster in antenna convention -- what `streaks.ancillary_from_streaks` returns, or
      `ancillary_wind` -- of which only the angle is used, taken by the array module (numpy or torch).
    model: a registered co-pol model name or object; a cross-pol model has no direction and is refused.
    fold_phi: the mirror images -phi of the solutions are candidates of the selection, by sigma0(phi) = sigma0(-phi).
    out_dtype: float64 (default) or float32.
    ValueError / TypeError before any device call: xarray / dask containers, mixed numpy and device inputs, unequal shapes, near
    together with wind, a cross-pol model, unknown units, a bad out_dtype."""
    who = "retrieve_dir"
    _refuse_containers(who, inc, sigma0, wspd, near, wind)
    if units not in ("dB", "linear"):
        raise ValueError(f"Unit not known: {units}. Known are 'dB' or 'linear' ")
    if wind is not None and near is not None:
        raise ValueError("give either wind= or near=, not both")
    out_dtype = _real_dtype(out_dtype)
    m = get_model(model)
    if not m.iscopol:
        raise ValueError(f"model {m.name} ({m.pol}) is a cross-pol model: its table has no direction to retrieve")
    for name, v in (("inc", inc), ("sigma0", sigma0)):
        if _is_scalar(v) or not (isinstance(v, np.ndarray) or _device.is_device_array(v)):
            raise TypeError(f"{name} must be a numpy or device raster")
    rasters = dict(inc=inc, sigma0=sigma0, wspd=None if _is_scalar(wspd) else wspd, near=None if (near is None or _is_scalar(near)) else near)
    _plan_of(who, **rasters)  # before anything is formed
    if wind is not None:
        _same_kind_shape(who, inc, wind)
        near = _angle_deg(wind)
    elif near is not None and _is_scalar(near):
        near = _full_like(inc, near)
    if _is_scalar(wspd):
        wspd = _full_like(inc, wspd)
    if units == "linear":
        sigma0 = _to_db(sigma0)
    plan = _plan_of(who, inc=inc, sigma0=sigma0, wspd=wspd, near=near)
    lut = _engine.lut_source(m, kwargs)
    if details:
        outputs = tuple(k for k in _engine.DIR_REALS + _engine.DIR_BYTES if near is not None or k not in ("phi_near", "sens_near"))
    else:
        outputs = ("phi_near",) if near is not None else ("phi1", "phi2")
    r = _engine.dir_solve(lut, plan, inc, sigma0, wspd, near=near, fold_phi=fold_phi, outputs=outputs, out_dtype=out_dtype)
    if details:
        return RetrievedDir(*(r.get(k) for k in _engine.DIR_REALS + _engine.DIR_BYTES))
    return r["phi_near"] if near is not None else (r["phi1"], r["phi2"])


def retrieve_wind(inc, sigma0_co, sigma0_cr, *, near=None, wind=None, model=None, units="linear", out_dtype=None, **kwargs):
    """The wind vector from dual-pol rasters without an a-priori wind speed: the speed from `retrieve_wspd` on the cross-pol model
    (which needs no direction), the direction from `retrieve_dir` on the co-pol model at that speed, the ambiguity chosen by the
    reference direction `near` (or the angle of the complex raster `wind`; one of the two is required).

    Returns wspd * exp(1j * radians(phi_near)) by the array module (numpy or torch): complex128, or complex64 with
    out_dtype=float32 (both steps run in float64 either way), antenna convention as `ancillary_wind`.  NaN where either step has no
    answer: sigma0_cr outside the cross-pol table, a speed beyond the co-pol table's axis (the default co-pol table ends at 50 m/s,
    the cross-pol one at 80), sigma0_co below or above everything the co-pol table holds at that speed, a NaN reference direction.

    model: (co-pol model, cross-pol model), names or objects.  units and **kwargs go to both steps."""
    who = "retrieve_wind"
    _refuse_containers(who, inc, sigma0_co, sigma0_cr, near, wind)
    if (near is None) == (wind is None):
        raise ValueError(f"{who}: give one of near= and wind=: the reference direction that picks the ambiguity")
    if not isinstance(model, (tuple, list)) or len(model) != 2:
        raise ValueError(f"{who}: model=(co-pol model, cross-pol model) is needed")
    co, cr = (get_model(x) for x in model)
    if not co.iscopol or cr.iscopol:
        raise ValueError(f"{who}: model=(co-pol model, cross-pol model), not ({co.name} ({co.pol}), {cr.name} ({cr.pol}))")
    out_dtype = _real_dtype(out_dtype)
    if units not in ("dB", "linear"):
        raise ValueError(f"Unit not known: {units}. Known are 'dB' or 'linear' ")
    for name, v in (("inc", inc), ("sigma0_co", sigma0_co), ("sigma0_cr", sigma0_cr)):
        if _is_scalar(v) or not (isinstance(v, np.ndarray) or _device.is_device_array(v)):
            raise TypeError(f"{name} must be a numpy or device raster")
    _plan_of(who, inc=inc, sigma0_co=sigma0_co, sigma0_cr=sigma0_cr, near=None if (near is None or _is_scalar(near)) else near)
    if wind is not None:
        _same_kind_shape(who, inc, wind)
    wspd = retrieve_wspd(inc, sigma0_cr, model=cr, units=units, **kwargs)
    phi = retrieve_dir(inc, sigma0_co, wspd, near=near, wind=wind, model=co, units=units, **kwargs)
    if _device.is_device_array(phi):
        import torch
        out = wspd * torch.exp(1j * torch.deg2rad(phi))
        return out.to(torch.complex64) if out_dtype == np.float32 else out
    out = wspd * np.exp(1j * np.radians(phi))
    return out.astype(np.complex64) if out_dtype == np.float32 else out
