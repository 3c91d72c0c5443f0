"""Wind speed at a known direction: the classical SAR scheme.  The direction comes from elsewhere (wind streaks, a model), the
speed is read off the GMF at that direction.

    wspd = retrieve_wspd(inc, sigma0, phi, model="gmf_cmod5n")                          # phi: degrees relative to the antenna
    wspd = retrieve_wspd(inc, sigma0, wind=ancillary_from_streaks(...), model="gmf_cmod5n")   # only the angle of `wind` is used
    wspd = retrieve_wspd(inc, sigma0_vh, model="gmf_s1_v2")                             # a cross-pol model takes no direction
    r = retrieve_wspd(inc, sigma0, phi, model="gmf_cmod5n", details=True)               # RetrievedWspd(wspd, dwspd_dsigma0, flag)

What is inverted is THE TABLE THE INVERSION SEARCHES, `model.to_lut(units="dB", **kwargs)`, along its wind-speed axis at the
pixel's incidence and direction (include/xsw.h: xsw_wspd_solve, xsw_wspd_solve_cr): `simulate_sigma0` of the
result gives sigma0 back to rounding.  No a-priori wind speed enters, unlike `invert_from_model`.

numpy rasters (numpy out) and device rasters (torch CUDA tensors / `__cuda_array_interface__`; torch out, asynchronous on
torch's current stream) only: xarray / dask containers are not handled here.
"""
import numpy as np

from .. import _device
from .._lib import SOLVE_ABOVE, SOLVE_BELOW, SOLVE_NAN, SOLVE_TAIL  # noqa: F401 (the bits of RetrievedWspd.flag)
from . import _engine, _plan
from .crosspol import _meta, _real_dtype, _refuse_containers
from .forward import _full_like, _is_scalar, _same_kind_shape
from .models import get_model


class RetrievedWspd:
    """Result of `retrieve_wspd(..., details=True)`, one raster each (numpy arrays, or torch tensors for device rasters):
    wspd in m/s, the LOWEST speed at which the table gives the observed sigma0; dwspd_dsigma0 in m/s per dB, the inverse of the
    table's speed slope in the cell of the solution (+-inf in a flat cell): |dwspd_dsigma0| * dsig is the a-posteriori speed error
    of this retrieval; flag, uint8: SOLVE_NAN (1: a NaN input, or incidence / direction outside the table), SOLVE_BELOW (2) /
    SOLVE_ABOVE (4): sigma0 below / above everything the table holds at that incidence and direction -- wspd is NaN with any of
    the three -- and SOLVE_TAIL (8): the solution lies past the rows over which the table rises monotonically (CMOD5.N turns
    over below 41 degrees of incidence, from 23.6 m/s on), where a second, higher solution may exist."""

    def __init__(self, wspd, dwspd_dsigma0=None, flag=None):
        self.wspd, self.dwspd_dsigma0, self.flag = wspd, dwspd_dsigma0, flag

    def __getitem__(self, name):
        return getattr(self, name)


def _plan_of(who, **named):
    """The `_plan.ForwardPlan` of (inc, sigma0, phi) after the refusals: one container kind, one shape, float32 / float64."""
    given = {k: v for k, v in named.items() if v is not None}
    kinds = {k: _device.is_device_array(v) for k, v in given.items()}
    if len(set(kinds.values())) > 1:
        raise ValueError(f"{who}: " + ", ".join(f"{k} is a {'device' if d else 'host'} array" for k, d in kinds.items()) +
                         ": one container kind per call")
    try:
        return _plan.ForwardPlan(*(None if v is None else _meta(v) for v in named.values()))
    except ValueError as exc:
        raise ValueError(f"{who}: {str(exc).replace('wspd', 'sigma0')}") from None


def _angle_deg(wind):
    """degrees(angle(wind)) by the array module of the complex raster `wind`."""
    if _device.is_device_array(wind):
        import torch
        t = _device.as_tensor(wind, _device.device_of(wind))
        if not t.is_complex():
            raise TypeError(f"wind must be a complex raster, not {t.dtype}")
        return torch.rad2deg(torch.angle(t))
    if not np.iscomplexobj(wind):
        raise TypeError(f"wind must be a complex raster, not {np.asarray(wind).dtype}")
    return np.degrees(np.angle(wind))


def _to_db(sigma0):
    """10 * log10(sigma0 + 1e-15) in sigma0's dtype, by its array module's helper (as `invert_from_model`)."""
    if _device.is_device_array(sigma0):
        return _device.to_db(_device.as_tensor(sigma0, _device.device_of(sigma0)))
    return _engine._to_db(sigma0)


def retrieve_wspd(inc, sigma0, phi=None, *, wind=None, model=None, units="linear", fold_phi=True, details=False, out_dtype=None, **kwargs):
    """Wind speed (m/s) at which `model` gives `sigma0` at incidence `inc` and wind direction `phi`, per pixel: the inverse along
    the wind-speed axis of the table the inversion searches, `model.to_lut(units="dB", **kwargs)` (`resolution="low"` and the
    step overrides pass through), interpolated linearly in incidence, then direction.  The LOWEST such speed is returned; NaN
    where there is none (see `RetrievedWspd` for the flags).

    sigma0: linear by default, as in `invert_from_model`: 10 * log10(sigma0 + 1e-15) in its own dtype first.  units="dB": taken as
      it is (the output of `simulate_sigma0`, say).
    phi: a raster of inc's shape or a Python scalar, degrees relative to the antenna (the convention of `simulate_sigma0`).
    wind: instead of phi, a complex raster in antenna convention -- what `streaks.ancillary_from_streaks` returns, or
      `ancillary_wind` -- of which only the angle is used, taken by the array module (numpy or torch).
    model: any registered model name or object.  A co-pol model needs one of phi / wind; a cross-pol model takes neither.
    fold_phi: directions are folded into the table by sigma0(phi) = sigma0(-phi), as `simulate_sigma0` does.
    details: return `RetrievedWspd(wspd, dwspd_dsigma0, flag)`.
    out_dtype: float64 (default) or float32.
    ValueError / TypeError before any device call: xarray / dask containers, mixed numpy and device inputs, unequal shapes, phi
    together with wind, a co-pol model without a direction, a cross-pol model with one, unknown units, a bad out_dtype."""
    who = "retrieve_wspd"
    _refuse_containers(who, inc, sigma0, phi, wind)
    if units not in ("dB", "linear"):
        raise ValueError(f"Unit not known: {units}. Known are 'dB' or 'linear' ")
    if wind is not None and phi is not None:
        raise ValueError("give either wind= or phi, not both")
    out_dtype = _real_dtype(out_dtype)
    m = get_model(model)
    copol = m.iscopol
    if not copol and (phi is not None or wind is not None):
        raise ValueError(f"model {m.name} ({m.pol}) is a cross-pol model: it takes no phi and no wind")
    if copol and wind is None and phi is None:
        raise ValueError(f"model {m.name} ({m.pol}) is a co-pol model: phi (or wind=) is needed")
    for name, v in (("inc", inc), ("sigma0", sigma0)):
        if _is_scalar(v) or not (isinstance(v, np.ndarray) or _device.is_device_array(v)):
            raise TypeError(f"{name} must be a numpy or device raster")
    _plan_of(who, inc=inc, sigma0=sigma0, phi=None if (phi is None or _is_scalar(phi)) else phi)  # before anything is formed
    if wind is not None:
        _same_kind_shape(who, inc, wind)
        phi = _angle_deg(wind)
    elif phi is not None and _is_scalar(phi):
        phi = _full_like(inc, phi)
    if units == "linear":
        sigma0 = _to_db(sigma0)
    plan = _plan_of(who, inc=inc, sigma0=sigma0, phi=phi)
    lut = _engine.lut_source(m, kwargs)
    if copol:
        outs = _engine.wspd_solve(lut, plan, inc, sigma0, phi, fold_phi=fold_phi, details=details, out_dtype=out_dtype)
    else:
        outs = _engine.wspd_solve_cr(lut, plan, inc, sigma0, details=details, out_dtype=out_dtype)
    return RetrievedWspd(*outs) if details else outs[0]
