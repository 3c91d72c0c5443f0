"""The forward direction on rasters: the sigma0 a model predicts for a wind field, and the tangent-linear operator.

    sim = simulate_sigma0(inc, wspd, phi, model="gmf_cmod5n")                       # dB raster
    sim = simulate_sigma0(inc, wind=ancillary_wind, model="gmf_cmod5n")             # from a complex wind, antenna convention
    vh = simulate_sigma0(inc, wspd, model="gmf_s1_v2")                              # a cross-pol model takes no direction
    jac = simulate_sigma0(inc, wspd, phi, model="gmf_cmod5n", jacobian=True)        # SimulatedSigma0(sigma0, dwspd, dphi)

What is evaluated is THE TABLE THE INVERSION SEARCHES, `model.to_lut(units="dB", **kwargs)`, interpolated linearly axis by axis
(incidence, wind speed, direction) on the device (include/xsw.h: xsw_lut_eval, xsw_lut_eval_cr), so the
result is consistent with `CopolCodes.cost(...).residual_db`; `model(inc, wspd, phi)` remains the analytic evaluation of a GMF.

numpy rasters (numpy out) and device rasters (torch CUDA tensors / `__cuda_array_interface__`; torch out, asynchronous on
torch's current stream) only: xarray / dask containers are not handled here.
"""
import numpy as np

from .. import _device
from . import _engine, _plan
from .crosspol import _meta, _real_dtype, _refuse_containers
from .models import get_model


class SimulatedSigma0:
    """Result of `simulate_sigma0(..., jacobian=True)`: sigma0 in dB and the derivatives of the table's interpolant, one real
    raster each (numpy arrays, or torch tensors for device rasters): dwspd in dB per m/s, dphi in dB per degree (None for a
    cross-pol model).  They are the slopes of the cell the point lies in: piecewise constant along their own axis, and at a node
    those of the cell below it.  NaN where sigma0 is."""

    def __init__(self, sigma0, dwspd=None, dphi=None):
        self.sigma0, self.dwspd, self.dphi = sigma0, dwspd, dphi

    def __getitem__(self, name):
        return getattr(self, name)


def _is_scalar(v):
    return np.isscalar(v) or (isinstance(v, np.ndarray) and v.ndim == 0)


def same_shape_rasters(arrays):
    """True when every one of `arrays` is a numpy or device array of at least two axes and all have one shape."""
    if not all(isinstance(a, np.ndarray) or _device.is_device_array(a) for a in arrays):
        return False
    shapes = {tuple(_meta(a)[0]) for a in arrays}
    return len(shapes) == 1 and len(next(iter(shapes))) >= 2


def _rasters(who, **named):
    """The `_plan.ForwardPlan` of the given rasters (None: absent) after the refusals every entry here shares: one container
    kind, one shape, float32 / float64.  Nothing here touches the device."""
    given = {k: v for k, v in named.items() if v is not None}
    kinds = {k: _device.is_device_array(v) for k, v in given.items()}
    if len(set(kinds.values())) > 1:
        raise ValueError(f"{who}: " + ", ".join(f"{k} is a {'device' if d else 'host'} array" for k, d in kinds.items()) +
                         ": one container kind per call")
    try:
        return _plan.ForwardPlan(*(None if v is None else _meta(v) for v in named.values()))
    except ValueError as exc:
        raise ValueError(f"{who}: {exc}") from None


def _full_like(ref, value):
    """A raster of `ref`'s shape, dtype and array module holding the Python scalar `value`."""
    if _device.is_device_array(ref):
        import torch
        return torch.full_like(_device.as_tensor(ref, _device.device_of(ref)), float(value))
    return np.full_like(ref, float(value))


def _polar(wind):
    """(|wind|, degrees(angle(wind))) by the array module of the complex raster `wind`."""
    if _device.is_device_array(wind):
        import torch
        t = _device.as_tensor(wind, _device.device_of(wind))
        if not t.is_complex():
            raise TypeError(f"wind must be a complex raster, not {t.dtype}")
        return torch.abs(t), torch.rad2deg(torch.angle(t))
    if not np.iscomplexobj(wind):
        raise TypeError(f"wind must be a complex raster, not {np.asarray(wind).dtype}")
    return np.abs(wind), np.degrees(np.angle(wind))


def _same_kind_shape(who, inc, wind):
    """`wind` against `inc`: one container kind, one shape (before the array module is asked for its modulus)."""
    if _device.is_device_array(wind) != _device.is_device_array(inc):
        raise ValueError(f"{who}: inc is a {'device' if _device.is_device_array(inc) else 'host'} array, wind a "
                         f"{'device' if _device.is_device_array(wind) else 'host'} array: one container kind per call")
    if tuple(_meta(wind)[0]) != tuple(_meta(inc)[0]):
        raise ValueError(f"{who}: wind has shape {tuple(_meta(wind)[0])}, inc has shape {tuple(_meta(inc)[0])}")


def simulate_sigma0(inc, wspd=None, phi=None, *, wind=None, model=None, units="dB", fold_phi=True, jacobian=False, out_dtype=None,
                    **kwargs):
    """sigma0 that `model` predicts for the wind (wspd in m/s, phi in degrees relative to the antenna) at incidence `inc`, per
    pixel, by linear interpolation of the table the inversion searches, `model.to_lut(units="dB", **kwargs)` (`resolution="low"`
    and the step overrides pass through).  `model(inc, wspd, phi)` remains the analytic evaluation of a GMF; this is its table.

    model: any registered model name or object.  A cross-pol model takes no `phi` and has no direction derivative.
    wind: a complex raster in antenna convention (the convention of `ancillary_wind`) instead of wspd and phi; its modulus and
      degrees(angle) are taken by the array module (numpy or torch), then the same kernel runs.  Those transcendentals are the
      platform's own: their last bit is not pinned across hosts and devices.
    wspd, phi: rasters of inc's shape, or Python scalars, which are expanded to it.
    fold_phi: directions are folded into the table by sigma0(phi) = sigma0(-phi): phi modulo 360 and, beyond the table's last
      direction, 360 - phi (dphi changes sign there).  A 0..180 table thus covers every direction.  False: plain interpolation.
    units: "dB", or "linear" = 10 ** (dB / 10) by the array module after the kernel: interpolation IN dB, not of a linear table.
    jacobian: return `SimulatedSigma0(sigma0, dwspd, dphi)` with the interpolant's own slopes (dB per m/s, dB per degree).
    out_dtype: float64 (default) or float32.
    NaN where a coordinate is NaN or outside the table's axes (the direction: after the fold).
    ValueError / TypeError before any device call: xarray / dask containers, mixed numpy and device inputs, unequal shapes,
    `wind` together with wspd or phi or none of them, a co-pol model without a direction, a cross-pol model with `phi`,
    jacobian with units="linear"."""
    who = "simulate_sigma0"
    _refuse_containers(who, inc, wspd, phi, wind)
    if units not in ("dB", "linear"):
        raise ValueError(f"Unit not known: {units}. Known are 'dB' or 'linear' ")
    if jacobian and units == "linear":
        raise ValueError("jacobian=True gives derivatives of sigma0 in dB: not available with units='linear'")
    if wind is not None and (wspd is not None or phi is not None):
        raise ValueError("give either wind= or wspd (and phi), not both")
    if wind is None and wspd is None:
        raise ValueError("give the wind: wind= (complex, antenna convention) or wspd (and phi)")
    out_dtype = _real_dtype(out_dtype)
    m = get_model(model)
    copol = m.iscopol
    if not copol and phi is not None:
        raise ValueError(f"model {m.name} ({m.pol}) is a cross-pol model: it takes no phi")
    if copol and wind is None and phi is None:
        raise ValueError(f"model {m.name} ({m.pol}) is a co-pol model: phi (or wind=) is needed")
    if _is_scalar(inc) or not (isinstance(inc, np.ndarray) or _device.is_device_array(inc)):
        raise TypeError("inc must be a numpy or device raster")
    _rasters(who, inc=inc, wspd=None)  # (its dtype)
    if wind is not None:
        _same_kind_shape(who, inc, wind)
        wspd, phi = _polar(wind)
        if not copol:
            phi = None
    else:
        _rasters(who, inc=inc, wspd=None if _is_scalar(wspd) else wspd, phi=None if (phi is None or _is_scalar(phi)) else phi)  # before any expansion
        wspd = _full_like(inc, wspd) if _is_scalar(wspd) else wspd
        phi = _full_like(inc, phi) if (phi is not None and _is_scalar(phi)) else phi
    plan = _rasters(who, inc=inc, wspd=wspd, phi=phi)
    lut = _engine.lut_source(m, kwargs)
    if copol:
        outs = _engine.lut_eval(lut, plan, inc, wspd, phi, fold_phi=fold_phi, jacobian=jacobian, out_dtype=out_dtype)
    else:
        outs = _engine.lut_eval_cr(lut, plan, inc, wspd, jacobian=jacobian, out_dtype=out_dtype) + [None]
    if jacobian:
        return SimulatedSigma0(*outs)
    return outs[0] if units == "dB" else 10 ** (outs[0] / 10)


def lut_model_rasters(model, inc, wspd, phi, units, kwargs):
    """`LutModel.__call__` on rasters of one shape (ndim >= 2, numpy or device): the table `model.to_lut(units="dB", **kwargs)`
    at every pixel, without a fold of the direction (plain `interp` semantics: NaN outside the table).  Units that resolve to
    "linear" are refused: the reference would interpolate the linear table, which the device does not hold."""
    if units not in (None, "dB", "linear"):
        raise ValueError(f"Unit not known: {units}. Known are 'dB' or 'linear' ")  # (as `Model._lut`)
    resolved = units if units is not None else model._raw_lut(**kwargs).attrs["units"]
    if resolved != "dB":
        raise NotImplementedError(f"LutModel on rasters evaluates the dB table only (units resolve to {resolved!r}): use "
                                  "windspeed.simulate_sigma0(..., units='linear') for 10 ** (dB / 10) of the dB interpolation")
    if model.iscopol != (phi is not None):
        raise ValueError(f"model {model.name} ({model.pol}) " + ("needs phi" if model.iscopol else "takes no phi"))
    plan = _rasters(f"{model.name}()", inc=inc, wspd=wspd, phi=phi)
    lut = _engine.lut_source(model, kwargs)
    if phi is not None:
        return _engine.lut_eval(lut, plan, inc, wspd, phi, fold_phi=False)[0]
    return _engine.lut_eval_cr(lut, plan, inc, wspd)[0]
