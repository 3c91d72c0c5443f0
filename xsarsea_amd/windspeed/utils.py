"""Cross-pol preprocessing helpers used right before `invert_from_model`
(reference: src/xsarsea/windspeed/utils.py): `get_dsig` (:47-91), `get_dsig_wspd` (:18-44),
`nesz_flattening` (:94-163).

`get_dsig*` are elementwise formulas (host numpy, bit-identical to the reference incl. its dtype promotion:
tests/golden/crosspol_prep.npz; rasters resident in HBM go through `xsw_dsig` / `xsw_dsig_wspd` and stay there), and
`dsig_from_nesz` is `get_dsig` on the flattened noise in one device pass (`xsw_dsig_flat`).  `nesz_flattening` is a full-raster pass -- column nan-mean, then one degree-1
least-squares fit per line in dB -- and runs on the device for large rasters (`xsw_nesz_flatten`, include/xsw.h;
`options.nesz_on_device`); the host route below reproduces the reference bit for bit.
"""
import warnings

import numpy as np

_DSIG_WSPD = {
    "dsig_wspd_rs2_v3": (-0.4908643753212401, 16.763199934792965, 1.3891445172991084, 20.616914824394343),
    "dsig_wspd_s1_ew_rec_v3": (-0.5858970325653666, 16.50039320910609, 1.1032031322520397, 7.434663633997121),
    "dsig_wspd_rcm_v3": (-0.7920301376936547, 15.8288289109038, 0.24040294696606557, 0.2538177092195224),
}
# logistic exponent c(inc) of the S1 v2 rule: rate, centre, floor, span.  numpy float64 scalars on purpose: like the
# reference's coefficient array they promote a float32 incidence raster to float64.
_S1_V2_EXPONENT = np.array([1.57952257, 25.61843791, 1.46852088, 1.4058646])


_DSIG_NAMES_MESSAGE = ("dsig names different than 'gmf_s1_v2' or 'gmf_rs2_v2' or 'sarwing_lut_cmodms1ahw' or "
                       "'nc_lut_cmodms1ahw' are not handled. You can compute your own dsig_cr.")


def _np_dtype(a):
    """numpy dtype of an argument of the device route, or the Python scalar itself (weak in numpy's promotion)."""
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, (np.ndarray, np.generic)):
        return a.dtype
    if hasattr(a, "__cuda_array_interface__"):
        return np.dtype(a.__cuda_array_interface__["typestr"])
    return np.asarray(a).dtype


def _raster_dtype(dt):
    """float32 stays, everything else is computed in float64 (the kernels' two raster types)."""
    return np.dtype(np.float32) if dt == np.float32 else np.dtype(np.float64)


def _shape_of(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _device_call(arrays):
    """(device, context) of a call whose arguments hold a device array."""
    from .. import _device
    dev = _device.device_of(*arrays)
    return dev, _device.context_of(dev)


def _get_dsig_wspd_device(name, U_crosspol, SNR_cr):
    """`xsw_dsig_wspd` on torch's current stream: float64 arithmetic, returned in numpy's promoted dtype."""
    import torch
    from .. import _device, _lib
    rule = _lib.DSIG_WSPD_RULES[name]
    shape = np.broadcast_shapes(_shape_of(U_crosspol), _shape_of(SNR_cr))
    res = np.result_type(_np_dtype(U_crosspol), _np_dtype(SNR_cr), 1.0)
    dev, ctx = _device_call((U_crosspol, SNR_cr))
    t_u, t_s = (_device.prep(_device.as_tensor(a, dev), np.float64, shape) for a in (U_crosspol, SNR_cr))
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    if out.numel():
        with _device.on_current_stream(ctx, dev):
            ctx.dsig_wspd_raw(rule, out.numel(), _lib.MEM_DEVICE, t_u.data_ptr(), t_s.data_ptr(), out.data_ptr())
            _device.keep_alive((t_u, t_s), dev)
    return out if res == np.float64 else out.to(_device.torch_dtype(_raster_dtype(res)))


def get_dsig_wspd(name, U_crosspol, SNR_cr):
    """Weight alpha(U, SNR) in [0, 1]: logistic in (U - c0 + gamma*SNR) times a roll-off above Umax = 30.

    Device arrays (torch CUDA tensors, `__cuda_array_interface__` objects) among the arguments: a torch tensor on that device
    comes back, computed by `xsw_dsig_wspd` on the current stream."""
    b, c0_base, gamma, k = _DSIG_WSPD[name]
    from .. import _device
    if _device.any_device_array(U_crosspol, SNR_cr):
        return _get_dsig_wspd_device(name, U_crosspol, SNR_cr)
    centre = c0_base - gamma * SNR_cr
    core = 1 / (1 + np.exp(-b * (U_crosspol - centre)))
    drop = 1 / (1 + np.exp((U_crosspol - 30) * k))
    return np.clip(core * drop, 0, 1)


def _get_dsig_device(name, inc, sigma0_cr, nesz_cr):
    """`xsw_dsig` on torch's current stream.  The dtypes are numpy's: the ratio in the common dtype of sigma0_cr and nesz_cr,
    float64 from there on under gmf_s1_v2.  The kernel reads sigma0_cr and inc in one dtype: where they differ both are widened
    to float64, which changes nothing unless sigma0_cr and nesz_cr are both float32 and inc is not (the ratio is then the
    float64 quotient instead of the float32 one)."""
    import torch
    from .. import _device, _lib
    rule = _lib.DSIG_RULES[name]
    s1 = name == "gmf_s1_v2"
    used = (sigma0_cr, nesz_cr) + ((inc,) if s1 else ())
    shape = np.broadcast_shapes(*(_shape_of(a) for a in used))
    weak = lambda a: isinstance(_np_dtype(a), (bool, int, float))  # Python scalars take the other operand's dtype
    both_weak = weak(sigma0_cr) and weak(nesz_cr)
    r_dt = _raster_dtype(np.float64 if both_weak else np.result_type(_np_dtype(sigma0_cr), _np_dtype(nesz_cr), np.float32))
    own = lambda a: r_dt if weak(a) else _raster_dtype(_np_dtype(a))
    s_dt, n_dt = own(sigma0_cr), own(nesz_cr)
    if s1 and (weak(inc) or _raster_dtype(_np_dtype(inc)) != s_dt):
        s_dt = np.dtype(np.float64)
    out_dt = np.dtype(np.float64) if s1 else r_dt
    dev, ctx = _device_call(used)
    t_s = _device.prep(_device.as_tensor(sigma0_cr, dev), s_dt, shape)
    t_n = _device.prep(_device.as_tensor(nesz_cr, dev), n_dt, shape)
    t_i = _device.prep(_device.as_tensor(inc, dev), s_dt, shape) if s1 else None
    out = torch.empty(shape, dtype=_device.torch_dtype(out_dt), device=dev)
    if out.numel():
        lines, samples = _lib.lines_samples(shape)
        with _device.on_current_stream(ctx, dev):
            ctx.dsig_raw(rule, lines, samples, _device.xsw_dtype(t_s), _device.xsw_dtype(t_n), _lib.MEM_DEVICE, _device.at(t_i),
                         t_s.data_ptr(), t_n.data_ptr(), out.data_ptr())
            _device.keep_alive((t_s, t_n, t_i), dev)
    return out


def get_dsig(name, inc, sigma0_cr, nesz_cr):
    """`dsig_cr` for `invert_from_model` from the cross-pol signal-to-noise ratio.

    Device arrays (torch CUDA tensors, `__cuda_array_interface__` objects) among the arguments: a torch tensor on that device
    comes back, computed by `xsw_dsig` on the current stream; scalars and host arrays are broadcast and uploaded."""
    from .. import _device, _lib
    if _device.any_device_array(inc, sigma0_cr, nesz_cr):
        if name not in _lib.DSIG_RULES:
            raise ValueError(_DSIG_NAMES_MESSAGE)
        return _get_dsig_device(name, inc, sigma0_cr, nesz_cr)
    if name == "gmf_s1_v2":
        rate, centre, floor, span = _S1_V2_EXPONENT
        c = floor + span / (1 + np.exp(-rate * (inc - centre)))
        return 1 / np.sqrt(1 * (sigma0_cr / nesz_cr) ** c)
    if name == "gmf_rs2_v2":
        return 1 / np.sqrt(1 * (sigma0_cr / nesz_cr) ** 8)
    if name in ("sarwing_lut_cmodms1ahw", "nc_lut_cmodms1ahw"):
        return (1.25 / (sigma0_cr / nesz_cr)) ** 4.0
    raise ValueError(_DSIG_NAMES_MESSAGE)


def _nesz_flattening_host(values, inc):
    """The reference's arithmetic, line by line (utils.py:119-163), dtypes left as they come."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        col_mean = np.nanmean(values, axis=0)
        inc_row = np.nanmean(inc, axis=0)  # "incidence is almost constant along line dim"
    out = np.empty(values.shape, dtype=np.float64)
    for i, row in enumerate(values):
        filled = row.copy()
        gap = np.isnan(filled)
        filled[gap] = col_mean[gap]
        with np.errstate(all="ignore"):
            db = 10.0 * np.log10(filled)
        ok = np.isfinite(db)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                slope, icpt = np.polyfit(inc_row[ok], db[ok], 1)
        except TypeError:  # nothing to fit on this line
            out[i] = np.nan
            continue
        out[i] = 10.0 ** ((inc_row * slope + icpt - 1.0) / 10.0)
    return out


def nesz_flattening(noise, inc):
    """Flatten a (line, sample) noise-equivalent sigma0 by a per-line degree-1 fit of its dB value
    against incidence; NaNs are first replaced by the column mean.  Returns 10**((fit - 1)/10), float64.

    >>> nesz_flat = nesz_flattening(nesz_cr, inc)
    >>> dsig_cr = (1.25 / (sigma0_cr / nesz_flat)) ** 4.0
    """
    if noise.ndim != 2:
        raise IndexError("Only 2D noise allowed")
    from .. import _device, _lib, options
    if _device.any_device_array(noise, inc):  # rasters resident in HBM: a float64 torch tensor comes back, asynchronously
        import torch
        dev = _device.device_of(noise, inc)
        t_n, t_i = _device.as_tensor(noise, dev), _device.as_tensor(inc, dev)
        dt = torch.float32 if (t_n.dtype == torch.float32 and t_i.dtype == torch.float32) else torch.float64
        t_n, t_i = t_n.to(dt).contiguous(), t_i.to(dt).expand(t_n.shape).contiguous()
        out = torch.empty(t_n.shape, dtype=torch.float64, device=dev)
        if t_n.numel():
            ctx = _device.context_of(dev)
            with _device.on_current_stream(ctx, dev):
                ctx.nesz_flatten_raw(t_n.shape[0], t_n.shape[1], _device.xsw_dtype(t_n), _lib.MEM_DEVICE, t_n.data_ptr(), t_i.data_ptr(),
                                     out.data_ptr())
                for t in (t_n, t_i):
                    t.record_stream(torch.cuda.current_stream(dev))
        return out
    values, inc_v = np.asarray(noise), np.asarray(inc)
    mode = options.nesz_on_device
    # "auto" is parity-first like the other defaults: float64 rasters only (device == host route to ~1e-13); float32 rasters
    # -- where the reference itself accumulates in float32 and the float64 device sums differ from it by ~1e-6 -- go to the
    # device on request only ("device")
    on_dev = mode == "device" or (mode == "auto" and values.size >= options.nesz_device_min_size
                                  and values.dtype == np.float64 and inc_v.dtype == np.float64
                                  and _lib.device_count_safe() > 0)
    if on_dev and values.dtype in (np.float32, np.float64) and inc_v.shape == values.shape and values.size:
        return _lib.default_context(options.device).nesz_flatten_host(values, inc_v)
    return _nesz_flattening_host(values, inc_v)


def dsig_from_nesz(name, inc, sigma0_cr, nesz_cr, out_dtype=None):
    """`get_dsig(name, inc, sigma0_cr, nesz_flattening(nesz_cr, inc))`: `dsig_cr` straight from the unflattened noise.

    Device arrays take one fused pass after the flattening's fit (`xsw_dsig_flat`): the flattened noise never reaches HBM, the
    result is bit-equal to the two calls.  `out_dtype=None` gives float64 (the reference's dtype, its flattened noise being
    float64); `np.float32` rounds that value once, for float32 inversion rasters.  Host arrays compute the composition itself
    (the flattening on the route `options.nesz_on_device` picks), then `.astype(out_dtype)` if given."""
    if nesz_cr.ndim != 2:
        raise IndexError("Only 2D noise allowed")
    from .. import _device, _lib
    if name not in _lib.DSIG_RULES:
        raise ValueError(_DSIG_NAMES_MESSAGE)
    if not _device.any_device_array(inc, sigma0_cr, nesz_cr):
        out = get_dsig(name, inc, sigma0_cr, nesz_flattening(nesz_cr, inc))
        return out if out_dtype is None else out.astype(out_dtype)
    import torch
    out_dt = np.dtype(np.float64 if out_dtype is None else out_dtype)
    if out_dt not in (np.float32, np.float64):
        raise TypeError(f"out_dtype must be float32 or float64 on the device route, not {out_dt}")
    dev, ctx = _device_call((nesz_cr, inc, sigma0_cr))
    t_n, t_i, t_s = (_device.as_tensor(a, dev) for a in (nesz_cr, inc, sigma0_cr))
    shape = tuple(t_n.shape)
    if np.broadcast_shapes(shape, tuple(t_s.shape), tuple(t_i.shape)) != shape:
        raise ValueError(f"sigma0_cr {tuple(t_s.shape)} and inc {tuple(t_i.shape)} must broadcast to the noise raster {shape}")
    dt = np.dtype(np.float32 if (t_n.dtype == torch.float32 and t_i.dtype == torch.float32) else np.float64)
    if dt == np.float32 and t_s.dtype != torch.float32:
        # a sigma0 wider than the float32 rasters the flattening is fitted on: the kernel has one raster dtype, so the two calls
        return get_dsig(name, t_i, t_s, nesz_flattening(t_n, t_i)).to(_device.torch_dtype(out_dt))
    t_n, t_i, t_s = (_device.prep(t, dt, shape) for t in (t_n, t_i, t_s))
    out = torch.empty(shape, dtype=_device.torch_dtype(out_dt), device=dev)
    if out.numel():
        with _device.on_current_stream(ctx, dev):
            ctx.dsig_flat_raw(_lib.DSIG_RULES[name], shape[0], shape[1], _device.xsw_dtype(t_n), _device.xsw_dtype(out), _lib.MEM_DEVICE,
                              t_n.data_ptr(), t_i.data_ptr(), t_s.data_ptr(), out.data_ptr())
            _device.keep_alive((t_n, t_i, t_s), dev)
    return out
