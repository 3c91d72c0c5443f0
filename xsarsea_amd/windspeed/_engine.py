"""Glue between the model layer and libxsw: LUT upload cache and the numpy-in/numpy-out call that
stands where the reference's `_invert_from_model_numpy` stands (windspeed/windspeed.py:132-331)."""
import ctypes

import numpy as np

from .. import _device, _host, _lib, options
from . import _plan


def host_tables(wspd, phi):
    """Tables of xsw_lut whose last bit depends on the math library, evaluated with numpy by the same
    expressions the reference uses (windspeed.py:167-168, :235-236, :257, :270-276), so that device
    results carry exactly the bits this host's CPU path would produce."""
    wspd = np.asarray(wspd, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    e = np.stack([np.exp(1j * np.deg2rad(phi)), np.exp(1j * np.deg2rad(-phi))])  # (2, n_phi)
    sol = wspd[None, :, None] * e[:, None, :]  # (2, n_wspd, n_phi)
    unit = np.exp(1j * np.angle(sol))
    return dict(cos_phi=np.cos(np.radians(phi)), sin_phi=np.sin(np.radians(phi)),
                out_dir=np.stack([e.real, e.imag], axis=-1), abs_co=np.abs(sol[0]),
                dual_dir=np.stack([unit.real, unit.imag], axis=-1))


def _ascending(values, axes):
    """The device wants strictly ascending axes (binary searches, uniform-grid windows); the reference takes any order
    (`np.argmin(abs(dim - x))` and a flat argmin over the table).  A LUT whose coordinate runs the other way (or is
    shuffled) is therefore re-ordered here, table permuted with it: the retrieved (wspd, phi) VALUES are those of the
    reference.  (Only the resolution of exact ties -- equal cost at two grid points -- follows the sorted order instead
    of the stored one.)  Repeated coordinates cannot be ordered and are refused."""
    values = np.asarray(values, dtype=np.float64)
    out_axes = []
    for k, ax in enumerate(axes):
        ax = np.asarray(ax, dtype=np.float64)
        if ax.size > 1 and not np.all(np.diff(ax) > 0):
            if np.isnan(ax).any() or np.unique(ax).size != ax.size:
                raise ValueError(f"LUT axis {k} holds NaN or repeated coordinates: cannot be inverted on the device")
            order = np.argsort(ax, kind="stable")
            ax = ax[order]
            values = np.take(values, order, axis=k)
        out_axes.append(ax)
    return np.ascontiguousarray(values), out_axes


def _co_dict(lut):
    db, (inc, wspd, phi) = _ascending(lut.values, (lut.incidence, lut.wspd, lut.phi))
    return dict(db=db, inc=inc, wspd=wspd, phi=phi, **host_tables(wspd, phi))


def _cr_dict(lut):
    db, (inc, wspd) = _ascending(lut.values, (lut.incidence, lut.wspd))
    return dict(db=db, inc=inc, wspd=wspd)


class DeviceLut:
    """A LUT that is BUILT on the device (`xsw_lut_build`: GMF grid fill -> interpolation -> dB -> search layout) instead of
    being prepared on the host and uploaded; stands where a host `Lut` stands in `invert_numpy`.  Carries the axes only."""

    def __init__(self, model_name, gmf_id, raw_axes, target_axes, key):
        self.model_name, self.gmf_id, self.raw_axes, self.key = model_name, gmf_id, raw_axes, key
        self.incidence, self.wspd, self.phi = target_axes
        self.shape = tuple(len(a) for a in target_axes if a is not None)

    def check_axes(self):
        for ax in (self.incidence, self.wspd, self.phi) + tuple(self.raw_axes):
            if ax is not None and np.size(ax) > 1 and not np.all(np.diff(np.asarray(ax, dtype=np.float64)) > 0):
                raise ValueError("device LUT build needs strictly ascending axes (the host route re-orders them: lut_build='host')")

    def build(self, ctx):
        self.check_axes()
        target = dict(inc=self.incidence, wspd=self.wspd)
        if self.phi is not None:
            target.update(phi=self.phi, **host_tables(self.wspd, self.phi))
        ctx.build_lut(self.gmf_id, self.raw_axes, target)


def lut_source(model, kwargs):
    """The dB LUT `invert_from_model` searches for `model`: the host-prepared `Lut` (`Model._lut`, memoised; the default:
    bit parity with a CPU run of the reference on this host), or -- `options.lut_build = "device"`, built-in GMFs only -- a
    `DeviceLut` whose table never exists on the host."""
    if options.lut_build == "device" and hasattr(model, "device_lut_plan"):
        plan = model.device_lut_plan(**kwargs)
        if plan is not None:
            # memoised on the model INSTANCE, like the host route's `Model._lut` (a model re-registered under the same name
            # with other ranges is another instance), and keyed by the plan's own axes, so a stale grid is never reused;
            # unhashable kwargs never reach a dict key
            key = (plan[0],) + tuple(None if a is None else np.asarray(a, dtype=np.float64).tobytes() for a in tuple(plan[1]) + tuple(plan[2]))
            cache = model.__dict__.setdefault("_device_luts", {})
            hit = cache.get(key)
            if hit is None:
                hit = cache[key] = DeviceLut(model.name, plan[0], plan[1], plan[2], key)
            return hit
    return model._lut(units="dB", **kwargs)


def ensure_luts(ctx, lut_co, lut_cr):
    """Upload (or build in place) the dB LUT objects unless this context already holds exactly them.  `ctx.lut_key` follows the
    context's tables step by step: a LUT is recorded the moment its install has succeeded, and a failing install leaves NO key
    for that slot (the context's table is then undefined: the next call installs again instead of searching a stale GMF)."""
    key_co, key_cr = ctx.lut_key
    up_co = lut_co is not None and key_co is not lut_co
    up_cr = lut_cr is not None and key_cr is not lut_cr
    for lut, up in ((lut_co, up_co), (lut_cr, up_cr)):  # validate both before the context is touched
        if up and isinstance(lut, DeviceLut):
            lut.check_axes()
    for slot, (lut, up) in enumerate(((lut_co, up_co), (lut_cr, up_cr))):
        if not up:
            continue
        key = list(ctx.lut_key)
        key[slot] = None
        ctx.lut_key = tuple(key)  # whatever happens below, the old table of this slot is gone
        if isinstance(lut, DeviceLut):
            lut.build(ctx)
        elif slot == 0:
            ctx.upload_luts(co=_co_dict(lut))
        else:
            ctx.upload_luts(cr=_cr_dict(lut))
        key[slot] = lut
        ctx.lut_key = tuple(key)


_BLOCK = _host.BLOCK
_pool = _host.pool


def _to_db(x):
    """10*log10(x + 1e-15) in x's dtype (windspeed.py:126-130).  Large rasters are cut into blocks handled by host
    threads: every element goes through the same numpy ufuncs, so the bits are those of the one-shot expression."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        if x.size < 4 * _BLOCK or not x.flags.c_contiguous:
            return 10 * np.log10(x + 1e-15)
        out = np.empty(x.shape, dtype=(x[:1].ravel() + 1e-15).dtype)
        xf, of = x.reshape(-1), out.reshape(-1)

        def work(i):
            with np.errstate(all="ignore"):
                of[i:i + _BLOCK] = 10 * np.log10(xf[i:i + _BLOCK] + 1e-15)

        list(_pool().map(work, range(0, x.size, _BLOCK)))
        return out


def dual_select(ws_co, ws_cr):
    """np.where((np.abs(ws_co) < 5) | (np.abs(ws_cr) < 5), ws_co, ws_cr)  (windspeed.py:426-428), block-wise on the host
    pool for large rasters: the same numpy calls on every element, so the same bits (numpy's complex abs is not libm's
    hypot, which is why this select is not left to the device for numpy inputs)."""
    with np.errstate(all="ignore"):
        if ws_co.size < 4 * _BLOCK or not (ws_co.flags.c_contiguous and ws_cr.flags.c_contiguous):
            return np.where((np.abs(ws_co) < 5) | (np.abs(ws_cr) < 5), ws_co, ws_cr)
        out = _host.empty_touched(ws_co.shape, np.result_type(ws_co, ws_cr))
        a, b, o = ws_co.reshape(-1), ws_cr.reshape(-1), out.reshape(-1)

        def work(i):
            with np.errstate(all="ignore"):
                x, y = a[i:i + _BLOCK], b[i:i + _BLOCK]
                o[i:i + _BLOCK] = np.where((np.abs(x) < 5) | (np.abs(y) < 5), x, y)

        list(_pool().map(work, range(0, a.size, _BLOCK)))
        return out


def abs_blocks(z):
    """np.abs(z), block-wise on the host pool for large rasters (same bits)."""
    if z.size < 4 * _BLOCK or not z.flags.c_contiguous:
        return np.abs(z)
    out = _host.empty_touched(z.shape, np.abs(z.reshape(-1)[:1]).dtype)
    a, o = z.reshape(-1), out.reshape(-1)

    def work(i):
        with np.errstate(all="ignore"):
            o[i:i + _BLOCK] = np.abs(a[i:i + _BLOCK])

    list(_pool().map(work, range(0, a.size, _BLOCK)))
    return out


def any_valid(a):
    """`np.any(~np.isnan(a))` without materialising two rasters: block-wise with early exit."""
    a = np.asarray(a)
    if a.size <= _BLOCK or not a.flags.c_contiguous:
        return bool(np.any(~np.isnan(a)))
    flat = a.reshape(-1)
    return any(not np.isnan(flat[i:i + _BLOCK]).all() for i in range(0, a.size, _BLOCK))


def all_nan(a):
    """`np.all(np.isnan(a))`, block-wise with early exit."""
    return not any_valid(a)


def _device_list():
    """Devices of the single-process multi-GPU path (`options.devices`), or None for the one-device path."""
    devs = options.devices
    if devs is None:
        return None
    if isinstance(devs, str):
        if devs != "all":
            raise ValueError('options.devices must be None, "all" or a list of device indices')
        devs = list(range(_lib.device_count()))
    devs = [int(d) for d in devs]
    if not devs:
        raise ValueError("options.devices is an empty list")
    return devs  # (a one-entry list runs on THAT device: a single tile)


def tile_rows(lines, parts):
    """[(l0, l1)] contiguous row tiles: `lines // parts` lines each, the last one takes the remainder (multi_gpu.tile_bounds)."""
    base = lines // parts
    return [(k * base, lines if k == parts - 1 else (k + 1) * base) for k in range(parts)]


def _staged(dst, npx, dt):
    return np.frombuffer((ctypes.c_char * (npx * np.dtype(dt).itemsize)).from_address(dst), dtype=dt)


def stage_db(x, dst, dt):
    """The dB of the linear sigma0 slice `x` (1-D), as `dt` at address `dst`: numpy's own log10 in the raster's dtype is the
    reference's arithmetic (windspeed.py:126-130) and, for float32, the only way to its bits (a platform-specific few-ulp SIMD
    routine).  Same dtype: the three ufunc loops of `10 * np.log10(x + 1e-15)` write in place; else the one-shot expression."""
    out = _staged(dst, x.size, dt)
    with np.errstate(all="ignore"):
        if x.dtype == dt:
            np.add(x, 1e-15, out=out)
            np.log10(out, out=out)
            np.multiply(out, 10, out=out)
        else:
            out[...] = 10 * np.log10(x + 1e-15)


def dsig_raster(sigma0_cr, dsig_cr):
    """A scalar dsig_cr broadcast from the LINEAR sigma0_cr, in its dtype (windspeed.py:122-123; numpy array or torch tensor) --
    finite where sigma0 is; formed from the dB value it would be NaN wherever sigma0_cr + 1e-15 == 0, i.e. -inf dB."""
    with np.errstate(all="ignore"):
        return sigma0_cr * 0 + dsig_cr


def stage_fill(x, dsig_cr, dst, dt):
    """`dsig_raster` of the linear cross-pol slice `x`, cast to `dt` on assignment at address `dst`."""
    _staged(dst, x.size, dt)[...] = dsig_raster(x, dsig_cr)


def _stager(src, dt, base=0, fill=None):
    """The staging step of xsw_invert's host pipeline (xsw_invert_args.stage) over the flat linear rasters `src` {STAGE_*: array}:
    the worker thread that is about to upload a piece calls back, numpy converts that piece straight into the page-locked
    staging buffer -- no pass of its own, no dB raster in host memory.  Pixel offsets count from `base`; fill: a scalar dsig_cr."""
    def stage(which, px0, npx, dst):
        px0 += base
        if which == _lib.STAGE_DSIG_CR and fill is not None:
            stage_fill(src[_lib.STAGE_SIGMA0_CR][px0:px0 + npx], fill, dst, dt)
        elif which in src:
            stage_db(src[which][px0:px0 + npx], dst, dt)
        else:
            return 0  # (not a raster this call stages)
        return 1
    return stage


def invert_numpy(lut_co, lut_cr, inc, sigma0_co, sigma0_cr, dsig_cr, anc, dsig_co=0.1, codes=False):
    """(ws_co, ws_cr) complex128 for numpy rasters (None for a search that was not requested); any of
    sigma0_co / sigma0_cr / anc may be None.  codes=True: the uint32 grid codes instead (include/xsw.h: out_code_*; what
    `multi_gpu.invert_from_model_tiled` gathers -- 4 instead of 16 bytes per pixel -- and `expand_codes` turns into the winds).

    Raster dtypes follow the reference: the dB conversion runs in each sigma0's own dtype, then
    everything is handled as float64/complex128 (the gufunc signature, windspeed.py:308-318).  When
    every raster is float32/complex64 the device reads them as such (half the PCIe and HBM bytes)
    and widens in registers, which is the same arithmetic.

    `options.devices`: the raster's row tiles go to several GPUs from host threads, one libxsw context each, every tile
    written in place into the one output raster (pixels are independent: no exchange).
    """
    inc = np.asarray(inc)
    plan = _plan.CallPlan(_plan.meta(inc), _plan.meta(sigma0_co), _plan.meta(sigma0_cr),
                          dsig_cr if np.isscalar(dsig_cr) else _plan.meta(dsig_cr), _plan.meta(anc), device=False)
    shape, dt, want_co, want_cr = plan.shape, plan.dtype, plan.want_co, plan.want_cr
    cast = lambda a, t=dt: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a), shape), dtype=t)
    full_inc = cast(inc)
    # host dB: the linear sigma0 rasters stay in their OWN dtype and are converted piece by piece by the staging callback; they
    # (and a scalar dsig_cr's raster) are never read through their pointer: the incidence raster stands in (right size)
    lin = {w: cast(a, None) for w, a in ((_lib.STAGE_SIGMA0_CO, sigma0_co), (_lib.STAGE_SIGMA0_CR, sigma0_cr)) if plan.is_db and a is not None}
    full = dict(sigma0_co=full_inc if lin else cast(sigma0_co), sigma0_cr=full_inc if lin else cast(sigma0_cr), anc=cast(anc, plan.cdtype),
                dsig_cr=full_inc if plan.dsig == _plan.DSIG_FILL else (cast(dsig_cr) if plan.dsig == _plan.DSIG_RASTER else plan.dsig_scalar))
    if not want_co:
        full["sigma0_co"] = None
    if not want_cr:
        full["sigma0_cr"] = None

    def run(ctx, rows, out_co, out_cr):
        """One context inverts rows [l0, l1) of the (lines, samples) view of every raster, into the same rows of the outputs
        (pixel offsets of the staging callback are tile-local)."""
        cut = lambda a: a if (rows is None or a is None or np.isscalar(a)) else a[rows[0]:rows[1]]
        stage = _stager({w: cut(a).reshape(-1) for w, a in lin.items()}, dt, fill=plan.dsig_fill) if lin else None
        with ctx.lock:  # LUT upload + inversion as one step: another thread may want other LUTs on the same context
            ensure_luts(ctx, lut_co if want_co else None, lut_cr if want_cr else None)
            if options.host_threads:
                ctx.set_host_threads(options.host_threads)
            res = ctx.invert_host(cut(full_inc), **{k: cut(a) for k, a in full.items()}, dsig_co=dsig_co, sigma0_is_db=plan.is_db,
                                  algo=plan.algo, out_dtype=plan.out_dtype, out_co=cut(out_co), out_cr=cut(out_cr), stage=stage,
                                  want_codes=codes, want_complex=not codes)
            return (res[3][0], res[3][1], None) if codes else res

    devs = _device_list()
    if codes or devs is None or len(devs) == 1 or len(shape) < 2 or plan.n < options.devices_min_pixels or shape[0] < 4 * len(devs):
        # one device: `options.device`, or the one entry of `options.devices` (a one-entry list names THE device, whatever the
        # raster's size); several entries with a raster too small to tile: the first of them
        one = options.device if devs is None else devs[0]
        out_co, out_cr, _ = run(_lib.default_context(one), None, None, None)
        return out_co, out_cr  # None where that search did not run (the caller never reads it)
    # several GPUs: contiguous row tiles of the leading axis, one host thread and one context per GPU, results in place
    out_co = np.empty(shape, plan.out_dtype) if want_co else None
    out_cr = np.empty(shape, plan.out_dtype) if want_cr else None
    ctxs = _lib.contexts_for(devs)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(ctxs)) as ex:
        futs = [ex.submit(run, c, t, out_co, out_cr) for c, t in zip(ctxs, tile_rows(shape[0], len(ctxs))) if t[1] > t[0]]
        for f in futs:
            f.result()  # re-raises a tile's error here
    return out_co, out_cr


def expand_codes(lut_co, lut_cr, codes_co, codes_cr):
    """Grid codes -> (ws_co, ws_cr) complex128 on the host, from the tables of these LUTs (installed on the context if they are not)."""
    ctx = _lib.default_context(options.device)
    with ctx.lock:
        ensure_luts(ctx, lut_co if codes_co is not None else None, lut_cr if codes_cr is not None else None)
        return ctx.expand_codes_host(codes_co, codes_cr)


def _device_rasters(inc, sigma0_co, sigma0_cr, dsig_cr, anc, dual_select, broadcast=None):
    """(plan, device, [inc, sigma0_co, sigma0_cr, dsig_cr, anc] as the kernel reads them) for rasters resident in HBM (host
    arrays among them are uploaded).  Mixed dtypes (float32 sigma0 next to a float64 incidence, say): torch converts sigma0 to
    dB in sigma0's OWN dtype before anything is widened, after a scalar dsig_cr was broadcast from the LINEAR sigma0_cr.
    broadcast: the caller's own shape check (`invert_device`: torch's, whose error a shape mismatch has always raised there)."""
    args = (inc, sigma0_co, sigma0_cr, None if np.isscalar(dsig_cr) else dsig_cr, anc)
    dev = _device.device_of(*(a for a in args if a is not None))
    t = [None if a is None else _device.as_tensor(a, dev) for a in args]
    if broadcast is not None:
        broadcast(*(x.shape for x in t if x is not None))
    plan = _plan.CallPlan(*(dsig_cr if (k == 3 and x is None) else _device.meta(x) for k, x in enumerate(t)), device=True, dual_select=dual_select)
    if plan.dsig == _plan.DSIG_FILL:
        t[3] = dsig_raster(t[2], dsig_cr)
    if plan.db_by == _plan.DB_TORCH:
        t[1], t[2] = _device.to_db(t[1]), _device.to_db(t[2])
    return plan, dev, [_device.prep(x, plan.cdtype if k == 4 else plan.dtype, plan.shape) for k, x in enumerate(t)]


def invert_device(lut_co, lut_cr, inc, sigma0_co, sigma0_cr, dsig_cr, anc, dsig_co=0.1, dual_select=False, codes=False):
    """(ws_co, ws_cr) torch complex tensors for rasters resident in HBM (torch CUDA tensors / `__cuda_array_interface__`
    objects; host arrays among them are uploaded): the drop-in call without PCIe.  sigma0 -> dB is fused into the kernel
    (float32 rasters: float32 arithmetic like the reference, the log10 correctly rounded -- numpy's float32 log10 is a few-ulp
    SIMD routine, so ~2e-5 of the pixels of a float32 raster land one grid step from a numpy run; float64 rasters agree bit for
    bit).  Asynchronous on torch's current stream.  dual_select: ws_cr receives the fused where(|co|<5 | |dual|<5, co, dual).
    codes=True: the grid codes (int32 tensors holding the uint32 bit patterns) instead of the winds."""
    import torch
    plan, dev, t = _device_rasters(inc, sigma0_co, sigma0_cr, dsig_cr, anc, dual_select, broadcast=torch.broadcast_shapes)
    ctx = _device.context_of(dev)
    odt = torch.int32 if codes else _device.torch_dtype(plan.out_dtype)
    out_co = torch.empty(plan.shape, dtype=odt, device=dev) if plan.want_co else None
    out_cr = torch.empty(plan.shape, dtype=odt, device=dev) if plan.want_cr else None
    p = _device.at
    if plan.n:
        with _device.on_current_stream(ctx, dev):
            ensure_luts(ctx, lut_co if plan.want_co else None, lut_cr if plan.want_cr else None)
            outs = (None, None, None) if codes else (p(out_co), p(out_cr), None)
            ctx.invert_raw(plan.lines, plan.samples, plan.code, plan.out_code, _lib.MEM_DEVICE, *(p(x) for x in t), *outs,
                           dsig_co, plan.dsig_scalar, plan.is_db, plan.algo, plan.fused_select,
                           out_code_co=p(out_co) if codes else None, out_code_cr=p(out_cr) if codes else None)
            _device.keep_alive(t, dev)
    return out_co, out_cr


def _code_tensor(codes):
    """Grid codes in device memory as a torch tensor (zero copy): an int32 / uint32 tensor or any `__cuda_array_interface__` array."""
    import torch
    t = _device.as_tensor(codes, _device.device_of(codes))
    if t.dtype not in (torch.int32, torch.uint32):
        raise TypeError(f"grid codes must be int32 or uint32, not {t.dtype}")
    return t


def expand_device(lut_co, codes_co):
    """Co-pol grid codes in device memory (int32 tensor) -> the complex winds `invert_device` stores, on torch's current stream."""
    import torch
    codes_co = _code_tensor(codes_co)
    dev = codes_co.device
    ctx = _device.context_of(dev)
    out_dtype = np.complex64 if options.device_out_dtype == "complex64" else np.complex128
    out = torch.empty(codes_co.shape, dtype=_device.torch_dtype(out_dtype), device=dev)
    if codes_co.numel():
        with _device.on_current_stream(ctx, dev):
            ensure_luts(ctx, lut_co, None)
            ctx.expand_codes_raw(codes_co.numel(), _lib.MEM_DEVICE, _lib.XSW_F32 if out_dtype == np.complex64 else _lib.XSW_F64,
                                 codes_co.data_ptr(), None, out.data_ptr(), None)
            _device.keep_alive([codes_co], dev)
    return out


def cross_plan(shape, inc, sigma0_co, anc, sigma0_cr, dsig_cr, *, device, dual_select=False):
    """The `CallPlan` of the dual-pol call whose cross-pol step runs on its own: inc, sigma0_co, anc are the (shape, dtype) the
    co-pol call saw, sigma0_cr / dsig_cr those of this one -- so dtype, dB route and dsig_cr handling are the fused call's.
    ValueError when the cross-pol rasters do not broadcast to the co-pol codes' `shape`."""
    try:
        plan = _plan.CallPlan(inc, sigma0_co, sigma0_cr, dsig_cr, anc, device=device, dual_select=dual_select)
    except ValueError as exc:
        raise ValueError(f"cross-pol rasters do not broadcast against the co-pol codes of shape {tuple(shape)}: {exc}") from None
    if plan.shape != tuple(shape):
        raise ValueError(f"cross-pol rasters broadcast to {plan.shape}, the co-pol codes have shape {tuple(shape)}")
    return plan


class _HostCodes:
    """The kernel-ready numpy rasters of one from-codes call, [inc, sigma0, dsig_cr, anc, *codes] (None for an absent one), formed
    with `invert_numpy`'s arithmetic: a scalar dsig_cr broadcast from the LINEAR sigma0 (`plan.dsig`), sigma0 to dB by numpy's
    own log10 in its own dtype when the plan says so, everything then cast to `plan.dtype` (the ancillary wind: `plan.cdtype`),
    the codes uint32.  `run` calls xsw_*_from_codes on host memory: synchronous, under the context's lock."""
    mem = _lib.MEM_HOST

    def __init__(self, plan, inc, sigma0, dsig_cr, anc, *codes, sigma0_too=None):
        cast = lambda a, t=plan.dtype: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a), plan.shape), dtype=t)
        sigma0 = np.asarray(sigma0)
        dsig = dsig_raster(sigma0, plan.dsig_fill) if plan.dsig == _plan.DSIG_FILL else (dsig_cr if plan.dsig == _plan.DSIG_RASTER else None)
        self.plan, self.ctx = plan, _lib.default_context(options.device)
        self.rasters = [cast(inc), cast(_to_db(sigma0) if plan.is_db else sigma0), cast(dsig), cast(anc, plan.cdtype)]
        self.rasters += [np.ascontiguousarray(c, dtype=np.uint32) for c in codes]
        if sigma0_too is not None:  # a second sigma0 raster, after the codes, to dB as the first (`joint_from_codes`: the co-pol one)
            self.rasters.append(cast(_to_db(np.asarray(sigma0_too)) if plan.is_db else sigma0_too))

    @staticmethod
    def at(a):
        return None if a is None else a.ctypes.data

    def empty(self, dtype=None):  # None: grid codes
        return np.empty(self.plan.shape, np.uint32 if dtype is None else dtype)

    def run(self, lut_co, lut_cr, call):
        if self.plan.n:
            with self.ctx.lock:
                ensure_luts(self.ctx, lut_co, lut_cr)
                call(self.ctx, *(self.at(x) for x in self.rasters))


class _DeviceCodes:
    """`_HostCodes` for rasters resident in HBM (host arrays among them are uploaded next to the codes), following
    `invert_device`: torch's dB (`_device.to_db`) where the plan leaves it to torch, int32 codes.  `run` is asynchronous on
    torch's current stream."""
    mem = _lib.MEM_DEVICE
    at = staticmethod(_device.at)

    def __init__(self, plan, inc, sigma0, dsig_cr, anc, *codes, sigma0_too=None):
        codes = [_code_tensor(c) for c in codes]
        dev = self.dev = codes[0].device
        t = [None if (a is None or np.isscalar(a)) else _device.as_tensor(a, dev) for a in (inc, sigma0, dsig_cr, anc)]
        if plan.dsig == _plan.DSIG_FILL:
            t[2] = dsig_raster(t[1], plan.dsig_fill)
        if plan.db_by == _plan.DB_TORCH:
            t[1] = _device.to_db(t[1])
        self.plan, self.ctx = plan, _device.context_of(dev)
        self.rasters = [_device.prep(x, plan.cdtype if k == 3 else plan.dtype, plan.shape) for k, x in enumerate(t)] + [c.contiguous() for c in codes]
        if sigma0_too is not None:
            x = _device.as_tensor(sigma0_too, dev)
            self.rasters.append(_device.prep(_device.to_db(x) if plan.db_by == _plan.DB_TORCH else x, plan.dtype, plan.shape))

    def empty(self, dtype=None):  # None: grid codes; uint8: a flag raster
        import torch
        t = torch.int32 if dtype is None else torch.uint8 if np.dtype(dtype) == np.uint8 else _device.torch_dtype(dtype)
        return torch.empty(self.plan.shape, dtype=t, device=self.dev)

    def run(self, lut_co, lut_cr, call):
        if self.plan.n:
            with _device.on_current_stream(self.ctx, self.dev):
                ensure_luts(self.ctx, lut_co, lut_cr)
                call(self.ctx, *(self.at(x) for x in self.rasters))
                _device.keep_alive(self.rasters, self.dev)


def _codes_call(plan, inc, sigma0, dsig_cr, anc, *codes, **more):
    """The inputs of a from-codes call where the co-pol codes are: `_DeviceCodes` or `_HostCodes`."""
    return (_DeviceCodes if _device.is_device_array(codes[0]) else _HostCodes)(plan, inc, sigma0, dsig_cr, anc, *codes, **more)


def cross_from_codes(lut_co, lut_cr, plan, codes_co, inc, sigma0_cr, dsig_cr, dual_select=False, codes=False):
    """The cross-pol step from the co-pol codes `codes_co` (xsw_cross_from_codes; `plan` from `cross_plan`), numpy rasters on
    host memory or device rasters on torch's current stream: the cross-pol winds (the select fused with dual_select) or,
    codes=True, the cross-pol grid codes (numpy: uint32; torch: int32)."""
    k = _codes_call(plan, inc, sigma0_cr, dsig_cr, None, codes_co)
    out = k.empty() if codes else k.empty(plan.out_dtype)
    k.run(lut_co, lut_cr, lambda ctx, inc, s_cr, dsig, _, cc: ctx.cross_from_codes_raw(
        plan.lines, plan.samples, plan.code, plan.out_code, k.mem, inc, cc, s_cr, dsig, k.at(out) if codes else None,
        None if codes else k.at(out), dsig_cr_scalar=plan.dsig_scalar, sigma0_is_db=plan.is_db, dual_select=dual_select))
    return out


def _cost_outputs(parts, empty):
    """[J, Jsig, Jwind, residual] rasters from `empty()`; parts=False: J alone, the others None (not computed)."""
    return [empty() if (k == 0 or parts) else None for k in range(4)]


def _real_code(out_dtype):
    return _lib.XSW_F32 if np.dtype(out_dtype) == np.float32 else _lib.XSW_F64


def cost_from_codes(lut_co, plan, codes_co, inc, sigma0, anc, dsig_co=0.1, parts=True, out_dtype=np.float64):
    """[J, Jsig, Jwind, residual_db] (`out_dtype`; numpy, or torch for device rasters) of the co-pol codes `codes_co` from the
    rasters they were computed from (xsw_cost_from_codes; `plan` is the co-pol call's, so the dB route is the search's)."""
    k = _codes_call(plan, inc, sigma0, None, anc, codes_co)
    outs = _cost_outputs(parts, lambda: k.empty(out_dtype))
    k.run(lut_co, None, lambda ctx, inc, s_co, _, anc, cc: ctx.cost_from_codes_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), k.mem, inc, cc, s_co, anc, *(k.at(o) for o in outs),
        dsig_co=dsig_co, sigma0_is_db=plan.is_db))
    return outs


def cost_cr_from_codes(lut_co, lut_cr, plan, codes_co, codes_cr, inc, sigma0_cr, dsig_cr, parts=True, out_dtype=np.float64):
    """[J, Jsig, Jwind, residual_db] of the cross-pol codes `codes_cr` (from `cross_from_codes`, with or without the select): the
    cross-pol inputs formed as that call forms them (`plan` from `cross_plan`), then xsw_cost_cr_from_codes."""
    k = _codes_call(plan, inc, sigma0_cr, dsig_cr, None, codes_co, codes_cr)
    outs = _cost_outputs(parts, lambda: k.empty(out_dtype))
    k.run(lut_co, lut_cr, lambda ctx, inc, s_cr, dsig, _, cc, ccr: ctx.cost_cr_from_codes_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), k.mem, inc, cc, ccr, s_cr, dsig, *(k.at(o) for o in outs),
        dsig_cr_scalar=plan.dsig_scalar, sigma0_is_db=plan.is_db))
    return outs


def joint_from_codes(lut_co, lut_cr, plan, codes_co, inc, sigma0_co, anc, sigma0_cr, dsig_cr, dsig_co=0.1, details=False, out_dtype=np.float64):
    """[codes, J, Jwind, Jsig_co, Jsig_cr] of the joint dual-pol inversion from the co-pol codes `codes_co` (xsw_joint_from_codes;
    `plan` from `cross_plan`, so dtype, dB route and dsig_cr handling are the fused dual-pol call's): the grid codes of the wind
    that minimises Jwind_co + Jsig_co + Jsig_cr (numpy: uint32; torch: int32) and, details=True, the cost and its terms there
    (`out_dtype`; else None: not computed)."""
    k = _codes_call(plan, inc, sigma0_cr, dsig_cr, anc, codes_co, sigma0_too=sigma0_co)
    outs = [k.empty()] + [k.empty(out_dtype) if details else None for _ in range(4)]
    k.run(lut_co, lut_cr, lambda ctx, inc, s_cr, dsig, anc, cc, s_co: ctx.joint_from_codes_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), k.mem, inc, cc, s_co, anc, s_cr, dsig, *(k.at(o) for o in outs),
        dsig_co=dsig_co, dsig_cr_scalar=plan.dsig_scalar, sigma0_is_db=plan.is_db))
    return outs


def uncertainty_from_codes(lut_co, plan, codes_co, inc, sigma0, anc, dsig_co=0.1, out_dtype=np.float64):
    """[wspd_std, dir_std, corr] (`out_dtype`) and the uint8 flag raster (numpy, or torch for device rasters) of the co-pol codes
    `codes_co` from the rasters they were computed from (xsw_uncertainty_from_codes; `plan` is the co-pol call's)."""
    k = _codes_call(plan, inc, sigma0, None, anc, codes_co)
    outs = [k.empty(out_dtype) for _ in range(3)] + [k.empty(np.uint8)]
    k.run(lut_co, None, lambda ctx, inc, s_co, _, anc, cc: ctx.uncertainty_from_codes_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), k.mem, inc, cc, s_co, anc, *(k.at(o) for o in outs),
        dsig_co=dsig_co, sigma0_is_db=plan.is_db))
    return outs


def uncertainty_cr_from_codes(lut_co, lut_cr, plan, codes_co, codes_cr, inc, sigma0_cr, dsig_cr, out_dtype=np.float64):
    """[wspd_std, flag] of the cross-pol codes `codes_cr`: the cross-pol inputs formed as `cost_cr_from_codes` forms them, then
    xsw_uncertainty_cr_from_codes."""
    k = _codes_call(plan, inc, sigma0_cr, dsig_cr, None, codes_co, codes_cr)
    outs = [k.empty(out_dtype), k.empty(np.uint8)]
    k.run(lut_co, lut_cr, lambda ctx, inc, s_cr, dsig, _, cc, ccr: ctx.uncertainty_cr_from_codes_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), k.mem, inc, cc, ccr, s_cr, dsig, *(k.at(o) for o in outs),
        dsig_cr_scalar=plan.dsig_scalar, sigma0_is_db=plan.is_db))
    return outs


def uncertainty_joint_from_codes(lut_co, lut_cr, plan, codes, inc, sigma0_co, anc, sigma0_cr, dsig_cr, dsig_co=0.1, out_dtype=np.float64):
    """[wspd_std, dir_std, corr, u_std, v_std, corr_uv] (`out_dtype`) and the uint8 flag raster of the grid codes `codes` from the
    curvature of the joint cost (xsw_uncertainty_joint_from_codes): the inputs formed as `joint_from_codes` forms them (`plan` from
    `cross_plan`), the outputs as `uncertainty_from_codes` returns them."""
    k = _codes_call(plan, inc, sigma0_cr, dsig_cr, anc, codes, sigma0_too=sigma0_co)
    outs = [k.empty(out_dtype) for _ in range(6)] + [k.empty(np.uint8)]
    k.run(lut_co, lut_cr, lambda ctx, inc, s_cr, dsig, anc, cc, s_co: ctx.uncertainty_joint_from_codes_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), k.mem, inc, cc, s_co, anc, s_cr, dsig, *(k.at(o) for o in outs),
        dsig_co=dsig_co, dsig_cr_scalar=plan.dsig_scalar, sigma0_is_db=plan.is_db))
    return outs


def _lut_eval(lut, cross, plan, rasters, n_out, out_dtype, call, n_flag=0):
    """The host path of `lut_eval` / `lut_eval_cr` / `wspd_solve` / `wspd_solve_cr` / `dir_solve`, in the manner of `_HostCodes` /
    `_DeviceCodes`: the rasters as the kernel reads them (`plan.dtype`, contiguous), `n_out` outputs of `out_dtype` and after them `n_flag` uint8
    ones, the LUT installed in its slot, then
    call(ctx, mem, input addresses, output addresses).  numpy rasters: host memory, synchronous, under the context's lock;
    device rasters: torch outputs, asynchronous on torch's current stream."""
    luts = (None, lut) if cross else (lut, None)
    if _device.is_device_array(rasters[0]):
        import torch
        dev = _device.device_of(*rasters)
        t = [_device.prep(_device.as_tensor(a, dev), plan.dtype, plan.shape) for a in rasters]
        outs = [torch.empty(plan.shape, dtype=_device.torch_dtype(out_dtype), device=dev) for _ in range(n_out)]
        outs += [torch.empty(plan.shape, dtype=torch.uint8, device=dev) for _ in range(n_flag)]
        if plan.n:
            ctx = _device.context_of(dev)
            with _device.on_current_stream(ctx, dev):
                ensure_luts(ctx, *luts)
                call(ctx, _lib.MEM_DEVICE, [_device.at(x) for x in t], [_device.at(o) for o in outs])
                _device.keep_alive(t, dev)
        return outs
    t = [np.ascontiguousarray(a, dtype=plan.dtype) for a in rasters]
    outs = [np.empty(plan.shape, out_dtype) for _ in range(n_out)] + [np.empty(plan.shape, np.uint8) for _ in range(n_flag)]
    if plan.n:
        ctx = _lib.default_context(options.device)
        with ctx.lock:
            ensure_luts(ctx, *luts)
            call(ctx, _lib.MEM_HOST, [x.ctypes.data for x in t], [o.ctypes.data for o in outs])
    return outs


def lut_eval(lut_co, plan, inc, wspd, phi, fold_phi=True, jacobian=False, out_dtype=np.float64):
    """[sigma0_db] or, jacobian=True, [sigma0_db, dwspd, dphi] (`out_dtype`; numpy, or torch for device rasters) that the co-pol
    dB LUT `lut_co` predicts for the wind (wspd, phi) at `inc` (xsw_lut_eval; `plan` a `_plan.ForwardPlan` of the three)."""
    return _lut_eval(lut_co, False, plan, (inc, wspd, phi), 3 if jacobian else 1, out_dtype, lambda ctx, mem, ins, outs: ctx.lut_eval_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), mem, *ins, *outs, fold_phi=fold_phi))


def lut_eval_cr(lut_cr, plan, inc, wspd, jacobian=False, out_dtype=np.float64):
    """[sigma0_db] or [sigma0_db, dwspd] of the cross-pol dB LUT `lut_cr`, which has no direction (xsw_lut_eval_cr)."""
    return _lut_eval(lut_cr, True, plan, (inc, wspd), 2 if jacobian else 1, out_dtype, lambda ctx, mem, ins, outs: ctx.lut_eval_cr_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), mem, *ins, *outs))


def wspd_solve(lut_co, plan, inc, sigma0_db, phi, fold_phi=True, details=False, out_dtype=np.float64):
    """[wspd] or, details=True, [wspd, dwspd_dsigma0, flag] (`out_dtype`, the flag uint8 SOLVE_* bits; numpy, or torch for device
    rasters): the lowest wind speed at which the co-pol dB LUT `lut_co` gives `sigma0_db` at `inc` and direction `phi`
    (xsw_wspd_solve; `plan` a `_plan.ForwardPlan` of the three)."""
    return _lut_eval(lut_co, False, plan, (inc, sigma0_db, phi), 2 if details else 1, out_dtype, lambda ctx, mem, ins, outs: ctx.wspd_solve_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), mem, *ins, *outs, fold_phi=fold_phi), n_flag=int(details))


def wspd_solve_cr(lut_cr, plan, inc, sigma0_db, details=False, out_dtype=np.float64):
    """The same on the cross-pol dB LUT `lut_cr`, which has no direction (xsw_wspd_solve_cr)."""
    return _lut_eval(lut_cr, True, plan, (inc, sigma0_db), 2 if details else 1, out_dtype, lambda ctx, mem, ins, outs: ctx.wspd_solve_cr_raw(
        plan.lines, plan.samples, plan.code, _real_code(out_dtype), mem, *ins, *outs), n_flag=int(details))


DIR_REALS = ("phi1", "phi2", "sens1", "sens2", "phi_near", "sens_near", "phi_closest")  # xsw_dir_solve's outputs, in its order
DIR_BYTES = ("count", "flag")


def dir_solve(lut_co, plan, inc, sigma0_db, wspd, near=None, fold_phi=True, outputs=("phi1", "phi2"), out_dtype=np.float64):
    """{name: raster} for the `outputs` asked for among DIR_REALS (`out_dtype`) and DIR_BYTES (uint8; numpy, or torch for device
    rasters): the directions at which the co-pol dB LUT `lut_co` gives `sigma0_db` at `inc` and wind speed `wspd`, and with the
    reference direction `near` the one nearest to it (xsw_dir_solve; `plan` a `_plan.ForwardPlan` of the rasters given)."""
    reals, small = [k for k in DIR_REALS if k in outputs], [k for k in DIR_BYTES if k in outputs]
    if set(outputs) - set(reals) - set(small) or not (reals or small):
        raise ValueError(f"dir_solve: outputs {tuple(outputs)} are not among {DIR_REALS + DIR_BYTES}")

    def call(ctx, mem, ins, outs):
        at = dict(zip(reals + small, outs))
        ctx.dir_solve_raw(plan.lines, plan.samples, plan.code, _real_code(out_dtype), mem, ins[0], ins[1], ins[2], ins[3] if near is not None else None,
                          *(at.get(k) for k in DIR_REALS + DIR_BYTES), fold_phi=fold_phi)

    rasters = (inc, sigma0_db, wspd) + ((near,) if near is not None else ())
    return dict(zip(reals + small, _lut_eval(lut_co, False, plan, rasters, len(reals), out_dtype, call, n_flag=len(small))))


def _uploaded_rasters(inc, sigma0_co, sigma0_cr, dsig_cr, anc):
    """`_device_rasters` for a tile of numpy rasters, which follow `invert_numpy`'s arithmetic: (plan, device, tensors, src).
    With host dB the linear sigma0 stays on the host -- `src` {STAGE_*: flat raster}, converted piece by piece on its way up,
    its tensors None -- and a scalar dsig_cr's raster is formed whole, in sigma0's own dtype, and uploaded."""
    import torch
    h = [None if a is None or np.isscalar(a) else np.asarray(a) for a in (inc, sigma0_co, sigma0_cr, dsig_cr, anc)]
    plan = _plan.CallPlan(*(dsig_cr if (k == 3 and x is None) else _plan.meta(x) for k, x in enumerate(h)), device=False, coded=True)
    dev = torch.device("cuda", int(options.device))
    if plan.dsig == _plan.DSIG_FILL:
        h[3] = dsig_raster(h[2], dsig_cr)
    src = {}
    if plan.is_db:
        src = {w: np.ascontiguousarray(np.broadcast_to(h[k], plan.shape)).reshape(-1)
               for k, w in ((1, _lib.STAGE_SIGMA0_CO), (2, _lib.STAGE_SIGMA0_CR)) if h[k] is not None}
        h[1] = h[2] = None
    t = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in h]
    return plan, dev, [_device.prep(x, plan.cdtype if k == 4 else plan.dtype, plan.shape) for k, x in enumerate(t)], src


def invert_coded(lut_co, lut_cr, inc, sigma0_co, sigma0_cr, dsig_cr, anc, dsig_co, sink, dual_select=False):
    """A rank's row tile -> 4-byte grid codes in DEVICE memory, chunk by chunk, for the gathered multi-GPU call
    (`multi_gpu.invert_from_model_tiled`; `sink` is its `_CodeSink`: it owns the code buffers, starts the gather of every
    chunk and queues its expansion on the destination rank).  numpy or device rasters; nothing of the answer visits the host.

    Two phases, so that a rank that fails leaves no peer waiting in a transfer: everything that can raise for a reason of
    the inputs -- dtypes, shapes, LUT install, uploads -- happens HERE, before any exchange; the returned `launch()` only queues
    kernels and transfers (the caller agrees with the other ranks in between).

    numpy rasters follow `invert_numpy`'s arithmetic: float32 sigma0 is converted to dB on the host with numpy's own log10
    (`options.db_on_device = "auto"`; bit parity with the reference) -- through libxsw's staging ring while the other rasters
    are already resident (XSW_MEM_DEVICE_SIGMA0_HOST) -- and a scalar `dsig_cr` is broadcast from the LINEAR sigma0
    (windspeed.py:122-123).  Device rasters follow `invert_device` (sigma0 -> dB fused, the dual-pol select fused)."""
    import torch
    from .. import multi_gpu
    if _device.any_device_array(inc, sigma0_co, sigma0_cr, dsig_cr, anc):
        (plan, dev, t), src = _device_rasters(inc, sigma0_co, sigma0_cr, dsig_cr, anc, dual_select), {}
    else:
        plan, dev, t, src = _uploaded_rasters(inc, sigma0_co, sigma0_cr, dsig_cr, anc)
    ctx = _device.context_of(dev)
    sink.begin(plan.shape, plan.want_co, plan.want_cr, dev, _device.torch_dtype(plan.out_dtype))
    with ctx.lock:
        ensure_luts(ctx, lut_co if plan.want_co else None, lut_cr if plan.want_cr else None)  # (also on a rank whose tile is empty: it may expand)

    def host_sigma0(off, npx, lines):
        """sigma0 of one chunk of host-dB rasters: through the staging ring (the host addresses are never read: the callback
        fills every piece), or -- a chunk too thin for the ring -- numpy's dB of these rows, uploaded (the tensors go back with
        their addresses: the chunk's launch holds them)."""
        if lines >= 4:
            return (_lib.MEM_DEVICE_SIGMA0_HOST,) + tuple(None if w not in src else src[w].ctypes.data + off * src[w].itemsize
                                                           for w in (_lib.STAGE_SIGMA0_CO, _lib.STAGE_SIGMA0_CR)) + (_stager(src, plan.dtype, off), ())
        up = {w: np.empty(npx, plan.dtype) for w in src}
        for w, buf in up.items():
            stage_db(src[w][off:off + npx], buf.ctypes.data, plan.dtype)
        up = {w: torch.from_numpy(buf).to(dev) for w, buf in up.items()}  # (held by the chunk's launch: `chunk_calls`)
        return _lib.MEM_DEVICE, _device.at(up.get(_lib.STAGE_SIGMA0_CO)), _device.at(up.get(_lib.STAGE_SIGMA0_CR)), None, list(up.values())

    invert_chunk, expand_rows = multi_gpu.chunk_calls(
        ctx, sink.pipe, t, plan.code, plan.out_code, _lib.MEM_DEVICE,
        (dsig_co, plan.dsig_scalar, plan.is_db, plan.algo, plan.fused_select), flat=len(plan.shape) < 2, sigma0=host_sigma0 if src else None)

    def launch():
        with _device.on_current_stream(ctx, dev):
            sink.pipe.run(invert_chunk, expand_rows)
            _device.keep_alive(t, dev)

    return launch
