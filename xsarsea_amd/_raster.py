"""What `gradients` and `streaks` share below their public functions: a raster with its coordinates (`_Raster`), and where one
kernel call runs and on which buffers (`_Call`).  Private: both modules import these names, nothing else should."""
import numpy as np

from . import _device, _lib, options


def _coord_values(v):
    return np.asarray(getattr(v, "values", v))


def _is_tensor(a):
    return _device.is_device_array(a)


def _unwrap(a):
    """The `.values` of a labelled array (an xarray.DataArray); a device tensor or a bare array passes as it is."""
    return a if _is_tensor(a) else getattr(a, "values", a)


class _Raster:
    """A 2-D or 3-D raster (numpy or device tensor) with its coordinates."""

    def __init__(self, sigma0, line=None, sample=None, pol=None, allow_pol=False):
        self.device = _device.is_device_array(sigma0)
        dims = tuple(getattr(sigma0, "dims", ()) or ())
        if self.device:
            values = _device.as_tensor(sigma0, _device.device_of(sigma0))
        elif hasattr(sigma0, "values") and not isinstance(sigma0, np.ndarray):
            values = np.asarray(sigma0.values)
            if dims:
                order = [d for d in ("pol", "line", "sample") if d in dims]
                if sorted(order) != sorted(dims) or "line" not in order or "sample" not in order:
                    raise ValueError(f"sigma0 dims must be (line, sample) with an optional pol, not {dims}")
                values = np.transpose(values, [dims.index(d) for d in order])
            line = _coord_values(sigma0.line) if line is None and hasattr(sigma0, "line") else line
            sample = _coord_values(sigma0.sample) if sample is None and hasattr(sigma0, "sample") else sample
            if pol is None and "pol" in dims:
                pol = _coord_values(sigma0.pol)
        else:
            values = np.asarray(sigma0)
        if values.ndim not in ((2, 3) if allow_pol else (2,)):
            raise ValueError(f"sigma0 must be {'2-D or 3-D' if allow_pol else '2-D'}, not {values.ndim}-D")
        self.values = values
        self.has_pol = values.ndim == 3
        shape = tuple(values.shape[-2:])
        self.line = np.arange(shape[0]) if line is None else _coord_values(line)
        self.sample = np.arange(shape[1]) if sample is None else _coord_values(sample)
        if self.line.shape != (shape[0],) or self.sample.shape != (shape[1],):
            raise ValueError("line / sample coordinates do not match the raster's shape")
        self.pol = (np.arange(values.shape[0]) if pol is None else _coord_values(pol)) if self.has_pol else None


_TORCH_DTYPE = {np.float32: "float32", np.float64: "float64", np.complex128: "complex128", np.int32: "int32", np.int64: "int64", np.uint8: "uint8"}


class _Call:
    """Where one kernel call runs: the default context of the array's device on torch's current stream (device arrays), or of
    options.device with host buffers."""

    def __init__(self, *arrays):
        self.device = any(_is_tensor(a) for a in arrays)
        if self.device:
            import torch
            self.torch = torch
            self.dev = _device.device_of(*[a for a in arrays if _is_tensor(a)])
            self.ctx = _device.context_of(self.dev)
        else:
            self.ctx = _lib.default_context(options.device)
        self.mem = _lib.MEM_DEVICE if self.device else _lib.MEM_HOST

    def _torch_dtype(self, dtype):
        return getattr(self.torch, _TORCH_DTYPE[np.dtype(dtype).type])

    def empty(self, shape, dtype):
        if self.device:
            return self.torch.empty(tuple(shape), dtype=self._torch_dtype(dtype), device=self.dev)
        return np.empty(shape, dtype)

    def prep(self, a, dtype=None):
        """Contiguous array of a kernel's input dtype (float32 / float64 rasters pass as they are, anything else -> float64)."""
        if self.device:
            t = _device.as_tensor(a, self.dev)
            if dtype is not None:
                t = t.to(self._torch_dtype(dtype))
            elif t.dtype not in (self.torch.float32, self.torch.float64):
                t = t.double()
            return t.contiguous()
        a = np.asarray(a)
        if dtype is not None:
            return np.ascontiguousarray(a, dtype=dtype)
        return np.ascontiguousarray(a if a.dtype in (np.float32, np.float64) else a.astype(np.float64))

    @staticmethod
    def ptr(a):
        return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data

    def xsw_dtype(self, a):
        if self.device:
            return _device.xsw_dtype(a)
        return _lib.XSW_F32 if a.dtype == np.float32 else _lib.XSW_F64

    def run(self, fn, inputs):
        """The low-level form of `launch`: fn(ctx, mem) on the context; the device tensors named in `inputs` are recorded on the
        launch stream (the caching allocator keeps them)."""
        if not self.device:
            return fn(self.ctx, self.mem)
        with _device.on_current_stream(self.ctx, self.dev):
            fn(self.ctx, self.mem)
            cur = self.torch.cuda.current_stream(self.dev)
            for t in inputs:
                t.record_stream(cur)

    def launch(self, name, *args):
        """ctx.<name>(*args) with every array among `args` (numpy or device tensor, input or output) passed as its address;
        `self.mem` is the call's memory kind.  Every device tensor handed in is recorded on the launch stream, so none can be
        forgotten; for one allocated on that stream this is a no-op."""
        is_array = lambda a: hasattr(a, "data_ptr") or isinstance(a, np.ndarray)
        self.run(lambda ctx, mem: getattr(ctx, name)(*[self.ptr(a) if is_array(a) else a for a in args]),
                 [a for a in args if is_array(a)])


def _small(call, a, dtype):
    """A small host table as the call's kernels want it.  On the device route it goes through page-locked staging and an
    asynchronous copy on the current stream: the host does not wait for the work queued there."""
    if not call.device or _is_tensor(a):
        return call.prep(a, dtype)
    return call.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).pin_memory().to(call.dev, non_blocking=True)


def _u8_kind(a):
    """'u8' for a bool / uint8 array (numpy or tensor), 'float' for a floating one; TypeError for anything else."""
    name = str(a.dtype).replace("torch.", "")
    if name in ("bool", "uint8"):
        return "u8"
    if name in ("float16", "bfloat16", "float32", "float64"):
        return "float"
    raise TypeError(f"a mask must be bool or uint8 (or floating, with a threshold), not {a.dtype}")


def _as_u8(call, a):
    """Contiguous uint8 array of the call's container kind from a bool / uint8 array (bool is reinterpreted, not converted)."""
    if call.device:
        t = _device.as_tensor(a, call.dev).contiguous()
        return t.view(call.torch.uint8) if t.dtype == call.torch.bool else t
    if _is_tensor(a):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a
