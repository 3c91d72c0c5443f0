"""Device-resident rasters at the drop-in boundary.

`invert_from_model`, `sigma0_detrend` and `nesz_flattening` accept rasters that already live in HBM -- torch CUDA(=HIP)
tensors, or any object exposing `__cuda_array_interface__` -- and then return torch tensors on the same device: nothing
crosses PCIe, the kernels run on torch's current stream (asynchronously, ordered with the caller's other work on it).  An
interface object that names the stream its data is produced on (version 3 `stream`) is waited for on that stream first.
PyTorch is plumbing here: it owns the device memory and the stream, the work is libxsw's.
"""
import numpy as np

from . import _lib


def _torch():
    import sys
    return sys.modules.get("torch")  # never imported on behalf of a numpy caller


def is_device_array(a):
    if a is None or np.isscalar(a) or isinstance(a, np.ndarray):
        return False
    torch = _torch()
    if torch is not None and isinstance(a, torch.Tensor):
        return a.is_cuda
    return hasattr(a, "__cuda_array_interface__")


def any_device_array(*arrays):
    return any(is_device_array(a) for a in arrays)


def as_tensor(a, device, dtype=None):
    """torch view of a device array (zero copy), or an upload of a host array / scalar raster, on `device`."""
    import torch
    if isinstance(a, torch.Tensor):
        t = a if a.device == device else a.to(device)
    elif hasattr(a, "__cuda_array_interface__"):
        wait_for_producer(a.__cuda_array_interface__, device)
        t = torch.as_tensor(a, device=device)
    else:
        t = torch.as_tensor(np.asarray(a)).to(device)
    return t if dtype is None or t.dtype == dtype else t.to(dtype)


def producer_stream(cai):
    """The stream a `__cuda_array_interface__` (v3) says its data is being produced on, as a HIP stream handle, or None when
    nothing needs to be waited for.  Per the interface: absent / None = no synchronisation, 1 = the legacy default stream,
    2 = the per-thread default stream, 0 = disallowed (ambiguous), anything else = a stream handle."""
    s = cai.get("stream")
    if s is None:
        return None
    if isinstance(s, bool) or not isinstance(s, int):
        raise TypeError(f"__cuda_array_interface__ stream must be an int or None, not {type(s).__name__}")
    if s == 0:
        raise ValueError("__cuda_array_interface__ stream 0 is disallowed (ambiguous between the legacy and the per-thread "
                         "default stream)")
    return s


def wait_for_producer(cai, device):
    """Orders torch's current stream of `device` (the one the kernels will run on) after the work queued so far on the stream
    the array's producer advertises (device-side event wait; the host does not block)."""
    s = producer_stream(cai)
    if s is None:
        return
    import torch
    src = torch.cuda.default_stream(device) if s == 1 else torch.cuda.ExternalStream(s, device=device)
    cur = torch.cuda.current_stream(device)
    if src.cuda_stream != cur.cuda_stream:
        cur.wait_stream(src)


def device_of(*arrays):
    import torch
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    for a in arrays:
        if is_device_array(a):
            return torch.as_tensor(a, device="cuda").device
    raise ValueError("no device array among the arguments")


def context_of(device):
    """The libxsw context of a torch device (one without an index: torch's current device)."""
    import torch
    return _lib.default_context(device.index if device.index is not None else torch.cuda.current_device())


class on_current_stream:
    """Runs the context's launches on torch's current stream of `device` (so they are ordered with the caller's other work,
    asynchronously), then hands the context back to its own stream; both hand-overs are device-side event waits."""

    def __init__(self, ctx, device):
        import torch
        self.ctx, self.handle = ctx, torch.cuda.current_stream(device).cuda_stream

    def __enter__(self):
        self.ctx.lock.acquire()
        self.ctx.set_stream(self.handle)
        return self.ctx

    def __exit__(self, *exc):
        try:
            self.ctx.use_own_stream()
        finally:
            self.ctx.lock.release()
        return False


def meta(t):
    """(shape, numpy dtype) of a tensor, None for an absent one: what `windspeed._plan.CallPlan` is made from."""
    return None if t is None else (tuple(t.shape), np.dtype(dict(_dtype_pairs()).get(t.dtype, np.void)))  # (void: none of the four)


def _dtype_pairs():
    import torch
    return ((torch.float32, np.float32), (torch.float64, np.float64), (torch.complex64, np.complex64), (torch.complex128, np.complex128))


def torch_dtype(dt):
    return {np.dtype(n): t for t, n in _dtype_pairs()}[np.dtype(dt)]


def prep(t, dtype, shape):
    """The raster a kernel reads: `dtype`, broadcast to the call's shape, contiguous."""
    return None if t is None else t.to(torch_dtype(dtype)).expand(shape).contiguous()


def to_db(t):
    """10*log10(t + 1e-15) in t's own dtype (windspeed.py:126-130)."""
    import torch
    return None if t is None else 10 * torch.log10(t + 1e-15)


def keep_alive(tensors, device):
    """The inputs of an asynchronous launch must outlive it: tie them to the stream they are read on."""
    import torch
    for t in tensors:
        if t is not None:
            t.record_stream(torch.cuda.current_stream(device))


def at(t, off=0, size=0):
    """Address of element `off` of a tensor of `size`-byte items, of its first element by default (None for an absent tensor)."""
    return None if t is None else t.data_ptr() + off * size


def xsw_dtype(t):
    import torch
    if t.dtype in (torch.float32, torch.complex64):
        return _lib.XSW_F32
    if t.dtype in (torch.float64, torch.complex128):
        return _lib.XSW_F64
    raise TypeError(f"raster dtype must be float32/float64 (complex64/complex128), not {t.dtype}")
