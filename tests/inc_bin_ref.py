"""CPU restatement of the device's incidence bin (test infrastructure; the executable specification of `nearest_index`,
csrc/xsw_device.hpp): `np.argmin(np.abs(dim - x))` on a strictly ascending axis, first minimum (the reference's
windspeed/windspeed.py:212, :254), found the way the kernels find it.

    inf shortcut   x = +-inf: every |dim - x| is inf, argmin gives 0
    uniform path   (host: `uniform_axis`, csrc/xsw_lutplan.hpp) g = (x - x0) * inv_step clamped to [-1, n] (a NaN becomes -1), the start
                   bin k = ceil(g) clamped to [0, n], then at most four steps of one node towards  dim[k - 1] < x <= dim[k];  a
                   walk that has not settled by then falls through to the bisection over the whole axis
    bisection      lo = the first node with dim[lo] >= x  (any other axis)
    tie rule       lo == 0 -> 0;  lo == n -> n - 1;  else  |dim[lo] - x| < |dim[lo - 1] - x| ? lo : lo - 1  (a tie: the lower node)

`x0` and `inv_step` are the host's (`plan`): dim[0] and (n - 1) / (dim[n - 1] - dim[0]), 0 for n = 1.  Scalar float64 throughout,
IEEE + - * and comparisons only, in the kernel's order."""
import math

import numpy as np

WALK_STEPS = 4


def plan(dim):
    """(x0, inv_step) as co_scalars / cr_scalars of csrc/xsw_lutplan.hpp set inc0 / inv_incstep."""
    dim = np.asarray(dim, dtype=np.float64)
    n = dim.size
    return float(dim[0]), float((n - 1) / (dim[n - 1] - dim[0])) if n > 1 else 0.0


def uniform_axis(dim):
    """`uniform_axis` of csrc/xsw_lutplan.hpp restated (tests/test_host_lutplan.py holds the header itself to these statements)."""
    a = np.asarray(dim, dtype=np.float64)
    n = a.size
    if n < 2:
        return False
    step = (a[n - 1] - a[0]) / (n - 1)
    if not (step > 0) or not math.isfinite(step):
        return False
    tol = 1e-12 * max(max(abs(a[0]), abs(a[n - 1])), step)
    return bool(np.all(np.abs(a - (a[0] + np.arange(n) * step)) <= tol))


def start_bin(n, x, x0, inv_step):
    """The bin the uniform path starts its walk from."""
    g = np.float64(x - x0) * np.float64(inv_step)
    g = -1.0 if np.isnan(g) else min(max(float(g), -1.0), float(n))  # fmin(fmax(g, -1), n): a NaN gives -1
    return min(max(int(math.ceil(g)), 0), n)


def lower_bound(dim, x, uniform=False, x0=0.0, inv_step=0.0):
    """(lo, fell_through): lo = the first index with dim[lo] >= x (n: none), fell_through = the uniform walk did not settle in
    WALK_STEPS steps and the bisection ran (always False on the bisection path itself)."""
    n = len(dim)
    lo, hi, fell = 0, n, False
    if uniform:
        k, ok = start_bin(n, x, x0, inv_step), False
        for _ in range(WALK_STEPS):
            below, here = dim[max(k - 1, 0)], dim[min(k, n - 1)]
            down, up = k > 0 and not (below < x), k < n and here < x
            k += int(up) - int(down)
            ok = not up and not down
            if ok:
                break
        if ok:
            lo = hi = k
        else:
            fell = True
    while lo < hi:
        mid = (lo + hi) >> 1
        if dim[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo, fell


def nearest_index(dim, x, uniform=False, x0=0.0, inv_step=0.0, details=False):
    """The device's incidence bin of one value (a NaN is the callers' business: they never pass one)."""
    n = len(dim)
    if math.isinf(x):
        return (0, False) if details else 0
    lo, fell = lower_bound(dim, x, uniform, x0, inv_step)
    if lo == 0:
        i = 0
    elif lo == n:
        i = n - 1
    else:
        dl, dh = abs(dim[lo - 1] - x), abs(dim[lo] - x)
        i = lo if dh < dl else lo - 1
    return (i, fell) if details else i


def nearest_indices(dim, xs, path="host"):
    """nearest_index of every value of `xs` (NaN: -1): path "host" as an install of `dim` would run it (uniform where
    `uniform_axis` says so), "uniform" / "bisect" forced.  Returns (indices int64, fell_through bool)."""
    dim = [float(v) for v in np.asarray(dim, dtype=np.float64)]
    x0, inv_step = plan(dim)
    uniform = {"host": uniform_axis(dim), "uniform": True, "bisect": False}[path]
    xs = np.asarray(xs, dtype=np.float64).ravel()
    idx, fell = np.full(xs.size, -1, np.int64), np.zeros(xs.size, bool)
    for j, x in enumerate(xs):
        if not np.isnan(x):
            idx[j], fell[j] = nearest_index(dim, float(x), uniform, x0, inv_step, details=True)
    return idx, fell


def argmin_indices(dim, xs):
    """The specification: np.argmin(np.abs(dim - x)) per value (NaN: -1)."""
    dim = np.asarray(dim, dtype=np.float64)
    xs = np.asarray(xs, dtype=np.float64).ravel()
    with np.errstate(all="ignore"):
        idx = np.argmin(np.abs(dim[None, :] - xs[:, None]), axis=1).astype(np.int64)
    return np.where(np.isnan(xs), -1, idx)
