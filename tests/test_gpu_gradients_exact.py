"""k_grad_r2, k_grad_local, k_grad_smooth, k_grad_mean and k_grad_filter on the MI355X against tests/gradients_exact.py, the
kernels restated in their own order of operations, on the cases of tests/gradient_cases.py.

No comparison here carries a relative or absolute tolerance.  Each kernel is compared with the restatement fed the device's own
upstream outputs.  R2, smoothing, Mean, the coarsened smoothing and the filters: bit for bit (NaN by position, everything else as
uint64).  G3, G2 and c, which pass through the device's hypot: inside the bracket of gradients_exact.LocalBracket, two float64
spacings either side of the longdouble hypot (the project's bound of 1.5 ulp on the device's hypot), carried
through the monotone rest of the kernel as plain float64 comparisons; on the interior of the Pythagorean ramps, where every
hypot is exact, bit for bit.  Every output starts as a finite sentinel, so a pixel that is never written shows.  The largest
distance of G3, G2 and c from the centre restatement is printed as a record (`-s`), not asserted."""
import numpy as np
import pytest

import filter_cases as fc
import gradient_cases as gc
import gradients_exact as gx
from xsarsea_amd import _lib, gradients
from xsarsea_amd._raster import _Call

pytestmark = pytest.mark.gpu
SENTINEL = -7.0  # finite, negative and no value any of these kernels can produce next to its neighbours unnoticed
DTYPE_IDS = ["float32", "float64"]
ROUTES = pytest.mark.parametrize("device", [False, True], ids=["numpy", "tensor"])


def to_numpy(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def raw(name, head, tail, inputs, outs, device):
    """ctx.<name>(*head, mem, *tail, *inputs, *outputs): inputs host arrays (None passes as NULL), outs a list of
    (shape, dtype) or None (a NULL output); every output pre-filled with the sentinel.  Returns the outputs as numpy arrays."""
    arrays = [None if a is None else np.array(a) for a in inputs]  # the cases are read-only
    if device:
        import torch
        arrays = [None if a is None else torch.from_numpy(a).cuda() for a in arrays]
    call = _Call(*[a for a in arrays if a is not None])
    assert call.device == device
    bufs = []
    for o in outs:
        if o is None:
            bufs.append(None)
            continue
        b = call.empty(*o)
        fill = SENTINEL * (1 + 1j) if np.dtype(o[1]).kind == "c" else SENTINEL
        b.fill_(fill) if device else b.fill(fill)
        bufs.append(b)
    call.launch(name, *head, call.mem, *tail, *arrays, *bufs)
    return [None if b is None else to_numpy(b) for b in bufs]


def xsw_dtype(dtype):
    return _lib.XSW_F32 if dtype == np.float32 else _lib.XSW_F64


def assert_bits(got, want, label):
    assert gx.same_bits(got, want), f"{label}: differs from the restatement in its own order " \
        f"({int((np.isnan(got) != np.isnan(want)).sum())} NaN positions, " \
        f"{int((~np.isnan(want) & ~np.isnan(got) & (got != want)).sum())} values)"


# ------------------------------------------------------------------------------------------------------- k_grad_r2
@ROUTES
@pytest.mark.parametrize("dtype", gc.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", gc.SIGMA0_NAMES)
def test_r2_bit_for_bit(name, dtype, device):
    """xsw_grad_r2 with take_sqrt 0 and 1 and xsw_grad_r2_sqrt; the public R2 is the raw entry."""
    s0 = gc.sigma0(name, dtype)
    L, S = s0.shape
    out = [((L // 2, S // 2), np.float64)]
    for take_sqrt in (0, 1):
        got, = raw("grad_r2_raw", (L, S, xsw_dtype(dtype)), (take_sqrt,), [s0], out, device)
        assert_bits(got, gc.r2_want(name, dtype, False, bool(take_sqrt)), f"{name} take_sqrt {take_sqrt}")
    got, = raw("grad_r2_sqrt_raw", (L, S, xsw_dtype(dtype)), (), [s0], out, device)
    assert_bits(got, gc.r2_want(name, dtype, True, False), f"{name} root on load")
    if not device:
        assert_bits(gradients.R2(np.array(s0)), gc.r2_want(name, dtype, False, False), f"{name} public R2")


# ---------------------------------------------------------------------------------------------------- k_grad_local
def local_raw(entry, x, dtype, with_g2, device):
    L, S = x.shape
    shape = (L // 2, S // 2)
    outs = [(shape, np.complex128) if with_g2 else None, (shape, np.float64), (shape, np.float64)]
    head = (L, S, xsw_dtype(dtype)) if entry == "grad_local_sqrt_raw" else (L, S)
    return raw(entry, head, (), [x], outs, device)


def record(label, b, G2, G3, c):
    print(f"distance from the centre restatement, spacings: {label}: " + ", ".join(f"{k} {v}" for k, v in b.distances(G2, G3, c).items()))


@ROUTES
@pytest.mark.parametrize("dtype", gc.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", gc.SIGMA0_NAMES)
def test_local_inside_the_bracket(name, dtype, device):
    """xsw_grad_local on ampl = sqrt(sigma0) and xsw_grad_local_sqrt on sigma0, the latter with and without g2: each inside the
    bracket, and all three the same bits (one kernel body, the same loaded values).  xsw_grad_local without g2 is refused
    before any launch."""
    b = gc.local_bracket(name, dtype)
    s0, am = gc.sigma0(name, dtype), gc.ampl(name, dtype)
    G2, G3, C = local_raw("grad_local_raw", am, np.float64, True, device)
    assert b.problems(G2, G3, C) == []
    record(f"{name} {np.dtype(dtype).name}", b, G2, G3, C)
    G2s, G3s, Cs = local_raw("grad_local_sqrt_raw", s0, dtype, True, device)
    assert b.problems(G2s, G3s, Cs) == []
    assert gx.same_bits(G2s, G2) and gx.same_bits(G3s, G3) and gx.same_bits(Cs, C)
    _none, G3n, Cn = local_raw("grad_local_sqrt_raw", s0, dtype, False, device)
    assert gx.same_bits(G3n, G3) and gx.same_bits(Cn, C)
    with pytest.raises(_lib.XswError, match="bad argument"):
        local_raw("grad_local_raw", am, np.float64, False, device)
    if not device:
        lg = gradients.local_gradients(np.array(am))
        assert gx.same_bits(lg.G2, G2) and gx.same_bits(lg.G3, G3) and gx.same_bits(lg.c, C)


@ROUTES
@pytest.mark.parametrize("name", gc.RAMP_NAMES)
def test_ramps(name, device):
    """The Pythagorean ramps: inside the bracket everywhere and, on the interior, the exact integers: G2 = (|dx|, dy sign(dx)),
    G3 = dx**2 + dy**2 and, at k = 2**20, c = 1.0, which is kept."""
    am, b, interior = gc.ramp(name)
    G2, G3, C = local_raw("grad_local_raw", am, np.float64, True, device)
    exact_hypot = gx.same_bits(G3[interior], b.za[interior])
    print(f"{name}: the device's hypot was {'exact' if exact_hypot else 'NOT exact'} on the interior's Pythagorean pairs; "
          f"c there {[repr(float(v)) for v in np.unique(C[interior])]}")
    assert b.problems(G2, G3, C, exact=interior) == []
    record(name, b, G2, G3, C)


# --------------------------------------------------------------------------------------- k_grad_mean / k_grad_smooth
MEAN_CASES = [(g, False) for g in fc.SMOOTH_GRIDS] + [(g, True) for g in fc.BIG_GRIDS]


@ROUTES
@pytest.mark.parametrize("grid,nan_edges", MEAN_CASES, ids=lambda v: "nan_edges" if v is True else "" if v is False else f"{v[0]}x{v[1]}")
def test_mean_and_smoothing_bit_for_bit(grid, nan_edges, device):
    x = fc.mean_input(grid, nan_edges)
    out = [(grid, np.float64)]
    got, = raw("grad_smooth_raw", grid, (False,), [x], out, device)
    assert_bits(got, gx.smooth_exact(x), f"smoothing {grid}")
    if grid in fc.MEAN_GRIDS:
        got, = raw("grad_mean_raw", grid, (), [x], out, device)
        assert_bits(got, gx.mean_exact(x), f"Mean {grid}")
    if not device:
        assert_bits(gradients.smoothing(np.array(x)), gx.smooth_exact(x), f"public smoothing {grid}")
        assert_bits(gradients.Mean(np.array(x)), gx.mean_exact(x), f"public Mean {grid}")


def test_mean_zero_taps_multiply():
    """One +inf: the zero taps of w9 turn its 13 x 13 footprint into NaN but for the four corners (without them all of it would
    be +inf)."""
    x = gc.inf_input()
    want = gx.mean_exact(x)
    assert np.isnan(want).sum() == 165 and np.isinf(want).sum() == 4
    for device in (False, True):
        got, = raw("grad_mean_raw", x.shape, (), [x], [(x.shape, np.float64)], device)
        assert_bits(got, want, "Mean of one inf")


@ROUTES
@pytest.mark.parametrize("shape", fc.COARSEN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coarsened_smoothing_bit_for_bit(shape, device):
    x, _want = fc.coarsen_input(shape)
    got, = raw("grad_smooth_raw", shape, (True,), [x], [((shape[0] // 2, shape[1] // 2), np.float64)], device)
    assert_bits(got, gx.smooth_exact(x, True), f"coarsened smoothing {shape}")


# ---------------------------------------------------------------------------------------------------- k_grad_filter
def raw_filter(t, device):
    L, S = t["r2"].shape
    got, = raw("grad_filter_raw", (L, S), (), [t["r2"], t["g3"], t["c"], t["q4"]], [((5, L, S), np.float64)], device)
    return got


@ROUTES
@pytest.mark.parametrize("case", gc.FILTER_CASES, ids=gc.filter_id)
def test_raw_filter_bit_for_bit(case, device):
    """The designed inputs of tests/filter_cases.py, inside the ramp of every filter, and their NaN variants."""
    t = fc.designed(*case)
    assert_bits(raw_filter(t, device), gc.filter_exact_of(t), f"filter {gc.filter_id(case)}")


@ROUTES
@pytest.mark.parametrize("grid", gc.NOISE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_raw_filter_sign_noise(grid, device):
    """J1 - J**2 is rounding noise of both signs: f1 and F are NaN exactly where the restatement's difference is negative."""
    t, want = gc.noise_inputs(grid), gc.noise_want(grid)
    got = raw_filter(t, device)
    np.testing.assert_array_equal(np.isnan(got[0]), np.isnan(want[0]))
    assert_bits(got, want, f"filter noise {grid}")


# -------------------------------------------------------------------------------------------------------- the chain
@ROUTES
@pytest.mark.parametrize("dtype", gc.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", gc.CHAIN_NAMES)
def test_chain_stage_by_stage(name, dtype, device):
    """filtering_parameters as its four raw entries, each stage compared with the restatement fed the DEVICE's outputs of the
    stages before it; the public call equals the composition bit for bit."""
    s0 = gc.sigma0(name, dtype)
    L, S = s0.shape
    L2, S2 = L // 2, S // 2
    r2, = raw("grad_r2_sqrt_raw", (L, S, xsw_dtype(dtype)), (), [s0], [((L2, S2), np.float64)], device)
    assert_bits(r2, gc.r2_want(name, dtype, True, False), f"{name} r2")
    _none, g3, c = local_raw("grad_local_sqrt_raw", s0, dtype, False, device)
    assert gc.local_bracket(name, dtype).problems(None, g3, c) == []
    q4, = raw("grad_smooth_raw", (L2, S2), (True,), [r2], [((L2 // 2, S2 // 2), np.float64)], device)
    assert_bits(q4, gx.smooth_exact(r2, True), f"{name} q4")
    t = dict(r2=r2, g3=g3, c=c, q4=q4)
    out = raw_filter(t, device)
    assert_bits(out, gc.filter_exact_of(t), f"{name} filters")
    if device:
        import torch
        res = gradients.filtering_parameters(torch.from_numpy(np.array(s0)).cuda())
    else:
        res = gradients.filtering_parameters(np.array(s0))
    assert gx.same_bits(np.stack([to_numpy(r) for r in res]), out), f"{name}: the public call differs from its raw entries"
