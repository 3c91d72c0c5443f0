"""The 32 x 32 tile kernels of the rain filter (k_grad_mean, k_grad_filter) and k_grad_smooth on the MI355X against the CPU
restatement (tests/filtering_ref.py) on the seam shapes and in-ramp inputs of tests/filter_cases.py: axes of 32k - 1, 32k and
32k + 1, last tiles narrower than Mean's reach of 6, 1-, 2-, 3- and 5-pixel axes across 22 tiles, NaN on reflected edges and on
tile corners, k_grad_smooth around its 64- and 4-seams and over every valid-count of the 2 x 2 mean.

No tolerance of its own: Mean, smoothing and the coarsened smoothing hold the module's 1e-12 relative with equal NaN positions
(`assert_close_rel`), the filters the 1e-9 absolute of tests/test_gpu_filtering.py (`compare`, whose derivation assumes
P1 >= 0.035: the lower end of f1's ramp, which the designed inputs stay inside).  The raw filter entry runs on designed inputs
that sit inside the ramps on >= 99 % of the pixels, so that a wrong J, J1, G4 or zoom tap cannot hide on a plateau;
tests/test_filtering_cpu.py asserts those conditions, and that four wrong halos move the restatement itself by more than 1e3 ATOL on
seam pixels."""
import numpy as np
import pytest

import filter_cases as fc
import filtering_ref as fr
import test_gpu_filtering as base
from xsarsea_amd._raster import _Call
from xsarsea_amd.gradients import Mean, filtering_parameters, smoothing

pytestmark = pytest.mark.gpu
SENTINEL = -7.0  # finite and outside [0, 1]: an output pixel that was never stored fails `compare`


def grid_id(v):
    return "nan_edges" if v is True else "" if v is False else f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


MEAN_CASES = [(g, False) for g in fc.MEAN_GRIDS] + [(g, True) for g in fc.BIG_GRIDS]
SMOOTH_CASES = [(g, False) for g in fc.SMOOTH_GRIDS] + [(g, True) for g in fc.BIG_GRIDS]


def same_shape_filter(fn, x, want, label):
    import torch
    out = fn(x)
    assert isinstance(out, np.ndarray)
    print(label, end=": ")
    base.assert_close_rel(out, want, 1e-12)
    dev = fn(torch.from_numpy(np.array(x)).cuda())
    assert dev.is_cuda and dev.dtype == torch.float64
    np.testing.assert_array_equal(dev.cpu().numpy(), out)  # the two routes bit for bit, NaN included


@pytest.mark.parametrize("grid,nan_edges", MEAN_CASES, ids=grid_id)
def test_mean_on_seams(grid, nan_edges):
    same_shape_filter(Mean, fc.mean_input(grid, nan_edges), fc.mean_want(grid, nan_edges), f"Mean {grid}")


@pytest.mark.parametrize("grid,nan_edges", SMOOTH_CASES, ids=grid_id)
def test_smoothing_on_seams(grid, nan_edges):
    same_shape_filter(smoothing, fc.mean_input(grid, nan_edges), fc.smoothing_want(grid, nan_edges), f"smoothing {grid}")


def raw_call(name, head, arrays, out_shape, device):
    """ctx.<name>(*head[:2], mem, *head[2:], *arrays, out) as tests/test_gpu_gradients.py calls its raw entries, on host arrays or
    device tensors, with `out` pre-filled with the sentinel."""
    arrays = [np.array(a) for a in arrays]  # the cases are read-only
    if device:
        import torch
        arrays = [torch.from_numpy(a).cuda() for a in arrays]
    call = _Call(*arrays)
    assert call.device == device
    out = call.empty(out_shape, np.float64)
    out.fill_(SENTINEL) if device else out.fill(SENTINEL)
    call.launch(name, *head[:2], call.mem, *head[2:], *arrays, out)
    return out.cpu().numpy() if device else out


@pytest.mark.parametrize("shape", fc.COARSEN_SHAPES, ids=grid_id)
def test_smoothing_of_the_coarsened_raster(shape):
    """k_grad_smooth<true>: smoothing of the NaN-skipping 2 x 2 mean, every valid-count 0 .. 4 among the groups, odd axes trimmed."""
    x, want = fc.coarsen_input(shape)
    outs = []
    for device in (False, True):
        out = raw_call("grad_smooth_raw", (*shape, True), [x], want.shape, device)
        print(f"coarsen {shape} {'tensor' if device else 'numpy'}", end=": ")
        base.assert_close_rel(out, want, 1e-12)
        outs.append(out)
    np.testing.assert_array_equal(outs[0], outs[1])


def raw_filter(grid, which, phase, nan, label):
    t, want = fc.designed(grid, which, phase, nan), fc.designed_want(grid, which, phase, nan)
    L, S = grid
    outs = []
    for device in (False, True):
        out = raw_call("grad_filter_raw", (L, S), [t["r2"], t["g3"], t["c"], t["q4"]], (5, L, S), device)
        base.compare(list(out), want, f"{label} {'tensor' if device else 'numpy'}")
        outs.append(out)
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("phase", fc.PHASES, ids=["plus", "minus"])
@pytest.mark.parametrize("which", fc.SETS)
@pytest.mark.parametrize("grid", fc.RAW_GRIDS, ids=grid_id)
def test_raw_filter_inside_the_ramps(grid, which, phase):
    """xsw_grad_filter on the designed inputs, host and device memory: f1 (set A), f2 (set B), f4 and, over the two phases, f3
    are inside their ramps on >= 99 % of the pixels, so every J, J1, G4 and zoom tap shows in the comparison."""
    raw_filter(grid, which, phase, None, f"raw {grid} set {which} phase {phase:+d}")


@pytest.mark.parametrize("which,nan", fc.NAN_CASES, ids=[f"{w}-{n}" for w, n in fc.NAN_CASES])
@pytest.mark.parametrize("grid", fc.BIG_GRIDS, ids=grid_id)
def test_raw_filter_single_nan(grid, which, nan):
    """One NaN in r2 at the corner of four tiles (or the grid's nearest seam corner), in g3 on the raster's last row, or in q4's
    last column: the NaN positions of every field are the restatement's."""
    raw_filter(grid, which, 1, nan, f"raw {grid} set {which} NaN in {nan}")


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape,nan_edges", fc.CHAIN_CASES, ids=grid_id)
def test_chain_on_seam_scenes(shape, nan_edges, dtype, device):
    """filtering_parameters on sigma0 scenes whose half-resolution grids are the seam shapes; each has at least 16 seam pixels
    inside every filter's ramp (without nan_edges), asserted on the restatement."""
    s0 = np.array(fc.chain_scene(shape, dtype, nan_edges))
    want = fc.chain_want(shape, dtype, nan_edges)
    line, sample = np.arange(shape[0]) * 10.0 + 5, np.arange(shape[1]) * 10.0 + 5
    if device:
        import torch
        res = filtering_parameters(torch.from_numpy(s0).cuda(), line=line, sample=sample)
        assert all(r.is_cuda and r.dtype == torch.float64 for r in res)
    else:
        res = filtering_parameters(s0, line=line, sample=sample)
        assert all(isinstance(r, np.ndarray) for r in res)
    assert len(res) == 5
    np.testing.assert_array_equal(res.line, fr.coarsen_coords(line, 2))
    np.testing.assert_array_equal(res.sample, fr.coarsen_coords(sample, 2))
    label = f"chain {shape}{' nan_edges' if nan_edges else ''} {np.dtype(dtype).name} {'tensor' if device else 'numpy'}"
    base.compare(list(res), want, label)
