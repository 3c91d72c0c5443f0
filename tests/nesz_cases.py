"""The rasters at which tests/test_gpu_nesz_chain.py holds the noise flattening (csrc/xsw_nesz.hpp) to tests/nesz_chain_ref.py, and
what each of them is for; tests/test_nesz_chain_cpu.py builds every one, so the assertions below run without a GPU.  Numpy only.

The base recipe makes every line and every column matter (on the smooth rasters of the older tests a dropped line or sample
moves the result by less than their tolerance):
    incidence   20 + 25 s / (S - 1) + d[l], d uniform in +-1.5 degrees per line
    noise (dB)  -31 + 0.1 (inc - 20) + g[l] + c[s] + N(0, 0.4), g a per-line gain in +-3 dB, c a per-column gain in +-2 dB
    30 % of the noise pixels and 10 % of the incidence pixels are NaN; every incidence column keeps one finite pixel (a NaN
    column mean there would make every line that fits a sample of it a NaN line: that is a branch case of its own).
Drawn in float64 and cast last: the float32 case holds the float64 case's values rounded.

  samples_S    11 x S (two colsum blocks of 6 and 5 lines), S over the boundaries of k_nesz_fit and k_nesz_center (EXPECT_SAMPLES
               writes down threads and waves that hold a sample, trips, tail samples).  S = 1: one fitted point per line, the
               minimum-norm branch; S = 2 has no NaN: the exact two-point fit
  lines_LxS    S = 130 and 131, L over the line-block rule and L % XSW_NESZ_LINES (EXPECT_LINES writes down (nb, lpb, last))
  tall_blocks  147 x 65540: nb = 15, lpb = 10, last block 7 -- every block runs two unrolled groups of k_nesz_colsum and two tail
               lines, the last one group and three; 129 trips of the fit loop, 65 of k_nesz_center, five lines per eval block
  branch cases 8 x 300 unless said (BRANCH; float32 only: F32_ONLY).

Every case carries the reference, the restatement, R and the bound, computed once and read-only.  What keeps a test from hiding
a failure: every pixel where the reference is finite is compared; NaN positions must be equal (asserted here between reference
and restatement); every finite exact value is a normal number of the output format (asserted: nothing is excluded as outside
the range); in the sweep cases and tall_blocks at least 99 % of the pixels are finite."""
import functools
from collections import namedtuple

import numpy as np

import nesz_chain_ref as ref

Case = namedtuple("Case", "name dtype noise inc ref rst R bound kind")

SWEEP_L = 11
SAMPLES = (1, 2, 3, 63, 64, 65, 127, 129, 255, 256, 257, 511, 512, 513, 1023, 1025, 2049)
LINES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
LINES_S = (130, 131)
TALL = (147, 65540)
BRANCH = ("nan_noise_column", "nan_noise_pair", "nan_noise_line", "nan_raster", "lone_sample", "two_samples", "const_inc_6", "const_inc_300",
          "nan_inc_column", "inf_noise")
F32_ONLY = ("denormal",)

# S: (threads of k_nesz_fit that hold a sample, waves that do, trips of its group loop, tail samples, trips of k_nesz_center) with
# groups of V = 2 samples, 256 threads (both dtypes: XSW_NESZ_F32_GROUP == 2)
EXPECT_SAMPLES = {1: (1, 1, 0, 1, 1), 2: (1, 1, 1, 0, 1), 3: (1, 1, 1, 1, 1), 63: (31, 1, 1, 1, 1), 64: (32, 1, 1, 0, 1), 65: (32, 1, 1, 1, 1),
                  127: (63, 1, 1, 1, 1), 129: (64, 1, 1, 1, 1), 255: (127, 2, 1, 1, 1), 256: (128, 2, 1, 0, 1), 257: (128, 2, 1, 1, 1),
                  511: (255, 4, 1, 1, 1), 512: (256, 4, 1, 0, 1), 513: (256, 4, 1, 1, 1), 1023: (256, 4, 2, 1, 1), 1025: (256, 4, 2, 1, 2),
                  2049: (256, 4, 4, 1, 3)}
# L: (nb, lpb, lines of the last block) of nesz_blocks at S = 130 / 131
EXPECT_LINES = {1: (1, 1, 1), 2: (1, 2, 2), 3: (1, 3, 3), 4: (1, 4, 4), 5: (1, 5, 5), 7: (1, 7, 7), 8: (1, 8, 8), 9: (2, 5, 4), 15: (2, 8, 7),
                16: (2, 8, 8), 17: (3, 6, 5), 33: (5, 7, 5)}


def sweep_names():
    return [f"samples_{s}" for s in SAMPLES] + [f"lines_{l}x{s}" for s in LINES_S for l in LINES]


def names(dtype):
    """Every case of `dtype` but tall_blocks."""
    return sweep_names() + list(BRANCH) + (list(F32_ONLY) if np.dtype(dtype) == np.float32 else [])


def _rng(name):
    return np.random.default_rng(list(name.encode()))


def base(name, lines, samples, nan=True):
    """(noise, inc) of the module docstring in float64."""
    rng = _rng(name)
    d, g, c = rng.uniform(-1.5, 1.5, lines), rng.uniform(-3.0, 3.0, lines), rng.uniform(-2.0, 2.0, samples)
    ramp = 25.0 * np.arange(samples) / (samples - 1) if samples > 1 else np.zeros(1)
    inc = 20.0 + ramp[None, :] + d[:, None]
    db = -31.0 + 0.1 * (inc - 20.0) + g[:, None] + c[None, :] + rng.normal(0.0, 0.4, (lines, samples))
    noise = 10.0 ** (db / 10.0)
    hole_n, hole_i = rng.random((lines, samples)) < 0.3, rng.random((lines, samples)) < 0.1
    if nan:
        full = np.flatnonzero(hole_i.all(axis=0))
        hole_i[full % lines, full] = False
        noise[hole_n] = np.nan
        inc[hole_i] = np.nan
    return noise, inc


def _finish(name, dtype, noise, inc, kind):
    dtype = np.dtype(dtype)
    noise, inc = np.ascontiguousarray(noise, dtype=dtype), np.ascontiguousarray(inc, dtype=dtype)
    r = ref.reference(noise, inc)
    rst = ref.restate(noise, inc)
    R = ref.line_error(rst.out, r)
    bnd = ref.bound(r, dtype, R)
    for a in (noise, inc, rst.out, R, bnd):
        a.setflags(write=False)
    finite = np.isfinite(r.out)
    assert np.array_equal(np.isnan(r.out), np.isnan(rst.out)), f"{name}: reference and restatement disagree on the NaN positions"
    assert np.array_equal(finite, ~np.isnan(r.out)), f"{name}: an exact value is infinite"
    fi = np.finfo(dtype)  # float32 rasters: v_exp_f32 returns float32
    assert (r.out[finite] >= fi.tiny).all() and (r.out[finite] <= fi.max).all(), f"{name}: an exact value is no normal number of the output format"
    assert np.isfinite(bnd[finite]).all() and (bnd[finite] > 0).all(), name
    if kind in ("samples", "lines", "tall"):
        assert finite.mean() >= 0.99, f"{name}: only {finite.mean():.3f} of the pixels are finite"
    return Case(name, dtype, noise, inc, r, rst, R, bnd, kind)


# ---------------------------------------------------------------------------------------------------------------- the sweeps
def _samples_case(name, dtype):
    S = int(name.split("_")[1])
    noise, inc = base(name, SWEEP_L, S, nan=S != 2)
    c = _finish(name, dtype, noise, inc, "samples")
    la = c.rst.launch
    assert la["blocks"] == (2, 6, 5), name
    assert (la["fit_threads"], la["fit_waves"], la["fit_trips"], la["fit_tail"], la["center_trips"]) == EXPECT_SAMPLES[S], (name, la)
    assert la["V"] == 2 and la["fit_groups_of_lines"] == 3 and la["lines_mod"] == 3
    if S == 1:
        assert (c.ref.n == 1).all() and c.ref.minnorm.all() and not c.rst.regular.any() and (c.rst.n == 1).all(), name
    elif S == 2:  # the exact two-point fit: the line passes through both points
        assert (c.ref.n == 2).all() and not c.ref.minnorm.any() and c.rst.regular.all()
        _passes_through(c, np.repeat(np.arange(SWEEP_L), 2), np.tile([0, 1], SWEEP_L))
    else:
        assert not c.ref.minnorm.any() and c.rst.regular.all() and np.array_equal(c.ref.n, c.rst.n), name
    return c


def _passes_through(c, ls, ss):
    want = c.noise[ls, ss].astype(ref.LD) * np.power(ref.LD(10), ref.LD(-1) / ref.LD(10))
    err = np.abs((c.ref.out[ls, ss] - want) / want).astype(np.float64)
    assert (err < 1e-16).all(), (c.name, err.max())


def _lines_case(name, dtype):
    L, S = (int(v) for v in name.split("_")[1].split("x"))
    noise, inc = base(name, L, S)
    c = _finish(name, dtype, noise, inc, "lines")
    la = c.rst.launch
    R = ref.constants()[0]
    assert R == 4 and la["blocks"] == EXPECT_LINES[L] and la["lines_mod"] == L % R and la["fit_groups_of_lines"] == -(-L // R), (name, la)
    assert la["eval_grid"] == (1, L, 1, 1), (name, la)  # the write pass: one line per workgroup, one column strip
    assert la["fit_tail"] == S % 2 and la["fit_threads"] == 65
    assert np.array_equal(c.ref.n, c.rst.n) and (c.ref.n >= 60).all(), name
    return c


@functools.lru_cache(maxsize=1)
def tall_blocks(dtype):
    """147 x 65540, 9.6 Mpx: the one large case (held one dtype at a time)."""
    L, S = TALL
    noise, inc = base("tall_blocks", L, S)
    c = _finish("tall_blocks", dtype, noise, inc, "tall")
    la = c.rst.launch
    nb, lpb, last = la["blocks"]
    assert (nb, lpb, last) == (15, 10, 7), la
    assert lpb != 8 and (lpb // 4, lpb % 4) == (2, 2) and (last // 4, last % 4) == (1, 3)  # unrolled groups and tail lines of k_nesz_colsum
    assert la["fit_trips"] == 129 and la["fit_tail"] == 0 and la["center_trips"] == 65 and la["eval_grid"] == (129, 30, 5, 2), la
    return c


# ---------------------------------------------------------------------------------------------------------------- branch cases
def _branch_case(name, dtype):
    L, S = 8, 300
    dtype = np.dtype(dtype)
    if name in ("const_inc_6", "const_inc_300"):
        S = int(name.split("_")[2])
    if name == "two_samples":
        S = 301
    noise, inc = base(name, L, S)
    ordinary = np.ones(L, bool)  # lines that fit as usual
    if name == "nan_noise_column":
        noise[:, 17] = np.nan
    elif name == "nan_noise_pair":
        noise[:, 40:42] = np.nan
    elif name == "nan_noise_line":
        noise[5, :] = np.nan
    elif name == "nan_raster":
        noise[:, :] = np.nan
        ordinary[:] = False
    elif name == "lone_sample":
        noise[:, 6] = np.nan
        noise[3, :] = np.resize([0.0, -1.5, np.inf], S)
        noise[3, 6] = np.nan
        noise[3, 123] = 10.0 ** -2.9
        ordinary[3] = False
    elif name == "two_samples":
        for l, (a, b) in TWO_SAMPLES.items():
            noise[l, :] = 0.0
            noise[l, a], noise[l, b] = 10.0 ** -3.0, 10.0 ** (-2.7 if b - a > 1 else -2.998)  # (adjacent: a slope that stays in float32's range 25 degrees away)
            inc[:2, [a, b]] = 20.0 + 25.0 * np.array([a, b]) / (S - 1)  # the column means there are finite
            ordinary[l] = False
    elif name in ("const_inc_6", "const_inc_300"):
        inc[:, :] = 35.3
        ordinary[:] = False
    elif name == "nan_inc_column":
        inc[:, 9] = np.nan
        noise[4, 9] = 0.0
        noise[2, 9] = 10.0 ** -3.1  # the column mean of noise is positive: every other line fits a sample at column 9
        ordinary[:] = False
    elif name == "inf_noise":
        noise[2, 50], noise[5, 50], noise[6, 50] = np.inf, np.nan, 10.0 ** -3.0
    noise, inc = noise.astype(dtype), inc.astype(dtype)
    if name == "denormal":
        assert dtype == np.float32
        fi = np.finfo(np.float32)
        for l in (1, 6):
            noise[l, [10, 150, 299]] = np.array([1e-40, fi.smallest_subnormal * 3, fi.tiny / 2], np.float32)
    c = _finish(name, dtype, noise, inc, "branch")
    r, rst = c.ref, c.rst
    assert np.array_equal(r.n, rst.n), name
    assert not r.minnorm[ordinary].any() and rst.regular[ordinary].all() and (r.n[ordinary] >= 100).all() and np.isfinite(r.out[ordinary]).all(), name
    if name == "nan_noise_column":
        assert np.isnan(rst.mean[17]) and np.isfinite(r.out[:, 17]).all()
    elif name == "nan_noise_pair":
        assert 40 % rst.launch["V"] == 0 and np.isnan(rst.mean[40:42]).all() and np.isfinite(r.out[:, 40:42]).all()
    elif name == "nan_noise_line":
        assert np.isnan(c.noise[5]).all() and np.isfinite(r.out[5]).all() and r.n[5] == np.isfinite(rst.mean).sum() >= S - 2  # it fits the column means
    elif name == "nan_raster":
        assert np.isnan(r.out).all() and (r.n == 0).all()
    elif name == "lone_sample":
        assert r.n[3] == 1 and r.minnorm[3] and not rst.regular[3] and np.isfinite(r.out[3]).all() and np.isnan(rst.mean[6])
    elif name == "two_samples":
        for l, (a, b) in TWO_SAMPLES.items():
            assert r.n[l] == 2 and not r.minnorm[l] and rst.regular[l] and np.isfinite(r.out[l]).all(), (name, l)
            _passes_through(c, [l, l], [a, b])
        assert rst.launch["fit_tail"] == 1 and TWO_SAMPLES[6] == (S - 2, S - 1)
    elif name in ("const_inc_6", "const_inc_300"):
        assert (r.n > 1).all() and r.minnorm.all() and not rst.regular.any() and np.isfinite(r.out).all(), name
        assert (r.x == np.asarray(35.3, dtype).astype(ref.LD)).all()
    elif name == "nan_inc_column":
        others = np.arange(L) != 4
        assert np.isnan(r.out[others]).all() and np.isnan(r.out[4, 9]) and np.isfinite(np.delete(r.out[4], 9)).all() and r.n[4] == S - 1
    elif name == "inf_noise":
        assert np.isposinf(rst.mean[50]) and np.isfinite(r.out).all() and r.n[2] == S - 1 and r.n[5] == S - 1 and r.n[6] == S
    elif name == "denormal":
        tiny = (c.noise > 0) & (c.noise < np.finfo(np.float32).tiny)
        assert tiny.sum() == 6 and (r.n[[1, 6]] >= S - 2).all() and (r.ymax[[1, 6]] > 400).all()
    return c


# line: the two samples it fits (8 x 301; the others are 0): adjacent, far apart, and the fit loop's tail sample with its neighbour
# in the last group (column 300 is also k_nesz_eval's odd last column)
TWO_SAMPLES = {1: (100, 101), 3: (3, 290), 6: (299, 300)}


def case(name, dtype):
    """The case `name` for rasters of `dtype`, built once."""
    return tall_blocks(np.dtype(dtype)) if name == "tall_blocks" else _case(name, np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    if name.startswith("samples_"):
        return _samples_case(name, dtype)
    if name.startswith("lines_"):
        return _lines_case(name, dtype)
    assert name in BRANCH or (name in F32_ONLY and dtype == np.float32), name
    return _branch_case(name, dtype)
