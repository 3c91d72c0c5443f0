"""xsarsea_amd.streaks on the MI355X against the CPU restatement (tests/streaks_ref.py).  Each stage is compared on ONE input:
the device-produced histograms are copied to the host and given to the restatement, so the histograms' own tolerance does not
stack on top of the stage's.  Host route against device route, resolve and the raster pass on hand-built fields, one full-size
raster against a torch restatement, and the whole chain sigma0 -> wind on a user stream."""
import warnings

import numpy as np
import pytest

import gradients_ref as ref
import streak_cases as sc
import streaks_ref as sref
import strip_shapes
from test_gpu_gradients import LINE, SAMPLE, scene
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import ASYNC, _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from util import bits_equal
from xsarsea_amd import _lib, gradients, streaks

pytestmark = pytest.mark.gpu
BINS = ref.angles_bins(72)
NAN = complex(np.nan, np.nan)


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def compare_streaks(s, W, R, angles, smooth, orthogonal, what):
    """Device result against the restatement on the same histograms: index equal at every window; weight, used_ratio and angle
    bit-equal (NaN included).  The restatement adds in the kernel's order (the mean in axis order with one division, every
    smoothing pass from 0 over all its taps in ascending order), the kernel is built without contractions and calls no library
    function, so nothing allows a difference in bits and no window is excused."""
    W, R = host(W), host(R)
    want = sref.streaks_direction(W, R, angles, smooth=smooth, orthogonal=orthogonal)
    index = host(s.index)
    assert index.dtype == np.int32
    np.testing.assert_array_equal(index, want["index"], err_msg=what)
    assert bits_equal(host(s.weight), want["weight"]), what + " weight"
    assert bits_equal(host(s.used_ratio), want["used_ratio"]), what + " used_ratio"
    assert bits_equal(host(s.angle), want["angle"]), what + " angle"
    assert bits_equal(host(s.angle), (angles + (np.pi / 2 if orthogonal else 0))[want["index"]]), what + " angle from the table"
    return want


@pytest.mark.parametrize("smooth,orthogonal", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("seed,dtype,step", [(21, np.float32, 0.5), (22, np.float64, 1)])
def test_streaks_direction_matches_the_restatement(seed, dtype, step, smooth, orthogonal):
    s0 = scene((1203, 1597), dtype, seed)
    h = gradients.Gradients(s0, windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=step, line=LINE, sample=SAMPLE).histogram
    s = streaks.streaks_direction(h, smooth=smooth, orthogonal=orthogonal)
    assert isinstance(s.angle, np.ndarray) and s.angle.shape == h.weight.shape[2:4] and s["index"] is s.index
    np.testing.assert_array_equal(s.line, h.line)
    np.testing.assert_array_equal(s.sample, h.sample)
    compare_streaks(s, h.weight, h.used_ratio, BINS, smooth, orthogonal, f"seed {seed} smooth {smooth}")


def test_hand_built_histograms_and_angle_counts():
    """Peaks at the first and last bin, an exact tie, all-NaN and all-zero windows, NaN in one configuration only; then other
    n_angles (8, 90, 360, 512: several bins per lane) and the bounds of the entry point."""
    rng = np.random.default_rng(30)
    W = np.zeros((3, 2, 4, 72))
    W[:, 0, 0, 0] = 1.0
    W[:, 0, 1, 71] = 2.0
    W[:, 0, 2, 10] = W[:, 0, 2, 50] = 1.0           # exact tie: the first index
    W[:, 0, 3] = np.nan                               # all NaN
    W[:, 1, 1] = rng.uniform(0, 1, (3, 72))
    W[1, 1, 1] = np.nan                               # one configuration NaN: skipped
    W[:, 1, 2] = rng.uniform(0, 1, (3, 72))
    W[2, 1, 2, 7] = np.nan                            # one bin of one configuration
    W[:, 1, 3] = rng.uniform(0, 1, 72)[None] * np.array([1.0, 2.0, 4.0])[:, None]
    R = rng.uniform(0, 1, (3, 2, 4))
    R[:, 0, 3] = np.nan
    R[1, 1, 1] = np.nan
    for smooth in (True, False):
        s = streaks.streaks_direction(W, smooth=smooth, angles=BINS)
        want = sref.streaks_direction(W, np.full(R.shape, np.nan), BINS, smooth=smooth)
        np.testing.assert_array_equal(s.index, want["index"])
        assert list(s.index[0]) == [0, 71, 10, 0] and np.isnan(s.weight[0, 3]) and np.isnan(s.used_ratio).all()
        assert bits_equal(s.weight, want["weight"]), "hand-built weight"
        assert bits_equal(s.angle, want["angle"]), "hand-built angle"
    h = gradients.GradientsHistogram(W, R, BINS, np.arange(2) * 100.0, np.arange(4) * 50.0, ("c", "line", "sample", "angles"))
    s = streaks.streaks_direction(h)
    compare_streaks(s, W, R, BINS, True, True, "hand-built, with used_ratio")
    assert s.line[1] == 100.0 and s.sample[3] == 150.0
    for n in (8, 12, 90, 360, 512):
        Wn = rng.uniform(0, 1, (2, 3, 5, n))
        Wn[0, 1, 2, n - 1] = 5.0
        bins = ref.angles_bins(n)
        for smooth in (True, False):
            s = streaks.streaks_direction(Wn, smooth=smooth, angles=bins)
            # 8 bins: the passes at reach 1, 2 and 4 average all of them, the smoothed histogram is flat and rounding decides the
            # peak: in the restatement's order, which is the kernel's, so these windows are asserted like the others
            want = compare_streaks(s, Wn, np.full((2, 3, 5), np.nan), bins, smooth, True, f"n_angles {n} smooth {smooth}")
            assert bits_equal(s.weight, np.take_along_axis(want["m"], s.index[..., None].astype(np.int64), -1)[..., 0]), f"n_angles {n}, own peak"
    for n in (7, 513):
        with pytest.raises(_lib.XswError):
            streaks.streaks_direction(np.zeros((1, 1, n)), angles=ref.angles_bins(n))


def test_host_route_equals_device_route(torch):
    s0 = scene((603, 797), np.float32, 23)
    kw = dict(windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=0.5, line=LINE[:603], sample=SAMPLE[:797])
    rng = np.random.default_rng(24)
    anc = (rng.normal(0, 5, s0.shape) + 1j * rng.normal(0, 5, s0.shape))
    anc[100:140, 300:420] = NAN
    hh = gradients.Gradients(s0, **kw).histogram
    sh = streaks.streaks_direction(hh)
    dh = sh.resolve(anc, LINE[:603], SAMPLE[:797], min_used_ratio=0.3)
    oh = streaks.ancillary_from_streaks(sh, anc, LINE[:603], SAMPLE[:797], min_used_ratio=0.3)
    assert isinstance(oh, np.ndarray) and oh.dtype == np.complex128 and oh.shape == s0.shape
    P = torch.cuda.Stream()
    with torch.cuda.stream(P):
        hd = gradients.Gradients(torch.from_numpy(s0).cuda(), **kw).histogram
        sd = streaks.streaks_direction(hd)
        anc_d = torch.from_numpy(anc).cuda()
        dd = sd.resolve(anc_d, LINE[:603], SAMPLE[:797], min_used_ratio=0.3)
        od = streaks.ancillary_from_streaks(sd, anc_d, LINE[:603], SAMPLE[:797], min_used_ratio=0.3)
        assert od.is_cuda and od.dtype == torch.complex128 and sd.index.dtype == torch.int32
        got = [host(t) for t in (sd.index, sd.angle, sd.weight, sd.used_ratio, dd, od)]
    for g, w, name in zip(got, (sh.index, sh.angle, sh.weight, sh.used_ratio, dh, oh), ("index", "angle", "weight", "used_ratio", "resolve", "ancillary")):
        assert bits_equal(g, w), name
    assert np.isnan(dh.real).any() and not np.isnan(dh.real).all()


def test_resolve_signs_and_values_bit_equal():
    """Fields that include exact +-pi/2, a zero dot product, NaN and zero a-priori winds and both thresholds; the a-priori wind as
    a windows-shaped array and as a raster with float coordinates (nearest pixel, ties to the larger coordinate)."""
    table = np.array([0.0, np.pi / 2, -np.pi / 2, 0.3, 2.5, -1.1, np.pi, 1e-3])
    rng = np.random.default_rng(31)
    index = rng.integers(0, len(table), (6, 9)).astype(np.int32)
    index[0, :5] = [0, 0, 1, 2, 0]
    a = rng.normal(0, 4, index.shape) + 1j * rng.normal(0, 4, index.shape)
    a[0, :5] = [5j, -5j, 2j, 2j, -1 + 5j]  # zero dot products (kept), +-pi/2 against +2j, a negative dot product
    a[1, 0], a[1, 1], a[1, 2] = 0, complex(np.nan, 1), complex(1, np.nan)
    weight, ratio = rng.uniform(0, 1, index.shape), rng.uniform(0, 1, index.shape)
    weight[2, 3] = np.nan
    s = streaks.Streaks(table[index], weight, ratio, index, np.arange(6) * 10.0, np.arange(9) * 10.0, table)
    for kw in ({}, dict(min_weight=0.3), dict(min_used_ratio=0.5), dict(min_weight=float(weight[3, 3]), min_used_ratio=float(ratio[4, 4]))):
        got = s.resolve(a, **kw)
        want = sref.resolve(table[index], weight, ratio, a, **kw)
        assert bits_equal(got, want), kw
        np.testing.assert_array_equal(np.signbit(got.real), np.signbit(want.real))
    got = s.resolve(a)
    assert got[0, 0] == 1 and got[0, 1] == 1 and got[0, 4] == -1 and got[0, 2] == np.exp(0.5j * np.pi) and got[0, 3] == -np.exp(-0.5j * np.pi)
    assert np.isnan(got[1, :3].real).all() and np.isnan(got[2, 3].real)
    assert not np.isnan(s.resolve(a, min_weight=float(weight[3, 3]))[3, 3].real)  # equality passes the threshold
    assert np.isnan(s.resolve(a, min_weight=float(np.nextafter(weight[3, 3], 2)))[3, 3].real)
    # a raster: irregular float coordinates, window centres between pixels and outside the raster
    line, sample = np.cumsum(rng.uniform(0.5, 3, 40)), np.cumsum(rng.uniform(0.5, 3, 57))
    s.line, s.sample = np.linspace(line[0] - 2, line[-1] + 2, 6), np.linspace(sample[0], sample[-1], 9)
    s.line[2] = (line[10] + line[11]) / 2  # a tie (when the midpoint is exact) or its neighbourhood
    raster = rng.normal(0, 4, (40, 57)) + 1j * rng.normal(0, 4, (40, 57))
    got = s.resolve(raster, line, sample)
    want = sref.resolve(table[index], weight, ratio, sref.at_windows(raster, line, sample, s.line, s.sample))
    assert bits_equal(got, want)
    s2 = streaks.Streaks(table[index], weight, ratio, None, s.line, s.sample)  # no peak bins: exp(1j angle) directly
    assert bits_equal(s2.resolve(raster, line, sample), want)


def field(rng, nl, ns, holes=True):
    """Resolved unit vectors with NaN windows, opposite neighbours and one all-NaN bracket."""
    d = np.exp(1j * rng.uniform(-np.pi, np.pi, (nl, ns)))
    if holes:
        d[rng.random((nl, ns)) < 0.2] = NAN
        if nl > 2 and ns > 3:
            d[:2, :2] = NAN
            d[-1, -2], d[-1, -1] = 1j, -1j  # exactly opposite: they cancel half-way
    return d


def raster(rng, shape):
    a = rng.normal(0, 6, shape) + 1j * rng.normal(0, 6, shape)
    a[rng.random(shape) < 0.01] = NAN
    a[rng.random(shape) < 0.01] = complex(np.nan, 2.0)
    a[rng.random(shape) < 0.01] = 0
    return a


# The raster pass cannot be held to the bit: its two moduli are the device library's double hypot, whose rounding is its own.
# Everything else is: the blend sums (four corners in a stated order, tests/streaks_ref.py::blend_sums), one product, one quotient.
# So each component is compared with the same finish done in np.longdouble on those sums (sref.ancillary_exact), in ulps of
# that component: K = 2 h + 1 + 1, for two hypot calls of at most h ulp each, the product and the quotient of half an ulp
# each, and one ulp of slack.  h is measured, the library's accuracy table not being shipped with it: the device's hypot against
# the longdouble value on every (vx, vy) and (a.re, a.im) of the blend pixels of the nine cases below (HYPOT_PAIRS pairs) is off
# by at most HYPOT_ULP_MEASURED ulp, which h rounds up to the next half ulp.  (glibc's hypot stays within 0.56 ulp on the same
# pairs, and numpy's own finish of the restatement within 2.8 ulp of the longdouble one.)
#
# Measured on the MI355X, worst error of a component in ulps of that component, per case: odd 3.17, one_row 2.38, one_window 1.31,
# irregular 2.88, dense 2.82, wide 3.44, dense_blocks 3.81 (16.4 million components), small_components 2.85, closed_form 1.32;
# tests/test_gpu_masked_gradients.py's masked chain 3.39.  No component below the smallest normal float64 in any of them.
HYPOT_PAIRS = 19265848
HYPOT_ULP_MEASURED = 1.1938
HYPOT_ULP = 1.5
K_ULP = 2 * HYPOT_ULP + 1 + 1   # 5


def check_ancillary(got, anc, geometry, what):
    """Every pixel in one of three classes: NaN positions equal; fallback pixels (the restated |v| is 0) bit-equal to a; every
    other pixel per component within K_ULP * spacing(|exact|) of the longdouble finish.  A component whose exact value is below
    the smallest normal float64 is held to K_ULP * 2**-1074 instead, and fewer than 1 in 1000 may be such (an exact zero is held
    to the bit and not counted, sref.ancillary_ulps).  Returns (fallback pixels, blend pixels)."""
    got = host(got)
    ex = sref.ancillary_exact(*geometry[:3], anc, *geometry[3:])
    assert sref.LONGDOUBLE_EPS < 2.0 ** -60, "np.longdouble is no wider than float64 here"
    assert (ex["nan"] ^ ex["fallback"] ^ ex["blend"]).all()
    np.testing.assert_array_equal(np.isnan(got.real), ex["nan"], err_msg=what)
    np.testing.assert_array_equal(np.isnan(got.imag), ex["nan"], err_msg=what)
    assert bits_equal(got[ex["fallback"]], anc[ex["fallback"]]), what + ": fallback pixels"
    worst, worst_tiny, n_tiny, n = sref.ancillary_ulps(got, ex)
    print(f"{what}: worst / K = {worst:.3f} / {K_ULP} = {worst / K_ULP:.3f} ulp of the component over {n} components; "
          f"{n_tiny} below the smallest normal (worst {worst_tiny:.3g} of 2**-1074); {int(ex['fallback'].sum())} fallback, {int(ex['nan'].sum())} NaN pixels")
    assert worst <= K_ULP, what
    assert worst_tiny <= K_ULP and n_tiny * 1000 < max(n, 1), what
    return int(ex["fallback"].sum()), int(ex["blend"].sum())


ANCILLARY_CASES = ["odd", "one_row", "one_window", "irregular", "dense", "wide", "dense_blocks"]


def ancillary_case(case):
    """(dirs, windows_line, windows_sample, anc, line, sample) of one case of the raster pass."""
    rng = np.random.default_rng(40)
    if case == "odd":  # odd sizes, regular centres that start inside the raster and end outside
        shape, wl, ws = (203, 317), np.arange(5) * 47.0 + 20, np.arange(8) * 45.0 + 11
        line, sample = np.arange(203.0), np.arange(317.0)
    elif case == "one_row":
        shape, wl, ws = (77, 129), np.array([30.0]), np.arange(4) * 40.0
        line, sample = np.arange(77.0), np.arange(129.0)
    elif case == "one_window":
        shape, wl, ws = (9, 70), np.array([3.0]), np.array([100.0])
        line, sample = np.arange(9.0), np.arange(70.0)
    elif case == "irregular":  # irregular centres, float-coordinate axes
        shape = (151, 263)
        line, sample = np.cumsum(rng.uniform(5, 15, 151)), np.cumsum(rng.uniform(5, 15, 263)) - 300.0
        wl, ws = np.sort(rng.uniform(line[0] - 50, line[-1] + 50, 7)), np.sort(rng.uniform(sample[0] - 50, sample[-1] + 50, 11))
        wl[3] = line[70]  # a centre exactly on a pixel
        wl = np.sort(wl)
    elif case == "dense":  # more centres than lines: the line bracket changes on every line
        shape, wl, ws = (33, 300), np.arange(80) * 0.5, np.arange(40) * 8.0
        line, sample = np.arange(33.0), np.arange(300.0)
    elif case == "dense_blocks":
        # nine lines per workgroup (tests/strip_shapes.py: two groups of XSW_STREAKS_LINES and one more line, two lines in the
        # last workgroup).  Centres every 2.5 lines over the first third: the line bracket changes after 3, 2, 3, 2, ... lines,
        # which against blocks of nine lines is at every position of every group; every 37 lines over the second third: blocks
        # that keep their corners throughout, blocks that change them once; one bracket over the rest
        shape = strip_shapes.shape("streaks")
        rpb = strip_shapes.SHAPES["streaks"].grid[2]
        line, sample = np.arange(float(shape[0])), np.arange(float(shape[1]))
        third = shape[0] // 3
        wl = np.concatenate([np.arange(0, third, 2.5), np.arange(third, 2 * third, 37.0), [shape[0] - 1.0]])
        ws = np.arange(9) * 251.0 + 17
        first = np.searchsorted(wl, line, side="right") - 1  # the bracket's first centre, as sref.bracket finds it
        changes = np.flatnonzero(np.diff(first)) + 1
        assert rpb > 8 and {int(p) for p in changes % rpb} == set(range(rpb))  # at every line of a block, its first included
        assert not np.diff(first[2 * third:-1]).any() and first[-1] == len(wl) - 1  # (the last line sits on the last centre)
    else:  # several 256-sample column strips and line blocks
        shape, wl, ws = (1031, 1237), np.arange(6) * 200.0, np.arange(7) * 200.0
        line, sample = np.arange(1031.0), np.arange(1237.0)
    dirs, anc = field(rng, len(wl), len(ws), holes=case != "one_window"), raster(rng, shape)
    return dirs, wl, ws, anc, line, sample


@pytest.mark.parametrize("case", ANCILLARY_CASES)
def test_ancillary_from_streaks_matches_the_restatement(case):
    """Every pixel through check_ancillary: K = 5 ulp of each component.  Measured worst on the MI355X: odd 3.17, one_row 2.38,
    one_window 1.31, irregular 2.88, dense 2.82, wide 3.44, dense_blocks 3.81 ulp."""
    dirs, wl, ws, anc, line, sample = ancillary_case(case)
    shape = anc.shape
    got = streaks.ancillary_from_streaks(dirs, anc, line, sample, windows_line=wl, windows_sample=ws)
    n, n_blend = check_ancillary(got, anc, (dirs, wl, ws, line, sample), case)
    assert got.dtype == np.complex128 and got.shape == shape
    if case in ("odd", "irregular", "wide"):
        assert 0 < n < (n + n_blend) // 2  # both the fallback and the blend occur, the blend on more than half of the non-NaN pixels


@pytest.mark.parametrize("name", sorted(sc.FIELDS))
def test_ancillary_on_the_designed_fields(name, torch):
    """small_components: directions within 1e-8 rad of the axes, so one component of v is 1e-8 of the other, with mixed signs: the
    pixels a bound relative to |a| said nothing about.  closed_form: windows of 1, -1 (as complex(-1.0, -0.0)), 1j and -1j, a on
    an axis with |a| = 7 * 2**k, dyadic weights: inside a bracket of four equal corners the output is |a| times that axis and the
    other part is +0.0, to the bit.  Both through numpy arrays and device tensors (bit-identical routes).  K = 5 ulp; measured
    worst on the MI355X: small_components 2.85, closed_form 1.32 ulp (its brackets of unequal corners)."""
    f = sc.FIELDS[name]()
    got = streaks.ancillary_from_streaks(f.dirs, f.anc, f.line, f.sample, windows_line=f.windows_line, windows_sample=f.windows_sample)
    check_ancillary(got, f.anc, (f.dirs, f.windows_line, f.windows_sample, f.line, f.sample), name)
    if name == "closed_form":
        eq = f.claim["equal"]
        assert bits_equal(got[eq], f.claim["expected"][eq]), "closed form, the sign of zero included"
    got_d = streaks.ancillary_from_streaks(torch.from_numpy(f.dirs.copy()).cuda(), torch.from_numpy(f.anc.copy()).cuda(), f.line, f.sample,
                                           windows_line=f.windows_line, windows_sample=f.windows_sample)
    assert bits_equal(host(got_d), got), name + ": device tensors"


def test_ancillary_full_size(torch):
    """20000 x 20000 on the device against a torch restatement of the same rules, every pixel (by blocks of lines)."""
    N = 20000
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(41)
    anc = torch.view_as_complex(6 * torch.randn((N, N, 2), generator=g, device=dev, dtype=torch.float64))
    anc[:3000, 15000:] = NAN
    anc[7000:7003, :] = 0
    rng = np.random.default_rng(42)
    wl = ws = np.arange(N)[::1600].astype(np.float64)  # the notebook configuration's 13 x 13 windows
    dirs = field(rng, 13, 13)
    out = streaks.ancillary_from_streaks(torch.from_numpy(dirs).to(dev), anc, windows_line=wl, windows_sample=ws)
    assert out.shape == (N, N) and out.dtype == torch.complex128
    i0, i1, tl = (torch.from_numpy(v).to(dev) for v in sref.bracket(wl, np.arange(N)))
    d = torch.from_numpy(dirs).to(dev)
    worst, n_fallback, n_nan = 0.0, 0, 0
    for a in range(0, N, 2000):
        rows = slice(a, a + 2000)
        vx = torch.zeros((2000, N), dtype=torch.float64, device=dev)
        vy = torch.zeros_like(vx)
        for ii, wgl in ((i0[rows], 1.0 - tl[rows]), (i1[rows], tl[rows])):
            for jj, wgs in ((i0, 1.0 - tl), (i1, tl)):
                w = wgl[:, None] * wgs[None, :]
                c = d[ii][:, jj]
                ok = ~(torch.isnan(c.real) | torch.isnan(c.imag))
                vx = torch.where(ok, vx + w * torch.where(ok, c.real, 0.0), vx)
                vy = torch.where(ok, vy + w * torch.where(ok, c.imag, 0.0), vy)
        ab, ob = anc[rows], out[rows]
        nv, m = torch.hypot(vx, vy), torch.hypot(ab.real, ab.imag)
        go = nv != 0
        wr, wi = torch.where(go, m * vx / nv, ab.real), torch.where(go, m * vy / nv, ab.imag)
        nan = torch.isnan(ab.real) | torch.isnan(ab.imag)
        assert bool((torch.isnan(ob.real) == nan).all()) and bool((torch.isnan(ob.imag) == nan).all())
        err = torch.maximum((ob.real - wr).abs(), (ob.imag - wi).abs())
        assert bool((err[~nan] <= 1e-12 * m[~nan]).all()), f"lines {a}.."
        fb = ~nan & ~go
        assert bool((torch.view_as_real(ob)[fb] == torch.view_as_real(ab)[fb]).all())
        worst = max(worst, float((err[~nan] / m[~nan].clamp_min(1e-300)).max()))
        n_fallback, n_nan = n_fallback + int(fb.sum()), n_nan + int(nan.sum())
    print(f"full size: max error / |a| = {worst:.3g} (bound 1e-12), {n_fallback} fallback pixels, {n_nan} NaN pixels")
    assert n_fallback > 0 and n_nan > 0


def test_sigma0_to_wind_on_a_user_stream(torch, gpu_ctx, delay_cycles):
    """Gradients(sigma0).histogram -> streaks_direction -> ancillary_from_streaks -> invert_from_model on a second stream, nothing
    synchronised before the winds are read back: bit-equal to the same chain run step by step with a device synchronisation
    after every step.  Then the new calls alone behind a held-back producer of the histograms: they return while it is in
    flight (no host synchronisation), and still read what it wrote."""
    from xsarsea_amd import windspeed
    inc, s_vv, _s_vh, _dsig, anc = synthetic_scene(603, 797, np.float64, 61)
    line, sample = LINE[:603], SAMPLE[:797]
    dev = torch.device("cuda", 0)
    kw = dict(windows_sizes=[1600, 3200], downscales_factors=[1, 2], window_step=0.5, line=line, sample=sample)

    def chain(s0, a, i, sync, hist=None):
        step = torch.cuda.synchronize if sync else (lambda: None)
        h = gradients.Gradients(s0, **kw).histogram if hist is None else hist
        step()
        s = streaks.streaks_direction(h)
        step()
        prior = streaks.ancillary_from_streaks(s, a, line, sample, min_used_ratio=0.2)
        step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wind = windspeed.invert_from_model(i, s0, ancillary_wind=prior, model="gmf_cmod5n", resolution="low", **ASYNC)
        step()
        return h, prior, wind

    t_s0, t_anc, t_inc = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (np.nan_to_num(s_vv, nan=0.01), anc, inc))
    torch.cuda.synchronize()
    h_ref, prior_ref, wind_ref = chain(t_s0, t_anc, t_inc, True)
    prior_ref, wind_ref = host(prior_ref), host(wind_ref)
    assert np.isfinite(wind_ref.real).any() and not bits_equal(prior_ref, anc)
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        b_s0, b_anc, b_inc = (torch.empty_like(t) for t in (t_s0, t_anc, t_inc))
        for b, t in ((b_s0, t_s0), (b_anc, t_anc), (b_inc, t_inc)):  # produced on P, consumed there without any synchronisation
            b.copy_(t, non_blocking=True)
        _h, prior, wind = chain(b_s0, b_anc, b_inc, False)
        got_prior, got_wind = _read_back(torch, P, prior, wind)
    assert bits_equal(got_prior, prior_ref), "a-priori raster"
    assert bits_equal(got_wind, wind_ref), "wind"
    # the new calls behind a held-back producer: the buffers hold another scene's histograms until the delayed copy lands
    decoy = gradients.Gradients(torch.from_numpy(scene((603, 797), np.float64, 62, land=False)).to(dev), **kw).histogram
    buf_w, buf_r = decoy.weight.clone(), decoy.used_ratio.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf_w, h_ref.weight), (buf_r, h_ref.used_ratio)])
        hb = gradients.GradientsHistogram(buf_w, buf_r, h_ref.angles, h_ref.line, h_ref.sample, h_ref.dims)
        _h, prior, wind = chain(t_s0, t_anc, t_inc, False, hist=hb)
        _in_flight(done)
        got_prior, got_wind = _read_back(torch, P, prior, wind)
    assert bits_equal(got_prior, prior_ref), "a-priori raster behind the held-back histograms"
    assert bits_equal(got_wind, wind_ref), "wind behind the held-back histograms"
