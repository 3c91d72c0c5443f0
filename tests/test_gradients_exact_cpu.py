"""tests/gradients_exact.py (the raster kernels of csrc/xsw_gradients.hip restated in their own order) on the CPU alone:
  - it states the same operations as the scipy restatements (tests/gradients_ref.py, tests/filtering_ref.py): 1e-12 relative on
    R2, G3, c, Mean and smoothing, G2 through its square and angle, 1e-9 absolute on the filters, equal NaN positions, on every
    case of tests/gradient_cases.py.  These are the existing tolerances of the scipy comparison, which stays the check of the
    semantics; nothing in the device comparison (tests/test_gpu_gradients_exact.py) carries one;
  - the conditions that the cases are there for hold (asserted where each case is built; `check_all` builds them all), the
    knife-edge count of the bracket on c among them;
  - the pin can see what 1e-12 cannot: seven numpy mutants each change a bit of the exact restatement, or leave the bracket,
    on a named case."""
import numpy as np
import pytest

import filter_cases as fc
import filtering_ref as fr
import gradient_cases as gc
import gradients_exact as gx
import gradients_ref as ref

RTOL, ATOL = 1e-12, 1e-9


def close(a, b, rtol=RTOL, atol=0.0):
    """|a - b| <= rtol |b| + atol with NaN positions equal."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(b)
    return bool((np.abs(a[m] - b[m]) <= rtol * np.abs(b[m]) + (atol[m] if np.ndim(atol) else atol)).all())


def local_close(G2, G3, C, g2, g3, c, c_mask=None):
    """The criteria of tests/test_gpu_gradients.py's assert_local_close."""
    scale = RTOL * np.nan_to_num(g3)
    ok = close((G2 ** 2).real, (g2 ** 2).real, RTOL, scale) and close((G2 ** 2).imag, (g2 ** 2).imag, RTOL, scale)
    ok = ok and np.array_equal(np.isnan(G2.real), np.isnan(g2.real))
    m = c > 1e-6
    if m.any():
        d = np.angle(G2[m]) - np.angle(g2[m])
        ok = ok and np.abs((d + np.pi / 2) % np.pi - np.pi / 2).max() < 1e-9
    if c_mask is not None:
        C, c = np.where(c_mask, C, 0.0), np.where(c_mask, c, 0.0)
    return bool(ok and close(G3, g3) and close(C, c, RTOL, RTOL))


def test_every_case_builds_and_its_conditions_hold():
    gc.check_all()
    fc.check_all()


def test_knife_edge_count_is_zero_on_every_case():
    """No pixel of any sigma0 case has c_lo <= 1 < c_hi or c_lo > 1; of the ramps only the interiors at k = 2**20, where c is
    exactly 1.0 by construction and the centre restatement is demanded bit for bit instead."""
    worst = 0.0
    for name in gc.SIGMA0_NAMES:
        for dtype in gc.DTYPES:
            b = gc.local_bracket(name, dtype)
            assert int(b.knife.sum()) == 0 and int(b.above.sum()) == 0, name
            if (~b.nan).any():
                worst = max(worst, float(b.c_hi[~b.nan].max()))
    assert worst < 1.0
    print(f"largest c_hi of the sigma0 cases {worst:.9f}")
    for name in gc.RAMP_NAMES:
        _am, b, interior = gc.ramp(name)
        assert not (b.knife & ~interior).any() and not b.above.any(), name
        assert b.knife[interior].all() == name.endswith("2p20") and b.knife[interior].any() == name.endswith("2p20")


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("name", gc.SIGMA0_NAMES)
def test_r2_and_local_state_what_the_scipy_restatement_states(name, dtype):
    s0 = gc.sigma0(name, dtype)
    with np.errstate(invalid="ignore"):
        want = ref.R2(s0)
        assert close(gc.r2_want(name, dtype, False, False), want)
        assert close(gc.r2_want(name, dtype, False, True), np.sqrt(want))
        a = gc.ampl(name, dtype)
        assert close(gc.r2_want(name, dtype, True, False), ref.R2(a))
        b = gc.local_bracket(name, dtype)
        g2, g3, c = ref.local_gradients(a)
    assert local_close(b.G2, b.za, b.c, g2, g3, c)
    assert gx.same_bits(np.stack(gx.local_exact(a)[1:]), np.stack([b.za, b.c])) and gx.same_bits(gx.local_exact(a)[0], b.G2)
    assert b.problems(b.G2, b.za, b.c) == []  # the centre lies inside its own bracket
    assert b.problems(None, b.za_lo, np.where(b.nan, 0.0, b.c_lo)) == [] and b.problems(None, b.za_hi, np.where(b.nan, 0.0, b.c_hi)) == []


@pytest.mark.parametrize("name", gc.RAMP_NAMES)
def test_ramps_state_what_the_scipy_restatement_states(name):
    am, b, interior = gc.ramp(name)
    g2, g3, c = ref.local_gradients(np.array(am))
    assert local_close(b.G2, b.za, b.c, g2, g3, c, c_mask=~b.knife)  # c on a knife-edge pixel is 1 or 0 by the last bit
    assert b.problems(b.G2, b.za, b.c, exact=interior) == []


def mean_cases():
    return [(g, False) for g in fc.SMOOTH_GRIDS] + [(g, True) for g in fc.BIG_GRIDS]


@pytest.mark.parametrize("grid,nan_edges", mean_cases(), ids=lambda v: "nan_edges" if v is True else "" if v is False else f"{v[0]}x{v[1]}")
def test_mean_and_smoothing_state_what_the_scipy_restatement_states(grid, nan_edges):
    x = fc.mean_input(grid, nan_edges)
    assert close(gx.smooth_exact(x), fc.smoothing_want(grid, nan_edges))
    if grid in fc.MEAN_GRIDS:
        assert close(gx.mean_exact(x), fc.mean_want(grid, nan_edges))


@pytest.mark.parametrize("shape", fc.COARSEN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_coarsened_smoothing_states_what_the_scipy_restatement_states(shape):
    x, want = fc.coarsen_input(shape)
    assert close(gx.smooth_exact(x, True), want)


def filters_close(got, want):
    """The criteria of tests/test_gpu_filtering.py's compare: 1e-9 absolute, NaN positions equal but for f1 and F where
    d <= 1e-9 J1."""
    d, J1 = want[5], want[6]
    with np.errstate(invalid="ignore"):
        ill = np.isfinite(J1) & (d <= 1e-9 * J1)
    for k in range(5):
        free = ill if k in (0, 4) else np.zeros_like(ill)
        a, b = got[k], want[k]
        if not np.array_equal(np.isnan(a) | free, np.isnan(b) | free):
            return False
        m = ~np.isnan(a) & ~np.isnan(b)
        if m.any() and np.abs(a[m] - b[m]).max() > ATOL:
            return False
    return True


@pytest.mark.parametrize("case", gc.FILTER_CASES, ids=gc.filter_id)
def test_filter_states_what_the_scipy_restatement_states(case):
    t = fc.designed(*case)
    got = gc.filter_exact_of(t)
    assert filters_close(got, fc.designed_want(*case))
    assert not (gx.filter_terms(t["r2"], t["g3"])[3] <= 0).any() or case[3] is not None  # in-ramp: d is no noise here
    np.testing.assert_array_equal(gx.zoom_exact(t["q4"], case[0]), fr.zoom_linear(t["q4"], case[0]))


@pytest.mark.parametrize("grid", gc.NOISE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_sign_noise_cases(grid):
    """d = J1 - J**2 is rounding noise: every pixel is exempt in the scipy comparison (d <= 1e-9 J1), f2..f4 are compared; the
    exact restatement has NaN exactly where its own d < 0, on at least 16 pixels, and finite f1 on at least 16."""
    t, want = gc.noise_inputs(grid), gc.noise_want(grid)
    scipy_side = fc.combine_with(t)
    assert (scipy_side[5] <= 1e-9 * scipy_side[6]).all()
    assert filters_close(want, scipy_side)
    assert not np.array_equal(np.isnan(want[0]), np.isnan(scipy_side[0]))  # scipy's order has another sign on some pixel


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("name", gc.CHAIN_NAMES)
def test_chain_states_what_the_scipy_restatement_states(name, dtype):
    if name.startswith("chain"):
        shape = tuple(int(v) for v in name.split("-")[1].split("x"))
        want = fc.chain_want(shape, dtype, name.endswith("-nan"))
    else:
        want = fr.filtering_parameters(gc.sigma0(name, dtype))
    b = gc.local_bracket(name, dtype)
    r2 = gc.r2_want(name, dtype, True, False)
    got = gx.filter_exact(r2, b.za, b.c, gx.smooth_exact(r2, True))
    assert filters_close(got, want)


# ------------------------------------------------------------------------------------------------------- the mutants
def test_mutant_scipy_summation_order():
    """scipy's order agrees to 1e-12 and differs in the bits."""
    s0 = gc.sigma0("tiles-70x134", np.float64)
    exact, scipy_side = gc.r2_want("tiles-70x134", np.float64, False, False), ref.R2(s0)
    assert close(scipy_side, exact) and not gx.same_bits(scipy_side, exact)
    x = fc.mean_input((63, 65))
    assert close(fr.Mean(x), gx.mean_exact(x)) and not gx.same_bits(fr.Mean(x), gx.mean_exact(x))


def test_mutant_halo_one_row_off_at_a_16_seam():
    """conv3 of k_grad_r2 whose lower halo row, for the last row of each 16-row tile, comes from one coarse row further."""
    a = gc.sigma0("tiles-70x134", np.float64)
    coarse = gx.nanmean4(gx.quad(gx.conv5(a)))
    P = gx.pad_symm(coarse, 1)
    exact = gx.conv_in_order(P, gx.W3, 1.0 / 16.0)
    assert gx.same_bits(exact, gc.r2_want("tiles-70x134", np.float64, False, False))
    mutant = exact.copy()
    rows = [Y for Y in range(exact.shape[0] - 1) if Y % 16 == 15]
    assert rows == [15, 31]
    for Y in rows:
        slab = P[Y:Y + 3].copy()
        slab[2] = P[Y + 3]
        mutant[Y] = gx.conv_in_order(slab, gx.W3, 1.0 / 16.0)[0]
    assert not gx.same_bits(mutant, exact) and gx.same_bits(np.delete(mutant, rows, 0), np.delete(exact, rows, 0))


def test_mutant_halo_one_row_off_at_a_32_seam():
    """The last line tap of Mean's B42 pass, for the last row of each 32-row tile, taken one row further."""
    x = fc.mean_input((63, 65))
    P = gx.sep_in_order(gx.pad_symm(gx.mean_stage1(x), 4), gx.W9_16, 1)
    exact = gx.sep_in_order(P, gx.W9_16, 0)
    assert gx.same_bits(exact, gx.mean_exact(x))
    mutant = exact.copy()
    slab = P[31:40].copy()
    slab[8] = P[40]
    mutant[31] = gx.sep_in_order(slab, gx.W9_16, 0)[0]
    assert not gx.same_bits(mutant, exact)
    # the same on the raw filter's J: f1 inside its ramp shows it
    t = fc.designed((63, 65), "A", 1)
    assert fc.inside(gc.filter_exact_of(t)[0])[31].all()


def test_mutant_coarse_stage_reflected_at_the_fine_edge():
    """The coarse halo computed from the fine raster's reflection: on an odd axis the halo group holds the trimmed pixel."""
    a = gc.sigma0("thin-34x35", np.float64).astype(np.float64)
    coarse_with_halo = gx.nanmean4(gx.quad(gx.pad_symm(gx.conv5(a), 2)))
    assert coarse_with_halo.shape == (17 + 2, 17 + 2)
    mutant = gx.conv_in_order(coarse_with_halo, gx.W3, 1.0 / 16.0)
    exact = gc.r2_want("thin-34x35", np.float64, False, False)
    assert mutant.shape == exact.shape and not gx.same_bits(mutant, exact)
    assert gx.same_bits(mutant[1:-1, 1:-1], exact[1:-1, 1:-1])  # only the rim can tell


def test_mutant_c_below_one_only():
    """c < 1 in place of c <= 1 zeroes the ramp interior, where c is exactly 1.0."""
    for name in gc.RAMP_NAMES:
        _am, b, interior = gc.ramp(name)
        mutant = gx.quality_exact(b.d, b.za, keep=np.less)
        if name.endswith("2p20"):
            assert (mutant[interior] == 0).all() and (b.c[interior] == 1).all()
            assert b.problems(b.G2, b.za, mutant, exact=interior) != []
        else:
            assert gx.same_bits(mutant, b.c)
    for dtype in gc.DTYPES:  # no other case has a pixel at the cut
        b = gc.local_bracket("scene-203x317", dtype)
        assert gx.same_bits(gx.quality_exact(b.d, b.za, keep=np.less), b.c)


@pytest.mark.parametrize("name", ["tiles-70x134", "designed-90x101"])
def test_mutant_g2_sign(name):
    """-G2 has the same square and the same angle modulo pi; conj(G2) the same modulus.  Both leave the bracket."""
    b = gc.local_bracket(name, np.float64)
    assert local_close(-b.G2, b.za, b.c, b.G2, b.za, b.c)  # what the existing comparison sees: nothing
    assert any(p.startswith("G2.real: sign") for p in b.problems(-b.G2, b.za, b.c))
    assert any(p.startswith("G2.imag") for p in b.problems(np.conj(b.G2), b.za, b.c))
    for _name in gc.RAMP_NAMES:
        _am, rb, interior = gc.ramp(_name)
        assert rb.problems(np.conj(rb.G2), rb.za, rb.c, exact=interior) != []


def test_mutant_csqrt_branch():
    """The x < 0 formula used for x >= 0 (and the reverse): equal in exact arithmetic, not in the bits, on a scene."""
    b = gc.local_bracket("tiles-70x134", np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(0.5 * (b.d - b.zr))
        r = np.sqrt(0.5 * (b.d + b.zr))
        re = np.where(b.branch == 2, np.fabs(0.5 * (b.zi / s)), np.where(b.branch == 3, r, b.re))
        im = np.where(b.branch == 2, np.copysign(s, b.zi), np.where(b.branch == 3, 0.5 * (b.zi / r), b.im))
    assert {2, 3} <= set(np.unique(b.branch))
    assert b.problems(re + 1j * im, b.za, b.c) != []


def test_mutant_zero_taps_of_w9_dropped():
    """The NaN footprint of one Inf (gradient_cases.inf_input): 0 * inf is NaN on the 13 x 13 outputs around it but the four
    corners, which only the outermost tap reaches (+inf); without the zero taps all 169 are +inf.  One NaN covers the 13 x 13
    either way (the 5 x 5 of B4 shifted by even offsets), and on a finite raster nothing shows: only this case pins the
    zero taps."""
    x = gc.inf_input()
    exact, mutant = gx.mean_exact(x), gx.mean_exact(x, skip_zero_taps=True)
    assert np.isnan(exact).sum() == 165 and np.isinf(exact).sum() == 4 and np.array_equal(np.isnan(exact), np.isnan(fr.Mean(x)))
    assert np.isnan(mutant).sum() == 0 and np.isinf(mutant).sum() == 169 and not gx.same_bits(mutant, exact)
    x = np.where(np.isinf(x), np.nan, x)
    assert np.isnan(gx.mean_exact(x)).sum() == np.isnan(gx.mean_exact(x, skip_zero_taps=True)).sum() == 169
    clean = fc.mean_input((63, 65))
    assert gx.same_bits(gx.mean_exact(clean, skip_zero_taps=True), gx.mean_exact(clean))


@pytest.mark.parametrize("grid", gc.NOISE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_mutant_d_clamped_at_zero(grid):
    t = gc.noise_inputs(grid)
    mutant = gx.filter_exact(t["r2"], t["g3"], t["c"], t["q4"], clamp_d=True)
    want = gc.noise_want(grid)
    assert not np.isnan(mutant[0]).any() and np.isnan(want[0]).any() and not gx.same_bits(mutant, want)
    assert filters_close(mutant, fc.combine_with(t))  # and the scipy comparison exempts exactly these pixels
