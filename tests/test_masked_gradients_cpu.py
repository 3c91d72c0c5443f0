"""CPU: the restatement of the masked direction histograms (tests/masked_ref.py) and the conditions that keep the GPU comparison
honest on every (scene, threshold) it uses, asserted on the restatement alone; then the argument checks of xsarsea_amd.gradients
that must raise before any device call (they run here without a GPU)."""
import numpy as np
import pytest

import filtering_ref as fr
import gradients_ref as ref
import keep_cases
import masked_ref as mr
import strip_shapes
from xsarsea_amd import gradients

BINS = ref.angles_bins(72)


def test_keep_blocks_properties():
    rng = np.random.default_rng(1)
    a = rng.uniform(0, 1, (11, 14))
    a[3, 4], a[8, 9], a[0, 13] = np.nan, np.inf, -np.inf
    k = mr.keep_blocks(a, 1, 0.5)
    assert k.dtype == np.uint8 and k.shape == a.shape
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(k, (a >= 0.5).astype(np.uint8))          # b = 1: the comparison itself
    assert k[3, 4] == 0 and k[8, 9] == 1 and k[0, 13] == 0                      # NaN -> 0, +Inf usable, -Inf not
    for b in (2, 3, 4, 8):
        k = mr.keep_blocks(a, b, 0.2)
        assert k.shape == (11 // b, 14 // b)                                     # the remainder is trimmed
        for i in range(k.shape[0]):
            for j in range(k.shape[1]):
                blk = a[b * i:b * i + b, b * j:b * j + b]
                with np.errstate(invalid="ignore"):
                    assert k[i, j] == int((blk >= 0.2).all())
    assert mr.keep_blocks(a, 2, 0.0)[1, 2] == 0 and mr.keep_blocks(a, 2, -np.inf)[1, 2] == 0   # the block of the NaN
    assert mr.keep_blocks(a, 2, -np.inf)[0, 6] == 1                              # -Inf >= -Inf
    u = (rng.uniform(0, 1, (9, 10)) > 0.2).astype(np.uint8) * 7                  # non-zero, not only 1
    np.testing.assert_array_equal(mr.keep_blocks(u, 1), (u != 0).astype(np.uint8))
    np.testing.assert_array_equal(mr.keep_blocks(u.astype(bool), 2), mr.keep_blocks(u, 2))
    other = (rng.uniform(0, 1, (4, 5)) > 0.5).astype(np.uint8)
    np.testing.assert_array_equal(mr.keep_blocks(u, 2, and_with=other), mr.keep_blocks(u, 2) & other)   # the AND input
    assert mr.keep_blocks(u, 2, and_with=np.zeros((4, 5), np.uint8)).sum() == 0


def test_masked_histogram_is_the_unmasked_one_on_nan():
    """The rule itself on one box: masking == NaN in G2 (not kept, outside the median, in no bin, not in the numerator)."""
    rng = np.random.default_rng(2)
    g2 = np.sqrt(rng.normal(size=(23, 31)) + 1j * rng.normal(size=(23, 31)))
    c = rng.uniform(0, 1, g2.shape)
    keep = (rng.uniform(0, 1, g2.shape) > 0.4).astype(np.uint8)
    h, u, _ = ref.gradient_histogram(mr.nan_where_masked(g2, keep), c, BINS)
    sel = keep != 0
    a = np.abs(g2[sel])
    want = np.zeros(72)
    np.add.at(want, np.round((np.angle(g2[sel]) - BINS[0]) / (BINS[1] - BINS[0])).astype(int) % 72, a / (a + np.median(a)) * c[sel])
    np.testing.assert_allclose(h, want, rtol=1e-12)
    assert u == sel.sum() / g2.size
    h1, u1, _ = ref.gradient_histogram(mr.nan_where_masked(g2, np.ones_like(keep)), c, BINS)
    h0, u0, _ = ref.gradient_histogram(g2, c, BINS)
    np.testing.assert_array_equal(h1, h0)
    assert u1 == u0 == 1.0


@pytest.mark.parametrize("threshold", mr.THRESHOLDS)
@pytest.mark.parametrize("spec", fr.GPU_SCENES + [fr.FULL_TILE], ids=lambda s: f"{s[0][0]}x{s[0][1]}-{np.dtype(s[1]).name}")
def test_scene_conditions(spec, threshold):
    """No restatement F within 1e-8 of the threshold (the device F is pinned to 1e-9, so the masks must then be equal); the kept
    share of every field's local-gradients grid within [0.15, 0.95]."""
    shape, dtype, seed, gamma = spec
    s0 = fr.full_tile() if spec == fr.FULL_TILE else fr.rain_scene(shape, dtype, seed, gamma)
    for f, (near, share) in zip(mr.FACTORS, mr.scene_conditions(s0, threshold)):
        print(f"{shape} {np.dtype(dtype).name} threshold {threshold} factor {f}: {near} pixels within 1e-8, kept share {share:.3f}")
        assert near == 0
        assert 0.15 <= share <= 0.95


def test_the_half_plateau_is_not_a_threshold():
    """Why 0.5 is not compared on: F sits exactly on it (three filters at 0, one at 1) on many pixels of every scene."""
    shape, dtype, seed, gamma = fr.GPU_SCENES[0]
    near, _ = mr.scene_conditions(fr.rain_scene(shape, dtype, seed, gamma), 0.5, (1,))[0]
    assert near > 100


@pytest.mark.parametrize("threshold", mr.THRESHOLDS)
@pytest.mark.parametrize("spec", fr.GPU_SCENES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{np.dtype(s[1]).name}")
def test_compared_windows_cover_both_groups(spec, threshold):
    """Among the windows the GPU test compares (both factors, both sizes) at least one live window is fully or nearly masked
    and at least one is untouched; no window has a pixel within 1e-9 rad of a bin edge."""
    shape, dtype, seed, gamma = spec
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    line, sample = mr.coords(shape)
    W, R, A, at, keeps, R0 = mr.histogram_masked(s0, line, sample, mr.WINDOWS_SIZES, mr.FACTORS, 1, min_F=threshold)
    masked, untouched = mr.window_groups(R, R0)
    print(f"{shape} {np.dtype(dtype).name} threshold {threshold}: {R.size} windows, {masked} nearly masked, {untouched} untouched")
    assert masked >= 1 and untouched >= 1
    assert (R <= R0).all() and (A == 0).all()


def test_argument_checks_raise_before_any_device_call():
    s0 = np.full((40, 52), 0.1, np.float32)
    with pytest.raises(ValueError, match="shape"):
        gradients.Gradients(s0, mask=np.ones((40, 51), bool))
    with pytest.raises(ValueError, match="shape"):
        gradients.Gradients(np.stack([s0, s0]), mask=np.ones((2, 40, 52), bool))   # the mask is not per pol
    with pytest.raises(ValueError, match="shape"):
        gradients.Gradients2D(s0, mask=np.ones((10, 13), np.uint8))
    with pytest.raises(TypeError, match="bool or uint8"):
        gradients.Gradients(s0, mask=np.ones((40, 52), np.float64))
    with pytest.raises(ValueError, match="NaN"):
        gradients.Gradients(s0, min_F=float("nan"))
    with pytest.raises(ValueError, match="no threshold"):
        gradients.keep_mask(np.ones((8, 8), bool), threshold=0.5)
    with pytest.raises(ValueError, match="no threshold"):
        gradients.keep_mask(np.ones((8, 8), np.uint8), threshold=0.5)
    with pytest.raises(ValueError, match="needs a threshold"):
        gradients.keep_mask(np.ones((8, 8)))
    with pytest.raises(ValueError, match="NaN"):
        gradients.keep_mask(np.ones((8, 8)), threshold=float("nan"))
    with pytest.raises(ValueError, match="block"):
        gradients.keep_mask(np.ones((8, 8), bool), block=0)
    with pytest.raises(ValueError, match="no 16 x 16 block"):
        gradients.keep_mask(np.ones((8, 32), bool), block=16)
    with pytest.raises(ValueError, match="output grid"):
        gradients.keep_mask(np.ones((8, 8), bool), block=2, and_with=np.ones((8, 8), bool))
    with pytest.raises(TypeError):
        gradients.keep_mask(np.ones((8, 8), np.int32))
    with pytest.raises(ValueError, match="2-D"):
        gradients.keep_mask(np.ones((2, 8, 8), bool))
    g2, c = np.ones((6, 7), np.complex128), np.ones((6, 7))
    with pytest.raises(ValueError, match="g2's shape"):
        gradients.gradient_histogram(g2, c, BINS, keep=np.ones((7, 6), bool))
    with pytest.raises(TypeError, match="bool or uint8"):
        gradients.gradient_histogram(g2, c, BINS, keep=np.ones((6, 7)))
    # accepted arguments construct without a device
    g = gradients.Gradients(s0, windows_sizes=[8], mask=np.ones((40, 52), bool), min_F=0.6)
    assert g.gradients_list[0]._field._min_F == 0.6


def test_chain_scene_separates_the_blob_windows():
    """The chain test's premise, on the restatement alone: with min_F the windows on the two strongest blobs fall below a
    used_ratio r that the quiet windows stay above, with a gap of at least 0.2; without min_F both groups are full."""
    shape, dtype, seed, gamma = mr.CHAIN_SCENE
    s0 = fr.rain_scene(shape, dtype, seed, gamma)
    line, sample = mr.coords(shape)
    at, blobs = mr.chain_windows()
    _, R, A, _, _, R0 = mr.histogram_masked(s0, line, sample, (400,), (1,), windows_at=at, min_F=mr.CHAIN_MIN_F)
    R, R0 = R[0, 0], R0[0, 0]
    r, gap, below, above = mr.separating_ratio(R, R0)
    print(f"r = {r:.3f}, gap {gap:.3f}, masked used_ratio\n{R}\nunmasked\n{R0}")
    assert gap >= 0.2 and above.sum() >= 3 and (A == 0).all()
    for i, j in blobs:
        assert below[i, j] and R0[i, j] == 1.0
    assert (R0[above] > r + gap / 2).all()


@pytest.mark.parametrize("key", keep_cases.KEYS)
def test_keep_cases_tell_a_one_row_kernel_from_a_right_one(key):
    """The premise of tests/test_gpu_strips.py's keep-mask tests, on the restatement alone, with and without and_with.  The
    probe blocks are what tests/keep_cases.py says: one element makes a block unusable, at every row and every column of the
    block in turn, and the blocks left usable are kept.  The expected mask, restricted to the output rows that are NOT the
    first of their workgroup, holds both values and differs from the mask that repeats each workgroup's first row -- also on
    every probe row by itself -- so a kernel that stopped after one row, or read row y0 again, cannot pass."""
    c = keep_cases.case(key)
    e = strip_shapes.SHAPES[key]
    b, (gx, gy, rpb, last) = c.block, e.grid
    Lo, So = e.lines // b, e.samples // b
    assert c.src.shape == (e.lines, e.samples) and str(c.src.dtype) == e.dtype and c.and_with.shape == (Lo, So)
    assert c.src.nbytes < 70e6
    assert (Lo * b < e.lines or So * b < e.samples) and Lo == (gy - 1) * rpb + last
    later = np.arange(Lo) % rpb != 0
    probes = strip_shapes.probe_lines(key)
    assert probes == list(range(rpb, 2 * rpb)) + list(range(Lo - last, Lo)) and len(c.holes) == len(probes)
    plain, anded = mr.keep_blocks(c.src, b, c.threshold), mr.keep_blocks(c.src, b, c.threshold, and_with=c.and_with)
    for Y, X in c.bad:
        assert plain[Y, X] == 0
        blk = np.array(c.src[Y * b:(Y + 1) * b, X * b:(X + 1) * b])
        with np.errstate(invalid="ignore"):
            unusable = ~(blk >= c.threshold) if c.threshold is not None else blk == 0
        assert unusable.sum() == 1                                       # a single element decides the block
    assert all(plain[Y, X] == 1 for Y, X in c.good)
    assert sorted(c.bad + c.good) == [(Y, X) for Y in sorted(probes) for X in range(So)]
    n = len(c.at)
    assert n >= b and {i for i, _ in c.at} == set(range(b)) and {j for _, j in c.at} == set(range(b))
    assert len(set(c.at)) == min(n, b * b)                               # every (i, j) of the block while n < b * b
    if c.threshold is not None:
        kinds = [c.src[Y * b + i, X * b + j] for (Y, X), (i, j) in zip(c.bad, c.at)]
        assert any(np.isnan(v) for v in kinds) and -np.inf in kinds and keep_cases.BELOW in kinds
        assert (c.src == c.threshold).any() and (c.src == np.inf).any()
    else:
        assert {int(v) for Y, X in c.good for v in np.unique(c.src[Y * b:(Y + 1) * b, X * b:(X + 1) * b])} == {0x01, 0x80, 0xFF}
    for Y, X in c.holes:                                                  # and_with's lone zero takes a usable block out
        assert plain[Y, X] == 1 and anded[Y, X] == 0 and (c.and_with[Y] == 0).sum() == 1
    assert {Y % rpb for Y, _ in c.holes} >= set(range(min(rpb, 5)))       # u = 0..3 of an unrolled group and a tail row
    for want in (plain, anded):
        assert want[later].min() == 0 and want[later].max() == 1
        stuck = keep_cases.repeat_first_rows(want, key)
        assert (want != stuck)[later].any()
        assert all((want[Y] != stuck[Y]).any() for Y in probes if Y % rpb)
        print(key, (gx, gy, rpb, last), f"kept share {want.mean():.3f}, rows that differ from their workgroup's first row "
              f"{int((want != stuck).any(axis=1).sum())} of {int(later.sum())}")
