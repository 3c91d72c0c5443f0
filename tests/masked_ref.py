"""CPU restatement of the masked direction histograms of xsarsea_amd.gradients (`keep_mask`, `gradient_histogram(keep=)`,
`Gradients(..., mask=, min_F=)`; DESIGN.md section 9, rule 8), built from tests/gradients_ref.py and tests/filtering_ref.py.

The rule, in one sentence: a masked-out pixel of the local-gradients grid behaves in gradient_histogram exactly as if its G2 were
NaN.  So the restatement writes NaN into G2 where the keep mask is 0 and calls the unmasked restatement; nothing else is new.
The reference computes filtering_parameters' F and applies it nowhere: this step has no counterpart there.
Test infrastructure only: the product never imports it.
"""
import numpy as np

import filtering_ref as fr
import gradients_ref as ref


def keep_blocks(a, b, threshold=None, and_with=None):
    """uint8 (L // b, S // b): 1 iff every input of the b x b block is usable, the remainder trimmed.  With a threshold usable is
    x >= threshold (NaN is not); without, non-zero.  and_with: a mask on the output grid, AND-ed in."""
    a = np.asarray(a)
    L, S = a.shape[0] // b, a.shape[1] // b
    blocks = a[:L * b, :S * b].reshape(L, b, S, b)
    if threshold is None:
        ok = blocks != 0
    else:
        with np.errstate(invalid="ignore"):
            ok = blocks >= threshold
    out = ok.all(axis=(1, 3))
    if and_with is not None:
        out = out & (np.asarray(and_with) != 0)
    return out.astype(np.uint8)


def field_F(sigma0, factor=1):
    """filtering_parameters' F of one field's own raster: the f x f box mean of sigma0 (in sigma0's dtype) for f > 1."""
    return fr.filtering_parameters(ref.area(sigma0, factor))[4]


def field_keep(sigma0, factor=1, min_F=None, mask=None, F=None):
    """Keep mask of one (pol, factor) field on its local-gradients grid (None without mask and min_F): the sigma0-grid mask
    reduced by 4 f x 4 f, AND F >= min_F reduced by 2 x 2.  F: a precomputed field_F(sigma0, factor)."""
    k = None
    if mask is not None:
        k = keep_blocks(mask, 4 * factor)
    if min_F is not None:
        k = keep_blocks(field_F(sigma0, factor) if F is None else F, 2, min_F, and_with=k)
    return k


def nan_where_masked(g2, keep):
    g2 = np.array(g2, dtype=np.complex128)
    if keep is not None:
        g2[np.asarray(keep) == 0] = complex(np.nan, np.nan)
    return g2


def histogram_masked(sigma0, line, sample, windows_sizes=(1600,), downscales_factors=(1,), window_step=1, windows_at=None, n_angles=72,
                     min_F=None, mask=None):
    """gradients_ref.histogram with NaN written into each field's G2 where its keep mask is 0: (weight [df, ws, line, sample,
    angles], used_ratio, ambiguous, windows_at, keeps [one per factor], unmasked used_ratio)."""
    bins = ref.angles_bins(n_angles)
    fields = [ref.lg_of(sigma0, line, sample, f) for f in downscales_factors]
    keeps = [field_keep(sigma0, f, min_F, mask) for f in downscales_factors]
    if windows_at is None:
        _, _, _, _, l0, s0 = fields[0]
        step = int(ref.window_pixels(windows_sizes[0], l0, s0) * window_step)
        windows_at = {"line": l0[::step], "sample": s0[::step]}
    wl, ws_ = np.asarray(windows_at["line"]), np.asarray(windows_at["sample"])
    W = np.zeros((len(downscales_factors), len(windows_sizes), len(wl), len(ws_), n_angles))
    R, A, R0 = np.zeros(W.shape[:-1]), np.zeros(W.shape[:-1]), np.zeros(W.shape[:-1])
    for a, ((g2, c, lgl, lgs, _, _), keep) in enumerate(zip(fields, keeps)):
        assert keep is None or keep.shape == g2.shape
        gm = nan_where_masked(g2, keep)
        rows, cols = ref.nearest(lgl, wl), ref.nearest(lgs, ws_)
        for b, wsz in enumerate(windows_sizes):
            w = ref.window_pixels(wsz, lgl, lgs)
            for i, r in enumerate(rows):
                for j, q in enumerate(cols):
                    cw = ref.rolling_window(c, r, q, w)
                    h, u, amb = ref.gradient_histogram(ref.rolling_window(gm, r, q, w), cw, bins)
                    _, u0, _ = ref.gradient_histogram(ref.rolling_window(g2, r, q, w), cw, bins)
                    W[a, b, i, j] = h / (w * w)
                    R[a, b, i, j] = 0.0 if np.isnan(u) else u
                    R0[a, b, i, j] = 0.0 if np.isnan(u0) else u0
                    A[a, b, i, j] = amb / (w * w)
    return W, R, A, windows_at, keeps, R0


# ---- what the GPU tests compare on (tests/test_masked_gradients_cpu.py asserts `scene_conditions` on each of them)
THRESHOLDS = (0.3, 0.7)       # between F's plateaus 0.5, sqrt(1/2), sqrt(3/4), 1; 0.5 lies ON one and must not be compared on
WINDOWS_SIZES = (200, 800)    # 5 and 20 pixels of the local-gradients grid at factor 1 (coordinates 10 apart), 2 and 10 at factor 2
FACTORS = (1, 2)


def coords(shape):
    return np.arange(shape[0]) * 10.0 + 5, np.arange(shape[1]) * 10.0 + 5


def window_groups(R, R0):
    """(fully or nearly masked, untouched) counts among the live windows (unmasked used_ratio R0 >= 0.5): masked used_ratio
    R <= 0.1 R0, and R == R0."""
    live = R0 >= 0.5
    return int(((R <= 0.1 * R0) & live).sum()), int(((R == R0) & live).sum())


def scene_conditions(sigma0, threshold, factors=FACTORS):
    """Per factor: (restatement F pixels within 1e-8 of the threshold, kept share of the local-gradients grid).  Required: 0 and
    within [0.15, 0.95]."""
    out = []
    for f in factors:
        F = field_F(sigma0, f)
        with np.errstate(invalid="ignore"):
            near = int((np.abs(F - threshold) < 1e-8).sum())
        out.append((near, float(keep_blocks(F, 2, threshold).mean())))
    return out


def blob_centres(shape, seed, gamma=20):
    """(line, sample, amplitude, radius) of filtering_ref.rain_scene's six blobs, in pixels: the scene's random draws replayed."""
    rng = np.random.default_rng(seed)
    L, S = shape
    rng.gamma(gamma, 1 / gamma, shape)
    out = []
    for amp, rad in zip(np.linspace(1.5, 4.0, 6), rng.permutation(np.linspace(4.0, 20.0, 6))):
        out.append((rng.uniform(0.1, 0.9) * L, rng.uniform(0.1, 0.9) * S, float(amp), float(rad)))
    return out


# the chain test's scene: windows of 400 (10 pixels of the local-gradients grid) centred on the two strongest blobs and on
# quiet water; one configuration, so a window's used_ratio is that of its one histogram
CHAIN_SCENE = ((402, 515), np.float64, 22, 100)
CHAIN_MIN_F = 0.7


def chain_windows():
    """(windows_at, [(i, j) of the windows centred on the two strongest blobs]) for CHAIN_SCENE."""
    shape, _dtype, seed, gamma = CHAIN_SCENE
    (l5, s5, *_), (l6, s6, *_) = blob_centres(shape, seed, gamma)[4:]
    at = {"line": np.array([605.0, np.round(l6) * 10 + 5, np.round(l5) * 10 + 5]), "sample": np.array([1005.0, np.round(s5) * 10 + 5, np.round(s6) * 10 + 5])}
    assert (np.diff(at["line"]) > 0).all() and (np.diff(at["sample"]) > 0).all()
    return at, [(1, 2), (2, 1)]


def separating_ratio(R, R0):
    """(r, gap, below, above): the middle of the largest gap in the masked used ratios of the live windows (unmasked R0 >= 0.5),
    the gap's width, and the windows on either side."""
    live = R0 >= 0.5
    v = np.sort(R[live])
    k = int(np.argmax(np.diff(v)))
    r = float((v[k] + v[k + 1]) / 2)
    return r, float(v[k + 1] - v[k]), live & (R < r), live & (R > r)
