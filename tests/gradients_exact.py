"""The five raster kernels of csrc/xsw_gradients.hip (k_grad_r2, k_grad_local, k_grad_smooth, k_grad_mean, k_grad_filter)
restated in numpy IN THEIR OWN ORDER of operations: every sum starts at +0.0 and adds its terms in the order the kernel's loops
do, every product and quotient is the kernel's, and no scipy call takes part.  The kernels are built with -ffp-contract=off and
each output is computed by the same statements wherever its tile lies, so a correct kernel reproduces these values bit for bit
(tests/test_gpu_gradients_exact.py); tests/gradients_ref.py and tests/filtering_ref.py stay the independent check of the
semantics (tests/test_gradients_exact_cpu.py holds the two together at 1e-12 / 1e-9).

The one library call of the five kernels is `hypot` (k_grad_local: |grad**2| per fine pixel, and d = |R2(grad**2)| per output).
Its value is not pinned but bracketed: `local_planes`, `csqrt_exact` and `quality_exact` take the modulus as an argument, and
`hyp_centre` / `hyp_lo` / `hyp_hi` give sqrt(re**2 + im**2) evaluated in np.longdouble and rounded to double (within
0.5 + 2**-10 ulp of the true value), and that value two float64 spacings down (clamped at 0) and up.  The project's bound on the
device's hypot is 1.5 ulp, so the device's value lies between the two; everything after hypot is monotone
in it (`local_bracket`).
Test infrastructure only: the product never imports it.
"""
import numpy as np

import filtering_ref as fr

W3 = (1.0, 2.0, 1.0)
W5 = (1.0, 4.0, 6.0, 4.0, 1.0)
W5_16 = tuple(k / 16 for k in W5)
W9_16 = (1.0 / 16, 0.0, 4.0 / 16, 0.0, 6.0 / 16, 0.0, 4.0 / 16, 0.0, 1.0 / 16)
HYPOT_STEPS = 2  # float64 spacings either side of the longdouble value: 1.5 ulp (the project's h) + 0.5 + 2**-10, rounded up
NAN = float("nan")


def quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            return fn(*a, **k)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def same_bits(got, want):
    """One shape; NaN where and only where `want` has NaN (payloads aside), every other float64 equal as uint64 (so -0.0 is not
    +0.0); complex arrays part by part."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    parts = ((got.real, want.real), (got.imag, want.imag)) if want.dtype.kind == "c" else ((got, want),)
    for g, w in parts:
        g, w = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        nan = np.isnan(w)
        if not np.array_equal(np.isnan(g), nan) or not np.array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64)):
            return False
    return True


def spacings(a, b):
    """|a - b| in float64 spacings (the count of doubles between them), elementwise; both finite and of one sign or zero."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)  # monotone in the value; -0.0 and +0.0 both 0
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------ building blocks
def pad_symm(a, n):
    """d c b a | a b c d | d c b a, any overshoot (refl_symm)."""
    return np.pad(a, n, mode="symmetric")


@quiet
def conv_in_order(padded, w, scale):
    """s = +0.0; for i: for j: s += (w[i] * w[j] * scale) * P[y + i][x + j]   (conv5 / conv3 of the 16 x 16 tile kernels)."""
    n = len(w)
    L, S = padded.shape[0] - n + 1, padded.shape[1] - n + 1
    s = np.zeros((L, S))
    for i in range(n):
        for j in range(n):
            s = s + (w[i] * w[j] * scale) * padded[i:i + L, j:j + S]
    return s


def conv5(a):
    return conv_in_order(pad_symm(a, 2), W5, 1.0 / 256.0)


def conv3(a):
    return conv_in_order(pad_symm(a, 1), W3, 1.0 / 16.0)


def quad(a):
    """The four members v00, v01, v10, v11 of every 2 x 2 group, the remainder trimmed."""
    L, S = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * L, :2 * S]
    return a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]


@quiet
def nanmean4(members, skip=None):
    """s = +0.0, cnt = 0; each member in turn: if it is not skipped: s += v, ++cnt; then s / cnt, NaN when cnt is 0.  skip: one
    bool array per member (default: the member's own NaN)."""
    s = np.zeros(members[0].shape)
    cnt = np.zeros(members[0].shape)
    for k, v in enumerate(members):
        use = ~(np.isnan(v) if skip is None else skip[k])
        s = np.where(use, s + v, s)
        cnt = cnt + use
    return np.where(cnt > 0, s / np.where(cnt > 0, cnt, 1.0), NAN)


@quiet
def rooted(x):
    """The root on load: in the input's dtype (numpy's float32 root is the correctly rounded one), widened afterwards."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64)
    return np.sqrt(x).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- k_grad_r2
@quiet
def r2_exact(x, root_on_load=False, take_sqrt=False):
    """k_grad_r2<T, SQ>: conv5 (symmetric border of the fine raster), the NaN-skipping 2 x 2 mean, conv3 (symmetric border of
    the COARSE raster), optional root."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and x.ndim == 2 and min(x.shape) >= 2
    a = rooted(x) if root_on_load else x.astype(np.float64)
    v = conv3(nanmean4(quad(conv5(a))))
    return np.sqrt(v) if take_sqrt else v


# ---------------------------------------------------------------------------------------------------- k_grad_local
@quiet
def hyp_centre(re, im):
    """sqrt(re**2 + im**2) in np.longdouble (63-bit mantissa), rounded to double."""
    assert np.finfo(np.longdouble).nmant >= 63
    r, i = np.asarray(re, dtype=np.longdouble), np.asarray(im, dtype=np.longdouble)
    return np.asarray(np.sqrt(r * r + i * i), dtype=np.float64)


def step(a, n):
    """`a` moved n float64 spacings (n < 0: down, clamped at 0 for the non-negative moduli this is used on); NaN stays."""
    a = np.array(a, dtype=np.float64)
    for _ in range(abs(n)):
        a = np.nextafter(a, np.inf if n > 0 else -np.inf)
    return np.maximum(a, 0.0) if n < 0 else a  # np.maximum keeps NaN


def hyp_lo(re, im):
    return step(hyp_centre(re, im), -HYPOT_STEPS)


def hyp_hi(re, im):
    return step(hyp_centre(re, im), HYPOT_STEPS)


@quiet
def grad2(ampl):
    """(re, im) of grad**2 per fine pixel: Scharr with the reflect-101 border, the statements as written (zero taps multiply),
    row pass then column pass; one NaN part makes both parts NaN."""
    p = np.pad(np.asarray(ampl, dtype=np.float64), 1, mode="reflect")
    hx = -1.0 * p[:, :-2] + 0.0 * p[:, 1:-1] + 1.0 * p[:, 2:]
    hy = 3.0 * p[:, :-2] + 10.0 * p[:, 1:-1] + 3.0 * p[:, 2:]
    dx = 3.0 * hx[:-2] + 10.0 * hx[1:-1] + 3.0 * hx[2:]
    dy = -1.0 * hy[:-2] + 0.0 * hy[1:-1] + 1.0 * hy[2:]
    nan = np.isnan(dx) | np.isnan(dy)
    dx, dy = np.where(nan, NAN, dx), np.where(nan, NAN, dy)
    return dx * dx - dy * dy, dx * dy + dy * dx


@quiet
def local_planes(ampl, hyp=hyp_centre):
    """(zr, zi, za) of k_grad_local: R2's steps on the planes re, im and hyp(re, im) of grad**2.  The complex pair skips a 2 x 2
    member when either part is NaN; the modulus plane skips on its own NaN.  zr and zi do not depend on `hyp`."""
    ampl = np.asarray(ampl)
    assert ampl.dtype == np.float64 and ampl.ndim == 2 and min(ampl.shape) >= 2
    re, im = grad2(ampl)
    ab = hyp(re, im)
    qr, qi, qa = quad(conv5(re)), quad(conv5(im)), quad(conv5(ab))
    skip = [np.isnan(r) | np.isnan(i) for r, i in zip(qr, qi)]
    return conv3(nanmean4(qr, skip)), conv3(nanmean4(qi, skip)), conv3(nanmean4(qa))


@quiet
def csqrt_exact(zr, zi, d):
    """csqrt_principal(x, y) with d standing for hypot(x, y): (real, imaginary, branch); branch 0: a NaN part (NaN, NaN),
    1: x == 0 and y == 0 (0.0, y), 2: x >= 0 (r, 0.5 * (y / r)), r = sqrt(0.5 * (d + x)), 3: x < 0 (|0.5 * (y / s)|,
    copysign(s, y)), s = sqrt(0.5 * (d - x))."""
    x, y = np.asarray(zr, dtype=np.float64), np.asarray(zi, dtype=np.float64)
    nan = np.isnan(x) | np.isnan(y)
    zero = (x == 0.0) & (y == 0.0)
    branch = np.where(nan, 0, np.where(zero, 1, np.where(x >= 0.0, 2, 3)))
    r = np.sqrt(0.5 * (d + x))
    s = np.sqrt(0.5 * (d - x))
    real = np.select([branch == 0, branch == 1, branch == 2], [NAN, 0.0, r], np.fabs(0.5 * (y / s)))
    imag = np.select([branch == 0, branch == 1, branch == 2], [NAN, y, 0.5 * (y / r)], np.copysign(s, y))
    return real, imag, branch


@quiet
def quality_exact(d, za, keep=np.less_equal):
    """c = d / (za + 0.00001), kept where c <= 1, else (above 1 or NaN) 0."""
    c = d / (za + 0.00001)
    return np.where(keep(c, 1.0), c, 0.0)


def local_exact(ampl, hyp=hyp_centre):
    """(G2 complex128, G3, c) of k_grad_local with one choice of hypot for both of its uses."""
    zr, zi, za = local_planes(ampl, hyp)
    d = hyp(zr, zi)
    re, im, _ = csqrt_exact(zr, zi, d)
    return re + 1j * im, za, quality_exact(d, za)


class LocalBracket:
    """What a k_grad_local whose hypot lies within HYPOT_STEPS spacings of the longdouble value can return for `ampl`.

    Everything after hypot is monotone in it: the sums have positive weights and a fixed order (IEEE +, x by a positive
    constant and / by a positive count are monotone), sqrt is, and so are the quotients of csqrt_principal and of c.  NaN
    positions and the skipped members of the 2 x 2 means do not depend on hypot's value.  So, with lo / hi the planes fed
    hyp_lo / hyp_hi:  za_lo <= G3 <= za_hi;  both parts of G2 lie between csqrt_exact(zr, zi, d_lo) and csqrt_exact(zr, zi, d_hi)
    (the two ends ordered per component), its real part has a clear sign bit and its imaginary part the sign of zi;
    d_lo / (za_hi + 1e-5) <= c <= d_hi / (za_lo + 1e-5) where both ends are <= 1.  `knife` marks c_lo <= 1 < c_hi (the cut to 0
    may fall either way), `above` c_lo > 1 (c is 0)."""

    def __init__(self, ampl):
        with np.errstate(invalid="ignore", divide="ignore"):
            self.zr, self.zi, self.za = local_planes(ampl, hyp_centre)
            _, _, self.za_lo = local_planes(ampl, hyp_lo)
            _, _, self.za_hi = local_planes(ampl, hyp_hi)
            self.d = hyp_centre(self.zr, self.zi)
            self.d_lo, self.d_hi = step(self.d, -HYPOT_STEPS), step(self.d, HYPOT_STEPS)
            self.re, self.im, self.branch = csqrt_exact(self.zr, self.zi, self.d)
            a = csqrt_exact(self.zr, self.zi, self.d_lo)
            b = csqrt_exact(self.zr, self.zi, self.d_hi)
            self.re_lo, self.re_hi = np.fmin(a[0], b[0]), np.fmax(a[0], b[0])
            self.im_lo, self.im_hi = np.fmin(a[1], b[1]), np.fmax(a[1], b[1])
            self.c = quality_exact(self.d, self.za)
            self.c_lo = self.d_lo / (self.za_hi + 0.00001)
            self.c_hi = self.d_hi / (self.za_lo + 0.00001)
            self.nan = np.isnan(self.c_lo)  # a NaN zr, zi or za: c is 0
            self.knife = (self.c_lo <= 1.0) & (self.c_hi > 1.0)
            self.above = self.c_lo > 1.0
        assert np.array_equal(np.isnan(self.za_lo), np.isnan(self.za)) and np.array_equal(np.isnan(self.za_hi), np.isnan(self.za))
        ok = ~np.isnan(self.za)
        assert (self.za_lo[ok] <= self.za[ok]).all() and (self.za[ok] <= self.za_hi[ok]).all()
        self.G2 = self.re + 1j * self.im

    def problems(self, G2, G3, c, exact=None):
        """The violations of the bracket by a device result, as strings (empty: inside).  G2 may be None.  exact: a mask of
        pixels where the centre restatement itself is demanded bit for bit (the Pythagorean ramp interiors)."""
        out = []

        def inside(name, v, lo, hi):
            v = np.asarray(v, dtype=np.float64)
            if not np.array_equal(np.isnan(v), np.isnan(lo)):
                out.append(f"{name}: NaN positions differ at {int((np.isnan(v) != np.isnan(lo)).sum())} pixels")
                return
            m = ~np.isnan(lo)
            bad = m & ~((v >= lo) & (v <= hi))  # plain float64 comparisons
            if bad.any():
                k = tuple(np.argwhere(bad)[0])
                out.append(f"{name}: {int(bad.sum())} pixels outside, first {k}: {v[k]!r} not in [{lo[k]!r}, {hi[k]!r}]")

        inside("G3", G3, self.za_lo, self.za_hi)
        if G2 is not None:
            G2 = np.asarray(G2)
            inside("G2.real", G2.real, self.re_lo, self.re_hi)
            inside("G2.imag", G2.imag, self.im_lo, self.im_hi)
            m = ~np.isnan(self.re)
            if np.signbit(G2.real[m]).any():
                out.append(f"G2.real: sign bit set at {int(np.signbit(G2.real[m]).sum())} pixels")
            if not np.array_equal(np.signbit(G2.imag[m]), np.signbit(self.im[m])):
                out.append(f"G2.imag: sign differs at {int((np.signbit(G2.imag[m]) != np.signbit(self.im[m])).sum())} pixels")
        c = np.asarray(c, dtype=np.float64)
        if np.isnan(c).any():
            out.append("c: NaN")
        else:
            zero = (c == 0.0) & ~np.signbit(c)
            ranged = (c >= self.c_lo) & (c <= np.minimum(self.c_hi, 1.0))
            ok = np.where(self.nan | self.above, zero, np.where(self.knife, ranged | zero, ranged))
            if not ok.all():
                k = tuple(np.argwhere(~ok)[0])
                out.append(f"c: {int((~ok).sum())} pixels outside, first {k}: {c[k]!r} not in [{self.c_lo[k]!r}, {self.c_hi[k]!r}]")
        if exact is not None and exact.any():
            for name, v, w in (("G3", G3, self.za), ("c", c, self.c)) + ((("G2", G2, self.G2),) if G2 is not None else ()):
                if not same_bits(np.asarray(v)[exact], w[exact]):
                    out.append(f"{name}: differs from the centre restatement on the exact pixels")
        return out

    def distances(self, G2, G3, c):
        """The largest distance, in spacings, of G3, the parts of G2 and c from the centre restatement (a record, no gate)."""
        d = {}
        m = ~np.isnan(self.za)
        d["G3"] = int(spacings(np.asarray(G3)[m], self.za[m]).max()) if m.any() else 0
        m = ~self.nan & ~self.knife & ~self.above
        d["c"] = int(spacings(np.asarray(c)[m], self.c[m]).max()) if m.any() else 0
        if G2 is not None:
            m = ~np.isnan(self.re)
            d["G2.real"] = int(spacings(np.asarray(G2).real[m], self.re[m]).max()) if m.any() else 0
            d["G2.imag"] = int(spacings(np.asarray(G2).imag[m], self.im[m]).max()) if m.any() else 0
        return d


# --------------------------------------------------------------------------------------- k_grad_smooth / k_grad_mean
@quiet
def smooth_exact(x, coarsen=False):
    """k_grad_smooth<COARSEN>: conv3's order over the raster itself or over coarsen_at's NaN-skipping mean (members in the order
    p[0], p[1], p[S], p[S + 1]), reflecting at the smoothed raster's own edge."""
    x = np.asarray(x, dtype=np.float64)
    return conv3(nanmean4(quad(x)) if coarsen else x)


@quiet
def sep_in_order(padded, w, axis, skip_zero_taps=False):
    """s = +0.0; for k: s += w[k] * P[.. + k] along `axis`, every tap multiplying (skip_zero_taps: the mutant that drops the
    taps of weight 0, tests only)."""
    n = len(w)
    m = padded.shape[axis] - n + 1
    s = np.zeros(tuple(m if a == axis else padded.shape[a] for a in range(2)))
    for k in range(n):
        if skip_zero_taps and w[k] == 0.0:
            continue
        s = s + w[k] * (padded[k:k + m] if axis == 0 else padded[:, k:k + m])
    return s


def mean_stage1(x):
    """B4 of mean_tile: along the sample axis then along lines (s += w5(j) * a[j], w5 = k / 16), the input reflected symmetrically."""
    return sep_in_order(sep_in_order(pad_symm(np.asarray(x, dtype=np.float64), 2), W5_16, 1), W5_16, 0)


@quiet
def mean_exact(x, skip_zero_taps=False):
    """mean_tile: `mean_stage1`, then the RESULT reflected symmetrically and all nine taps of w9 per axis, the zero taps
    multiplying, samples then lines."""
    rows = sep_in_order(pad_symm(mean_stage1(x), 4), W9_16, 1, skip_zero_taps)
    return sep_in_order(rows, W9_16, 0, skip_zero_taps)


# ---------------------------------------------------------------------------------------------------- k_grad_filter
@quiet
def zoom_exact(q4, shape):
    """The bilinear sample of k_grad_filter: zoom_tap's taps and weights (filtering_ref.zoom_axis states them), then
    z = +0.0; z += q[y0][x0] * wy0 * wx0; z += q[y0][x1] * wy0 * wx1; z += q[y1][x0] * wy1 * wx0; z += q[y1][x1] * wy1 * wx1,
    0.0 where a coordinate lies outside."""
    q4 = np.asarray(q4, dtype=np.float64)
    y0, y1, wy0, wy1, iny = fr.zoom_axis(q4.shape[0], shape[0])
    x0, x1, wx0, wx1, inx = fr.zoom_axis(q4.shape[1], shape[1])
    wy0, wy1 = wy0[:, None], wy1[:, None]
    z = np.zeros(shape)
    z = z + q4[np.ix_(y0, x0)] * wy0 * wx0
    z = z + q4[np.ix_(y0, x1)] * wy0 * wx1
    z = z + q4[np.ix_(y1, x0)] * wy1 * wx0
    z = z + q4[np.ix_(y1, x1)] * wy1 * wx1
    return np.where(iny[:, None] & inx[None, :], z, 0.0)


def clip01(v):
    """v < 0 -> 0.0, v > 1 -> 1.0, else v: NaN passes (np.clip's result)."""
    with np.errstate(invalid="ignore"):
        return np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))


@quiet
def filter_terms(r2, g3):
    """(J, J1, G4, d = J1 - J * J) of k_grad_filter's three Means."""
    r2, g3 = np.asarray(r2, dtype=np.float64), np.asarray(g3, dtype=np.float64)
    J, J1, G4 = mean_exact(r2), mean_exact(r2 * r2), mean_exact(g3)
    return J, J1, G4, J1 - J * J


@quiet
def filter_exact(r2, g3, c, q4, clamp_d=False):
    """k_grad_filter's output [5][L][S] = f1, f2, f3, f4, F.  clamp_d: the mutant that clamps J1 - J**2 at 0 (tests only)."""
    r2, g3, c = (np.asarray(a, dtype=np.float64) for a in (r2, g3, c))
    J, J1, G4, d = filter_terms(r2, g3)
    if clamp_d:
        d = np.where(d < 0.0, 0.0, d)
    P1 = np.sqrt(d) / (J + 0.00001)
    K = r2 - zoom_exact(q4, r2.shape)
    P2 = K * K / (J * J + 0.00001)
    P3 = g3 / (G4 + 0.00001)
    P4 = np.sqrt(c)
    f1, f2 = clip01(-50.0 * P1 + 2.75), clip01(-5000.0 * P2 + 3.0)
    f3, f4 = clip01(-2.5 * P3 + 4.0), clip01(-10.0 * P4 + 6.3)
    F = np.sqrt(1.0 / 4.0 * (f1 * f1 + f2 * f2 + f3 * f3 + f4 * f4))
    return np.stack([f1, f2, f3, f4, F])
