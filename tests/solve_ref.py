"""numpy restatement of the wind speed at a known direction (include/xsw.h: xsw_wspd_solve,
xsw_wspd_solve_cr): the inverse of the forward operator (tests/forward_ref.py) along the wind-speed axis.  Per pixel, in float64,
with only IEEE + - * / in the order written here:

  fold, cells            forward_ref's (fold_phi; hi = clip(searchsorted(axis, x, side left), 1, n - 1))
  gate                   inc, phi or s NaN, inc or phi (after the fold) outside its axis, s not finite: NaN, flag NAN
  c(k)                   lerp over direction of lerp_inc(T[il][k][pl], T[ih][k][pl]) and lerp_inc(T[il][k][ph], T[ih][k][ph]):
                         incidence first, then direction (cross-pol: lerp_inc(T[il][k], T[ih][k]))
  bracket                M = min(mono_rows[il], mono_rows[ih]) (cross-pol: n_w if cr_monotone else 0).  M >= 2: lo, hi = 0, M - 1;
                         while lo < hi: mid = (lo + hi) >> 1; c(mid) < s ? lo = mid + 1 : hi = mid.  j = lo;
                         c(j) >= s and j > 0: k = j - 1;  j == 0 and c(0) == s: k = 0;  else none
  tail                   none yet: k from max(M - 1, 0) to n_w - 2, the first with min(c(k), c(k+1)) <= s <= max(c(k), c(k+1)); flag TAIL.
                         None: NaN; BELOW where s < c(0), ABOVE where s > c(0) (NAN where neither: a NaN in the table)
  solution               slope = (c(k+1) - c(k)) / (aw[k+1] - aw[k]); w = aw[k] + (s - c(k)) / slope, aw[k] where c(k+1) == c(k),
                         clamped to [aw[k], aw[k+1]]; sens = 1 / slope

`mono_rows` / `cr_monotone` restate what the LUT install derives (csrc/xsw_lutbuild.hpp k_mono_rows, csrc/xsw_lutplan.hpp CrPlan).
`solve_*_scan` is the plain meaning, kept as a second function: the first bracketing cell by a linear scan from row 0."""
import numpy as np

from forward_ref import _cell, _lerp, fold

NAN, BELOW, ABOVE, TAIL = 1, 2, 4, 8


def mono_rows(table):
    """[n_inc]: index of the first row of slice i that is lower than its predecessor in some column, n_w when none."""
    table = np.asarray(table, dtype=np.float64)
    drop = np.any(table[:, 1:, :] < table[:, :-1, :], axis=2)  # [n_inc][n_w - 1]
    return np.where(drop.any(axis=1), drop.argmax(axis=1) + 1, table.shape[1]).astype(np.int64)


def cr_monotone(table, aw):
    """The table is finite, its speed axis uniform (to 1e-12) and every row non-decreasing."""
    table, aw = np.asarray(table, dtype=np.float64), np.asarray(aw, dtype=np.float64)
    n = len(aw)
    if n < 2 or not np.isfinite(table).all():
        return False
    step = (aw[-1] - aw[0]) / (n - 1)
    if not (step > 0 and np.isfinite(step)):
        return False
    tol = 1e-12 * max(abs(aw[0]), abs(aw[-1]), step)
    if not np.all(np.abs(aw - (aw[0] + np.arange(n) * step)) <= tol):
        return False
    return not np.any(table[:, 1:] < table[:, :-1])


class _Column:
    """c(k) of a set of pixels, all inside the axes: k an int array of the pixels' length -> their node values."""

    def __init__(self, table, ai, ap, inc, p):
        self.table, self.ai, self.ap, self.inc, self.p = table, ai, ap, inc, p
        self.il, self.ih, _ = _cell(ai, inc)
        if ap is not None:
            self.pl, self.ph, _ = _cell(ap, p)

    def pick(self, at):
        out = object.__new__(_Column)
        out.table, out.ai, out.ap = self.table, self.ai, self.ap
        for name in ("inc", "p", "il", "ih") + (("pl", "ph") if self.ap is not None else ()):
            v = getattr(self, name)
            setattr(out, name, None if v is None else v[at])
        return out

    def __call__(self, k):
        t, ai, il, ih = self.table, self.ai, self.il, self.ih
        with np.errstate(all="ignore"):
            if self.ap is None:
                return _lerp(t[il, k], t[ih, k], ai[il], ai[ih], self.inc)[1]
            u0 = _lerp(t[il, k, self.pl], t[ih, k, self.pl], ai[il], ai[ih], self.inc)[1]
            u1 = _lerp(t[il, k, self.ph], t[ih, k, self.ph], ai[il], ai[ih], self.inc)[1]
            return _lerp(u0, u1, self.ap[self.pl], self.ap[self.ph], self.p)[1]

    def all_rows(self, n_w):
        """[pixels][n_w]: the same elementwise statements, broadcast over the rows"""
        wide = self.pick(slice(None))
        for name in ("inc", "p", "il", "ih") + (("pl", "ph") if self.ap is not None else ()):
            v = getattr(self, name)
            setattr(wide, name, None if v is None else v[:, None])
        return wide(np.arange(n_w)[None, :])


def _first_bracket(C, s, start):
    """First k >= start[pixel] with min(C[k], C[k+1]) <= s <= max(C[k], C[k+1]), -1 when none.  C: [pixels][n_w]."""
    a, b, x = C[:, :-1], C[:, 1:], s[:, None]
    hit = (((a <= x) & (x <= b)) | ((b <= x) & (x <= a))) & (np.arange(C.shape[1] - 1)[None, :] >= start[:, None])
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def _solution(col, aw, s, k, flag, n):
    """dict(wspd, sens, flag, k) over n pixels from the bracket k (-1: none) of the pixels `col` holds (index array col.at)."""
    wspd, sens, kk = np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1, np.int64)
    ok = k >= 0
    if ok.any():
        c, kq, sq = col.pick(ok), k[ok], s[ok]
        ck, ck1, w0, w1 = c(kq), c(kq + 1), aw[kq], aw[kq + 1]
        with np.errstate(all="ignore"):
            slope = (ck1 - ck) / (w1 - w0)
            x = np.where(ck1 == ck, w0, w0 + (sq - ck) / slope)
            x = np.where(x < w0, w0, x)
            x = np.where(x > w1, w1, x)
            at = col.at[ok]
            wspd[at], sens[at], kk[at] = x, 1.0 / slope, kq
    out_flag = np.full(n, NAN, np.uint8)
    out_flag[col.at] = flag
    return dict(wspd=wspd, sens=sens, flag=out_flag, k=kk)


def _solve(col, aw, s, M, n):
    """The definition on the gated pixels `col` (their raster positions col.at, sigma0 s, leading rows M)."""
    m = len(s)
    n_w = len(aw)
    k = np.full(m, -1, np.int64)
    flag = np.zeros(m, np.uint8)
    bis = M >= 2
    lo, hi = np.zeros(m, np.int64), np.where(bis, M - 1, 0)
    while True:
        act = np.flatnonzero(lo < hi)
        if not len(act):
            break
        mid = (lo[act] + hi[act]) >> 1
        less = col.pick(act)(mid) < s[act]
        lo[act] = np.where(less, mid + 1, lo[act])
        hi[act] = np.where(less, hi[act], mid)
    cj = col(lo)
    k = np.where(bis & (cj >= s) & (lo > 0), lo - 1, k)
    k = np.where(bis & (lo == 0) & (cj == s), 0, k)
    rest = np.flatnonzero(k < 0)
    if len(rest):
        sub = col.pick(rest)
        found = _first_bracket(sub.all_rows(n_w), s[rest], np.maximum(M[rest] - 1, 0))
        k[rest] = found
        c0 = sub(np.zeros(len(rest), np.int64))
        flag[rest] = np.where(found >= 0, TAIL, np.where(s[rest] < c0, BELOW, np.where(s[rest] > c0, ABOVE, NAN)))
    return _solution(col, aw, s, k, flag, n)


def _gated(table, ai, ap, inc, s, p):
    """(column of the pixels that pass the gate, with their raster positions in .at; their s)."""
    with np.errstate(invalid="ignore"):
        ok = (inc >= ai[0]) & (inc <= ai[-1]) & np.isfinite(s)
        if ap is not None:
            ok &= (p >= ap[0]) & (p <= ap[-1])
    at = np.flatnonzero(ok)
    col = _Column(table, ai, ap, inc[at], None if ap is None else p[at])
    col.at = at
    return col, s[at]


def _prepare_co(table, ai, aw, ap, inc, s, phi, fold_phi):
    table, ai, aw, ap = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw, ap))
    inc, s, phi = (np.asarray(v).astype(np.float64) for v in (inc, s, phi))
    shape = inc.shape
    inc, s, phi = inc.ravel(), s.ravel(), phi.ravel()
    p = fold(phi, ap[-1])[0] if fold_phi else phi
    col, sg = _gated(table, ai, ap, inc, s, p)
    return table, ai, aw, ap, shape, col, sg


def node_values(table, ai, ap, inc, phi, k, fold_phi=True):
    """c(k) of the definition at every pixel (flat arrays, all inside the axes; ap None: cross-pol): for tests that put sigma0
    exactly on a node value."""
    table, ai = np.asarray(table, dtype=np.float64), np.asarray(ai, dtype=np.float64)
    inc = np.asarray(inc, dtype=np.float64)
    if ap is None:
        return _Column(table, ai, None, inc, None)(np.asarray(k))
    ap = np.asarray(ap, dtype=np.float64)
    p = fold(phi, ap[-1])[0] if fold_phi else np.asarray(phi, dtype=np.float64)
    return _Column(table, ai, ap, inc, p)(np.asarray(k))


def _shaped(out, shape):
    return {name: v.reshape(shape) for name, v in out.items()}


def solve_co(table, ai, aw, ap, inc, s, phi, fold_phi=True, mono=None):
    """dict(wspd, sens, flag, k) for the co-pol table[i][w][p]; mono: its mono_rows (default: derived as the install derives them).
    k is the bracketing cell (-1: none), for the comparison with `solve_co_scan` only."""
    table, ai, aw, ap, shape, col, sg = _prepare_co(table, ai, aw, ap, inc, s, phi, fold_phi)
    mono = mono_rows(table) if mono is None else np.asarray(mono, dtype=np.int64)
    M = np.minimum(mono[col.il], mono[col.ih])
    return _shaped(_solve(col, aw, sg, M, int(np.prod(shape))), shape)


def solve_cr(table, ai, aw, inc, s, monotone=None):
    """dict(wspd, sens, flag, k) for the cross-pol table[i][w]; monotone: its cr_monotone (default: derived)."""
    table, ai, aw = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw))
    inc, s = (np.asarray(v).astype(np.float64) for v in (inc, s))
    shape = inc.shape
    col, sg = _gated(table, ai, None, inc.ravel(), s.ravel(), None)
    monotone = cr_monotone(table, aw) if monotone is None else monotone
    M = np.full(len(sg), len(aw) if monotone else 0, np.int64)
    return _shaped(_solve(col, aw, sg, M, int(np.prod(shape))), shape)


def _scan(col, aw, s, n, chunk=4000):
    """The plain meaning: the first bracketing cell from row 0 (flag: 0 or NAN only; TAIL / BELOW / ABOVE are the definition's)."""
    k = np.full(len(s), -1, np.int64)
    for a in range(0, len(s), chunk):
        at = np.arange(a, min(a + chunk, len(s)))
        k[at] = _first_bracket(col.pick(at).all_rows(len(aw)), s[at], np.zeros(len(at), np.int64))
    return _solution(col, aw, s, k, np.zeros(len(s), np.uint8), n)


def solve_co_scan(table, ai, aw, ap, inc, s, phi, fold_phi=True):
    table, ai, aw, ap, shape, col, sg = _prepare_co(table, ai, aw, ap, inc, s, phi, fold_phi)
    return _shaped(_scan(col, aw, sg, int(np.prod(shape))), shape)


def solve_cr_scan(table, ai, aw, inc, s):
    table, ai, aw = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw))
    inc, s = (np.asarray(v).astype(np.float64) for v in (inc, s))
    col, sg = _gated(table, ai, None, inc.ravel(), s.ravel(), None)
    return _shaped(_scan(col, aw, sg, inc.size), inc.shape)


def turnover_table():
    """(co, ai, aw, ap, mono): a hand-made co[3][8][2] that rises, falls and rises again along the speed, the same in both
    directions and shifted by the incidence, with a flat cell; the slices' monotone rows differ (4, 3, 8: the last slice rises
    throughout).  Small integers: every operation on it is exact for coordinates on multiples of 1/8."""
    ai, aw, ap = np.array([20.0, 24.0, 28.0]), np.array([1.0, 2.0, 4.0, 5.0, 7.0, 8.0, 10.0, 12.0]), np.array([0.0, 16.0])
    rows = np.array([[-20.0, -16.0, -12.0, -12.0, -18.0, -22.0, -14.0, -6.0],     # flat cell 2, falls from row 4, rises from row 5
                     [-24.0, -20.0, -14.0, -18.0, -24.0, -26.0, -18.0, -10.0],    # falls from row 3
                     [-28.0, -24.0, -20.0, -18.0, -16.0, -14.0, -12.0, -10.0]])   # rises throughout
    co = np.repeat(rows[:, :, None], 2, axis=2) + np.array([0.0, 2.0])[None, None, :]
    return co, ai, aw, ap, np.array([4, 3, 8])


def falling_table():
    """(co, ai, aw, ap, mono): every column falls from the first row on: the scan alone."""
    ai, aw, ap = np.array([20.0, 24.0]), np.array([1.0, 2.0, 4.0, 8.0]), np.array([0.0, 16.0, 32.0])
    co = -10.0 - 2.0 * aw[None, :, None] - 0.25 * (ai - 20.0)[:, None, None] + 0.125 * ap[None, None, :]
    return co, ai, aw, ap, np.array([1, 1])


def nonmonotone_cr():
    """(cr, ai, aw): a cross-pol table on a uniform speed axis whose rows rise, fall and rise again (cr_monotone = 0)."""
    ai, aw = np.array([20.0, 30.0, 45.0]), np.arange(1.0, 10.0)
    row = np.array([-30.0, -26.0, -22.0, -24.0, -27.0, -27.0, -21.0, -15.0, -12.0])
    return row[None, :] - 0.25 * (ai - 20.0)[:, None], ai, aw
