"""numpy restatement of the wind direction at a known speed (include/xsw.h: xsw_dir_solve): the inverse of
the forward operator (tests/forward_ref.py) along the direction axis.  Per pixel, in float64, with only IEEE + - * / (and fmod,
which is exact) in the order written here:

  gate       inc, w or s NaN, inc or w outside its axis, s not finite: reals NaN, count 0, flag NAN
  cells      forward_ref's (hi = clip(searchsorted(axis, x, side left), 1, n - 1)) on the incidence and the speed axis
  d(j)       lerp_w(lerp_inc(T[il][wl][j], T[ih][wl][j]), lerp_inc(T[il][wh][j], T[ih][wh][j])): incidence first, then speed
  scan       every cell k = 0 .. n_phi - 2: it holds a solution iff d(k) <= s < d(k+1), or d(k) >= s > d(k+1), or k == n_phi - 2 and
             s == d(k+1) (and d(k) is no NaN)
  solution   slope = (d(k+1) - d(k)) / (p[k+1] - p[k]); phi = p[k] + (s - d(k)) / slope, p[k] where d(k+1) == d(k), clamped to
             [p[k], p[k+1]]; sens = 1 / slope
  outputs    phi1 / phi2, sens1 / sens2: the first and second solution in scan order; count = min(number of such cells, 255);
             flag MORE where more than two; no such cell: BELOW where s < d(0), ABOVE where s > d(0), else NAN
  closest    p[j] of the first node j that minimises |d(j) - s| among the nodes with a finite d (NaN when there is none)
  selection  near given: in scan order every solution +phi and, fold_phi, -phi right after it; r = fmod(c - near, 360); r < 0:
             r = r + 360; dist = r > 180 ? 360 - r : r; the candidate of the smallest dist, strict < (the earlier one on a tie);
             sens_near its sens, negated for a mirrored candidate

`count_dense` is the plain meaning of `count`, kept as a second function: the sign changes of forward_ref's own interpolant minus
s on a grid of 64 directions per cell."""
import numpy as np

import forward_ref as fref
from forward_ref import _cell, _lerp

NAN, BELOW, ABOVE, MORE = 1, 2, 4, 8
REALS = ("phi1", "phi2", "sens1", "sens2", "phi_near", "sens_near", "phi_closest")
FIELDS = REALS + ("count", "flag")


def node_values(table, ai, aw, inc, w):
    """[pixels][n_phi]: d(j) of the definition at every pixel (flat arrays; a pixel outside the axes gets its clipped cell)."""
    table, ai, aw = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw))
    inc, w = (np.asarray(v, dtype=np.float64).ravel() for v in (inc, w))
    il, ih, _ = _cell(ai, inc)
    wl, wh, _ = _cell(aw, w)
    i0, i1, x = ai[il][:, None], ai[ih][:, None], inc[:, None]
    with np.errstate(all="ignore"):
        a = _lerp(table[il, wl, :], table[ih, wl, :], i0, i1, x)[1]
        b = _lerp(table[il, wh, :], table[ih, wh, :], i0, i1, x)[1]
        return _lerp(a, b, aw[wl][:, None], aw[wh][:, None], w[:, None])[1]


def distance(c, near):
    """The selection's distance on the circle, in [0, 180] (NaN with a NaN among them)."""
    with np.errstate(invalid="ignore"):
        r = np.fmod(c - near, 360.0)
        r = np.where(r < 0, r + 360.0, r)
        return np.where(r > 180.0, 360.0 - r, r)


def _solve_gated(D, ap, s, near, fold_phi):
    """The definition on gated pixels: D [m][n_phi] node values, s [m], near [m] or None -> dict of [m] arrays."""
    m, n_phi = D.shape
    a, b, x = D[:, :-1], D[:, 1:], s[:, None]
    p0, p1 = ap[None, :-1], ap[None, 1:]
    is_last = (np.arange(n_phi - 1) == n_phi - 2)[None, :]
    with np.errstate(all="ignore"):
        hit = ((a <= x) & (x < b)) | ((a >= x) & (x > b)) | (is_last & (x == b) & ~np.isnan(a))
        slope = (b - a) / (p1 - p0)
        phi = np.where(b == a, p0, p0 + (x - a) / slope)
        phi = np.where(phi < p0, p0, phi)
        phi = np.where(phi > p1, p1, phi)
        sens = 1.0 / slope
    n = hit.sum(axis=1)
    rank = np.cumsum(hit, axis=1)
    out = {}
    for which in (1, 2):
        at = hit & (rank == which)
        have = at.any(axis=1)
        k = at.argmax(axis=1)
        out[f"phi{which}"] = np.where(have, phi[np.arange(m), k], np.nan)
        out[f"sens{which}"] = np.where(have, sens[np.arange(m), k], np.nan)
    out["n"] = n
    out["count"] = np.minimum(n, 255).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        d0 = D[:, 0]
        none = np.where(s < d0, BELOW, np.where(s > d0, ABOVE, NAN))
    out["flag"] = np.where(n == 0, none, np.where(n > 2, MORE, 0)).astype(np.uint8)
    # the closest node: the first finite one that minimises |d - s| (which may itself overflow to inf)
    fin = np.isfinite(D)
    with np.errstate(all="ignore"):
        err = np.where(fin, np.abs(D - x), np.inf)
    j = err.argmin(axis=1)
    j = np.where(fin[np.arange(m), j], j, fin.argmax(axis=1))  # (every error inf: the first finite node)
    out["phi_closest"] = np.where(fin.any(axis=1), ap[j], np.nan)
    out["phi_near"], out["sens_near"] = np.full(m, np.nan), np.full(m, np.nan)
    if near is not None:
        best = np.full(m, np.inf)
        for k in range(n_phi - 1):  # scan order; +phi, then its mirror image
            if not hit[:, k].any():
                continue
            for sign in (1.0, -1.0) if fold_phi else (1.0,):
                c = sign * phi[:, k]
                with np.errstate(invalid="ignore"):
                    better = hit[:, k] & (distance(c, near) < best)
                best = np.where(better, distance(c, near), best)
                out["phi_near"] = np.where(better, c, out["phi_near"])
                out["sens_near"] = np.where(better, sign * sens[:, k], out["sens_near"])
    return out


def solve(table, ai, aw, ap, inc, s, w, near=None, fold_phi=True, chunk=4000):
    """dict(phi1, phi2, sens1, sens2, phi_near, sens_near, phi_closest: float64; count, flag: uint8; n: the unsaturated number of
    solutions, for the comparison with `count_dense` only) of inc's shape, for the co-pol table[i][w][p]."""
    table, ai, aw, ap = (np.asarray(v, dtype=np.float64) for v in (table, ai, aw, ap))
    inc, s, w = (np.asarray(v).astype(np.float64) for v in (inc, s, w))
    shape, size = inc.shape, inc.size
    inc, s, w = inc.ravel(), s.ravel(), w.ravel()
    near = None if near is None else np.asarray(near).astype(np.float64).ravel()
    with np.errstate(invalid="ignore"):
        ok = (inc >= ai[0]) & (inc <= ai[-1]) & (w >= aw[0]) & (w <= aw[-1]) & np.isfinite(s)
    at = np.flatnonzero(ok)
    out = {k: np.full(size, np.nan) for k in REALS}
    out["count"], out["flag"], out["n"] = np.zeros(size, np.uint8), np.full(size, NAN, np.uint8), np.zeros(size, np.int64)
    for c0 in range(0, len(at), chunk):
        q = at[c0:c0 + chunk]
        r = _solve_gated(node_values(table, ai, aw, inc[q], w[q]), ap, s[q], None if near is None else near[q], fold_phi)
        for k, v in r.items():
            out[k][q] = v
    return {k: v.reshape(shape) for k, v in out.items()}


def count_dense(table, ai, aw, ap, inc, s, w, per_cell=64, chunk=16):
    """The number of directions on [ap[0], ap[-1]] at which forward_ref's interpolant takes the value s, by its sign changes on a
    grid of `per_cell` directions per cell (and the last node): for s off the node values.  Flat arrays, all inside the axes."""
    ap = np.asarray(ap, dtype=np.float64)
    inc, s, w = (np.asarray(v, dtype=np.float64).ravel() for v in (inc, s, w))
    t = np.arange(per_cell) / per_cell
    grid = np.append((ap[:-1, None] + (ap[1:] - ap[:-1])[:, None] * t[None, :]).ravel(), ap[-1])
    out = np.zeros(len(inc), np.int64)
    for c0 in range(0, len(inc), chunk):
        q = slice(c0, c0 + chunk)
        sim = fref.eval_co(table, ai, aw, ap, inc[q, None], w[q, None], grid[None, :], fold_phi=False)["sigma0_db"]
        above = sim > s[q, None]
        out[q] = np.sum(above[:, 1:] != above[:, :-1], axis=1)
    return out


# ------------------------------------------------------------------------------------------------ hand-made tables
# co[2][2][n_phi] = row[j] + 2 i + 4 w on the axes ai = (20, 24), aw = (2, 6): at a node of incidence and speed every d(j) is the
# row's entry plus an integer, exactly; midway (inc 22, w 4) it is row[j] + 3.
def _table(row, ap=None):
    row = np.asarray(row, dtype=np.float64)
    ap = np.linspace(0.0, 180.0, len(row)) if ap is None else np.asarray(ap, dtype=np.float64)
    co = row[None, None, :] + 2.0 * np.arange(2)[:, None, None] + 4.0 * np.arange(2)[None, :, None]
    return co, np.array([20.0, 24.0]), np.array([2.0, 6.0]), ap


def wavy_table():
    """A column that crosses s = -12 four times (cells 0 .. 3), then stays above it: MORE, and a selection among four solutions
    and their mirror images.  Directions 0, 30, .. 180."""
    return _table([-10.0, -14.0, -10.0, -14.0, -10.0, -9.0, -8.0])


def zigzag_table(n_phi=301):
    """A column that crosses s = -12 in every one of its n_phi - 1 cells: the saturating count."""
    return _table(np.where(np.arange(n_phi) % 2 == 0, -10.0, -14.0))


def flat_table():
    """Two flat runs at s = -12: one ends inside the axis (nodes 1 .. 3; counted once, in cell 3, at 90 degrees), one at the last
    node (nodes 5, 6; counted once, in the last cell, which is flat: 150 degrees, infinite sensitivity)."""
    return _table([-10.0, -12.0, -12.0, -12.0, -15.0, -12.0, -12.0])


def nan_table():
    """A NaN at node 1 and one at the last-but-one node: the cells on either side of a NaN hold nothing, not even s on the last
    node.  Directions 0, 36, .. 180."""
    return _table([-10.0, np.nan, -14.0, -10.0, np.nan, -12.0])


def monotone_table():
    """A column that falls from 0 to 180 degrees: one solution, or none."""
    return _table([-8.0, -9.0, -11.0, -12.0, -16.0], ap=[0.0, 20.0, 50.0, 120.0, 180.0])
