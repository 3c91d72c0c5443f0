"""The inversion kernels' tile walk (csrc/xsw_tilewalk.hpp), restated in Python.

A raster of `strips` tile columns and `lg` line groups is walked by 8 * C * lg workgroup slots (xcd, y, g), C = ceil(strips / 8).
With base = strips // 8 and R = strips % 8:
  * y < base: tile column xcd * base + y, line group g;
  * y == base (R > 0 only): the R * lg leftover tiles, numbered t = (column - 8 * base) * lg + line group, in eight contiguous
    shares of q = ceil(R * lg / 8): XCD xcd takes t = xcd * q + g for g < q and t < R * lg;
  * every other slot has no tile.
"""
import numpy as np


def cols_per_xcd(strips):
    return (strips + 7) // 8


def share(strips, lg):
    """q: the leftover tiles one XCD takes at most."""
    return -(-((strips % 8) * lg) // 8)


def tile_walk(strips, lg, xcd, y, g):
    """Slot -> (tile column, line group), or None."""
    base, rem = divmod(strips, 8)
    if y < base:
        return xcd * base + y, g
    if y > base or rem == 0:
        return None
    q = share(strips, lg)
    t = xcd * q + g
    if g >= q or t >= rem * lg:
        return None
    return 8 * base + t // lg, t % lg


def tile_map(strips, lg):
    """int32 [8, C, lg, 2]: (tile column, line group) of every slot, (-1, -1) where there is none.  Vectorised, same rule."""
    base, rem = divmod(strips, 8)
    C = cols_per_xcd(strips)
    m = np.full((8, C, lg, 2), -1, dtype=np.int32)
    if base:
        m[:, :base, :, 0] = np.arange(8).reshape(8, 1, 1) * base + np.arange(base).reshape(1, base, 1)
        m[:, :base, :, 1] = np.arange(lg).reshape(1, 1, lg)
    if rem:
        q = share(strips, lg)
        g = np.arange(lg, dtype=np.int64).reshape(1, lg)
        t = np.arange(8, dtype=np.int64).reshape(8, 1) * q + g  # [8, lg]
        ok = (g < q) & (t < rem * lg)
        m[:, base, :, 0] = np.where(ok, 8 * base + t // lg, -1)
        m[:, base, :, 1] = np.where(ok, t % lg, -1)
    return m


def old_tile_map(strips, lg):
    """The walk before the leftover columns were shared: XCD x owns the columns [x * C, x * C + C)."""
    C = cols_per_xcd(strips)
    col = np.arange(8)[:, None, None] * C + np.arange(C)[None, :, None] + np.zeros((1, 1, lg), dtype=np.int64)
    grp = np.zeros((8, C, 1), dtype=np.int64) + np.arange(lg)[None, None, :]
    ok = col < strips
    return np.stack([np.where(ok, col, -1), np.where(ok, grp, -1)], axis=-1).astype(np.int32)
