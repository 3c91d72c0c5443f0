"""The inputs at which the GPU tests run k_grad_keep with SEVERAL OUTPUT ROWS PER WORKGROUP (tests/test_gpu_strips.py), one per
keep entry of tests/strip_shapes.py, built with numpy alone; tests/test_masked_gradients_cpu.py asserts on the restatement
(masked_ref.keep_blocks) that they can tell a kernel that stops after its first row, or reads it again, from a right one.

Background: every element usable, then single unusable elements at random flat positions, so many that about 0.3 of the blocks
lose one; float rasters also hold the threshold itself and +inf, both kept.  and_with is non-zero on 0.8 of the output grid.

Probes: every output row of strip_shapes.probe_lines (the second workgroup row: each position u = 0..3 of its unrolled group
and the tail rows behind it; the last, short workgroup row) is rewritten block by block.  A random half of its blocks, at least
one, is made unusable by ONE element; the n-th such block of an entry has it at block row i = n % b and column
j = (n // b + n) % b, which walks through every (i, j) of the block while n < b * b, and through every i and every j on their
own once n >= b -- so through every row of the block and every lane and byte of its vectors.  The other blocks of the row, at
least one, are usable by the narrowest margin.
  float64  the element is NaN, -inf or the double just below the threshold in turn, and its neighbours in the block row are the
           threshold itself, which is kept; a usable block holds the threshold and +inf at the rotated position.
  uint8    the block is filled with 0x01, 0x80 and 0xFF, the bytes the borrow of the kernel's zero-byte test travels through, and
           the element is a lone 0x00 among them; a usable block is the same fill without it.
and_with is non-zero along every probe row but for ONE zero on a block that is usable, a different column in each row."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import strip_shapes

THRESHOLD = 0.25
BELOW = np.nextafter(THRESHOLD, -np.inf)
BAD_F64 = (np.nan, -np.inf, BELOW)
NEIGHBOURS = np.array([0x01, 0x80, 0xFF], np.uint8)

KEYS = sorted(k for k, e in strip_shapes.SHAPES.items() if e.kernel == "keep")

# src: the input raster; threshold: None for uint8; and_with: uint8 on the output grid; bad / good: the (Y, X) output pixels of
# the probe blocks made unusable / left usable; holes: the (Y, X) of and_with's lone zeros; at: (i, j) of every bad probe
KeepCase = namedtuple("KeepCase", "key src threshold block and_with bad good holes at")


def probe_position(n, b):
    return n % b, (n // b + n) % b


@functools.lru_cache(maxsize=1)
def case(key):
    """The KeepCase of one entry; its arrays are read-only and shared by everything that asks for the same key in a row."""
    e = strip_shapes.SHAPES[key]
    assert e.kernel == "keep"
    b, L, S = e.reduce, e.lines, e.samples
    Lo, So = L // b, S // b
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    is_float = e.dtype == "float64"
    if is_float:
        src = rng.uniform(THRESHOLD + 0.01, 1.0, (L, S))
        flat = src.reshape(-1)
        kept = rng.integers(0, flat.size, flat.size // 50)
        flat[kept] = np.where(rng.random(kept.size) < 0.5, THRESHOLD, np.inf)
    else:
        src = rng.integers(1, 256, (L, S), dtype=np.uint8)
        flat = src.reshape(-1)
    lost = rng.integers(0, flat.size, int(flat.size * (1.0 - 0.7 ** (1.0 / (b * b)))))
    flat[lost] = np.asarray(BAD_F64)[np.arange(lost.size) % 3] if is_float else 0
    and_with = np.where(rng.random((Lo, So)) < 0.8, rng.integers(1, 256, (Lo, So)), 0).astype(np.uint8)

    bad, good, holes, at = [], [], [], []
    for m, Y in enumerate(strip_shapes.probe_lines(key)):
        unusable = rng.random(So) < 0.5
        unusable[(3 * m) % So], unusable[(3 * m + 1) % So] = True, False   # at least one of each
        for X in range(So):
            blk = src[Y * b:(Y + 1) * b, X * b:(X + 1) * b]
            n = len(bad)
            i, j = probe_position(n, b)
            if is_float:
                blk[...] = rng.uniform(THRESHOLD + 0.01, 1.0, (b, b))
                if unusable[X]:
                    blk[i, :] = THRESHOLD
                    blk[i, j] = BAD_F64[n % 3]
                else:
                    blk[i, j], blk[(i + 1) % b, (j + 1) % b] = THRESHOLD, np.inf
            else:
                r, c = np.mgrid[0:b, 0:b]
                blk[...] = NEIGHBOURS[(r + c + n) % 3]
                if unusable[X]:
                    blk[i, j] = 0
            if unusable[X]:
                bad.append((Y, X))
                at.append((i, j))
            else:
                good.append((Y, X))
        usable = np.flatnonzero(~unusable)
        hole = int(usable[m % usable.size])
        and_with[Y, :] = NEIGHBOURS[(np.arange(So) + m) % 3]
        and_with[Y, hole] = 0
        holes.append((Y, hole))
    for a in (src, and_with):
        a.setflags(write=False)
    return KeepCase(key, src, THRESHOLD if is_float else None, b, and_with, bad, good, holes, at)


def repeat_first_rows(mask, key):
    """`mask` with every output row replaced by the first row of its workgroup: what a kernel that never advanced would store."""
    rpb = strip_shapes.SHAPES[key].grid[2]
    return mask[np.arange(mask.shape[0]) // rpb * rpb]
