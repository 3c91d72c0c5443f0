"""The rasters at which the GPU tests run the strip kernels with MORE THAN FOUR LINES PER WORKGROUP (tests/test_gpu_strips.py,
the "dense_blocks" case of tests/test_gpu_streaks.py).

`strip_grid` (csrc/xsw_plan.hpp) aims for about 4096 workgroups, so a workgroup gets a second line only once
lines x ceil(columns / 256) exceeds that: below some 4 Mpx per column unit the kernels' four-line unrolled loops never run, only
their one-line tail loop, once.  Each raster here gives every workgroup one or two unrolled groups AND a tail behind them, and a
last workgroup that is shorter than the others and no whole number of groups.

`grid` is what strip_grid answers for the entry: (gx, gy, rows_per_block, lines of the last block).  It is written down, not
computed, because the GPU tests place their special values by it; tests/test_host_plan.py::test_strip_shapes_stay_multi_line asks
the header itself (compiled, with the kernels' own constants read from the sources) and fails when an entry no longer holds."""
from collections import namedtuple

# kernel: whose strip_grid call (its workgroups-per-CU argument differs); col_div: samples per column unit of that call
StripShape = namedtuple("StripShape", "kernel lines samples col_div grid")

SHAPES = {
    "detrend_vec": StripShape("detrend", 2561, 8192, 4, (8, 427, 6, 5)),       # samples % 4 == 0: 16-byte accesses
    "detrend_elem": StripShape("detrend", 2561, 8190, 4, (8, 427, 6, 5)),      # element-wise, a last quad of two samples
    "dsig_flat_vec": StripShape("dsig_flat", 1281, 8192, 2, (16, 214, 6, 3)),  # even samples: pair accesses
    "dsig_flat_elem": StripShape("dsig_flat", 1281, 8191, 2, (16, 214, 6, 3)),  # element-wise, a last pair of one sample
    "streaks": StripShape("streaks", 4097, 2048, 1, (8, 456, 9, 2)),           # two unrolled groups and one more line
}


def shape(key):
    return SHAPES[key].lines, SHAPES[key].samples


def block_lines(key, block):
    """The lines of workgroup row `block` (negative: from the end), in order."""
    e = SHAPES[key]
    _gx, gy, rpb, _last = e.grid
    b = block % gy
    return list(range(b * rpb, min((b + 1) * rpb, e.lines)))


def probe_lines(key):
    """Where a test puts what it wants every code path to meet: all lines of the second workgroup row (each position u = 0..3 of
    every unrolled group, and the tail lines behind them) and all lines of the last, short one."""
    return block_lines(key, 1) + block_lines(key, -1)
