"""The rasters at which the GPU tests run the strip kernels with MORE THAN FOUR LINES PER WORKGROUP (tests/test_gpu_strips.py,
the "dense_blocks" case of tests/test_gpu_streaks.py, the keep masks of tests/keep_cases.py).

`strip_grid` (csrc/xsw_plan.hpp) aims for about 4096 workgroups, so a workgroup gets a second line only once
lines x ceil(columns / 256) exceeds that: below some 4 Mpx per column unit the kernels' four-line unrolled loops never run, only
their one-line tail loop, once.  Each raster here gives every workgroup one or two unrolled groups AND a tail behind them, and a
last workgroup that is shorter than the others and no whole number of groups.

`grid` is what strip_grid answers for the entry: (gx, gy, rows_per_block, lines of the last block).  It is written down, not
computed, because the GPU tests place their special values by it; tests/test_host_plan.py::test_strip_shapes_stay_multi_line asks
the header itself (compiled, with the kernels' own constants read from the sources) and fails when an entry no longer holds."""
from collections import namedtuple

# kernel: whose strip_grid call (its workgroups-per-CU argument differs); col_div: samples per column unit of that call.
# reduce: the kernel's grid is on the raster reduced by reduce x reduce blocks, the remainder trimmed (k_grad_keep: 1 otherwise);
# dtype / inst: the keep entries' input type and the k_grad_keep<T, W, B> instantiation the entry claims to reach
StripShape = namedtuple("StripShape", "kernel lines samples col_div grid reduce dtype inst", defaults=(1, None, None))

SHAPES = {
    "detrend_vec": StripShape("detrend", 2561, 8192, 4, (8, 427, 6, 5)),       # samples % 4 == 0: 16-byte accesses
    "detrend_elem": StripShape("detrend", 2561, 8190, 4, (8, 427, 6, 5)),      # element-wise, a last quad of two samples
    "dsig_flat_vec": StripShape("dsig_flat", 1281, 8192, 2, (16, 214, 6, 3)),  # even samples: pair accesses
    "dsig_flat_elem": StripShape("dsig_flat", 1281, 8191, 2, (16, 214, 6, 3)),  # element-wise, a last pair of one sample
    "streaks": StripShape("streaks", 4097, 2048, 1, (8, 456, 9, 2)),           # two unrolled groups and one more line
    # k_grad_keep: strip_grid(lines // reduce, samples // reduce), one output column per thread.  grad_keep (xsw_gradients.hip)
    # launches the widest W among 16, 8, 4 (> the element size) that divides the block's row bytes and the raster's row bytes and
    # to which the base is aligned, else the element size; B = 2 for float64 at W = 16 and 2 x 2 blocks.  One entry per
    # instantiation.  With reduce <= 2 two column strips (8193 x 258 outputs); the wide blocks take one strip that ends in a
    # partial wave and 20487 output rows, which keeps every input under 70 MB.
    "keep_f64_b2": StripShape("keep", 16387, 516, 1, (2, 1639, 5, 3), 2, "float64", ("double", 16, 2)),   # 16 B block rows, even samples; a trimmed row
    "keep_f64_b4": StripShape("keep", 81951, 54, 1, (1, 3415, 6, 3), 4, "float64", ("double", 16, 0)),    # 32 B block rows, even samples; trimmed rows and columns
    "keep_f64_odd": StripShape("keep", 61463, 65, 1, (1, 3415, 6, 3), 3, "float64", ("double", 8, 0)),    # odd samples: row bytes % 16 == 8; trimmed
    "keep_u8_w16": StripShape("keep", 327797, 144, 1, (1, 3415, 6, 3), 16, "uint8", ("uint8_t", 16, 0)),  # samples % 16 == 0; trimmed rows
    "keep_u8_w8": StripShape("keep", 163899, 160, 1, (1, 3415, 6, 3), 8, "uint8", ("uint8_t", 8, 0)),     # 8 B block rows; trimmed rows
    "keep_u8_w4": StripShape("keep", 81949, 400, 1, (1, 3415, 6, 3), 4, "uint8", ("uint8_t", 4, 0)),      # 4 B block rows; a trimmed row
    "keep_u8_w1": StripShape("keep", 61463, 151, 1, (1, 3415, 6, 3), 3, "uint8", ("uint8_t", 1, 0)),      # 3 B block rows, odd samples; trimmed
}


def shape(key):
    return SHAPES[key].lines, SHAPES[key].samples


def grid_rows(key):
    """The rows of the entry's grid: its lines, or for a keep entry the output rows."""
    return SHAPES[key].lines // SHAPES[key].reduce


def block_lines(key, block):
    """The lines (keep entries: output rows) of workgroup row `block` (negative: from the end), in order."""
    _gx, gy, rpb, _last = SHAPES[key].grid
    b = block % gy
    return list(range(b * rpb, min((b + 1) * rpb, grid_rows(key))))


def probe_lines(key):
    """Where a test puts what it wants every code path to meet: all lines of the second workgroup row (each position u = 0..3 of
    every unrolled group, and the tail lines behind them) and all lines of the last, short one."""
    return block_lines(key, 1) + block_lines(key, -1)
