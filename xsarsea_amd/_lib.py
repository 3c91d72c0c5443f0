"""ctypes binding of libxsw.so (include/xsw.h).  There is no CPU fallback: if the library is missing
or no GPU is present the calls raise."""
import ctypes
import functools
import os
import threading

import numpy as np

from . import _build, _host

XSW_F32, XSW_F64 = 0, 1
MEM_HOST, MEM_DEVICE, MEM_HOST_PINNED, MEM_DEVICE_SIGMA0_HOST = 0, 1, 2, 3
CODE_NAN_RE, CODE_NAN, CODE_PICK_CO, CODE_NO_INDEX = 0xFFFFFFFF, 0xFFFFFFFE, 0x40000000, 0x3FFFFFFF
UNC_NO_SOLUTION, UNC_WSPD_BORDER, UNC_PHI_BORDER, UNC_NOT_CONVEX = 1, 2, 4, 8  # XSW_UNC_*: the bits of an uncertainty flag raster
UNC_NO_CROSSPOL = 16  # XSW_UNC_NO_CROSSPOL (xsw_uncertainty_joint_from_codes): no cross-pol information, the co-pol stencil; not a NaN by itself
SOLVE_NAN, SOLVE_BELOW, SOLVE_ABOVE, SOLVE_TAIL = 1, 2, 4, 8  # XSW_SOLVE_*: the bits of a `retrieve_wspd` flag raster
DIR_NAN, DIR_BELOW, DIR_ABOVE, DIR_MORE = 1, 2, 4, 8  # XSW_DIR_*: the bits of a `retrieve_dir` flag raster
ALGO_AUTO, ALGO_PRUNED, ALGO_EXHAUSTIVE, ALGO_EXACT, ALGO_EXHAUSTIVE_F64 = 0, 1, 2, 3, 4
ALGOS = {"auto": ALGO_AUTO, "pruned": ALGO_PRUNED, "exhaustive": ALGO_EXHAUSTIVE, "exact": ALGO_EXACT,
         "exhaustive_f64": ALGO_EXHAUSTIVE_F64}


def lines_samples(shape):
    """The (lines, samples) view of a raster: samples = the last axis, (1, 1) for a 0-d raster, (0, 0) for an empty one."""
    n = int(np.prod(shape, dtype=np.int64))
    if not n:
        return 0, 0
    return (n // shape[-1], shape[-1]) if len(shape) else (1, 1)


def algo_code(algo):
    """XSW_ALGO_* of an `options.algo` name (a code passes through)."""
    return ALGOS.get(algo, algo)


# get_dsig / get_dsig_wspd names -> XSW_DSIG_* / XSW_DSIG_WSPD_* (include/xsw.h)
DSIG_RULES = {"gmf_s1_v2": 0, "gmf_rs2_v2": 1, "sarwing_lut_cmodms1ahw": 2, "nc_lut_cmodms1ahw": 2}
DSIG_WSPD_RULES = {"dsig_wspd_rs2_v3": 0, "dsig_wspd_s1_ew_rec_v3": 1, "dsig_wspd_rcm_v3": 2}

GMF_IDS = {"gmf_cmod5": 0, "gmf_cmod5n": 1, "gmf_cmod5n_pr_zhangA": 2, "gmf_cmod5n_pr_mouche1": 3, "gmf_cmodifr2": 4,
           "gmf_rs2_v2": 5, "gmf_s1_v2": 6, "gmf_rcm_noaa": 7, "gmf_s1_v3_ew_rec": 8, "gmf_rs2_v3": 9, "gmf_rcm_v3": 10,
           "gmf_rcm_v4": 11, "gmf_rs2_v4": 12}

EXPORTS = (
    "xsw_version", "xsw_device_count", "xsw_ctx_create", "xsw_ctx_destroy", "xsw_last_error", "xsw_set_stream", "xsw_use_own_stream",
    "xsw_synchronize", "xsw_lut_upload", "xsw_invert", "xsw_stats_enable", "xsw_stats_read", "xsw_stats_read_chain", "xsw_detrend", "xsw_lut_interp", "xsw_gmf_eval",
    "xsw_nesz_flatten", "xsw_lut_build", "xsw_lut_read", "xsw_lut_table_read", "xsw_timing_enable", "xsw_timing_read", "xsw_expand_codes", "xsw_expand_codes_on_stream",
    "xsw_host_alloc", "xsw_host_free", "xsw_set_host_threads", "xsw_grad_area", "xsw_grad_r2", "xsw_grad_local", "xsw_grad_hist",
    "xsw_grad_r2_sqrt", "xsw_grad_local_sqrt", "xsw_grad_smooth", "xsw_grad_mean", "xsw_grad_filter",
    "xsw_grad_hist_masked", "xsw_grad_keep_f64", "xsw_grad_keep_u8",
    "xsw_streaks_peak", "xsw_streaks_resolve", "xsw_streaks_ancillary", "xsw_ancillary_model",
    "xsw_wind_cells", "xsw_raster_cells", "xsw_wind_grid", "xsw_wind_polar", "xsw_wind_centre", "xsw_land_mask", "xsw_land_chunk_edges", "xsw_calibrate",
    "xsw_cross_from_codes", "xsw_cost_from_codes", "xsw_cost_cr_from_codes",
    "xsw_uncertainty_from_codes", "xsw_uncertainty_cr_from_codes", "xsw_joint_from_codes",
    "xsw_uncertainty_joint_from_codes",
    "xsw_lut_eval", "xsw_lut_eval_cr",
    "xsw_wspd_solve", "xsw_wspd_solve_cr", "xsw_dir_solve",
    "xsw_dsig", "xsw_dsig_flat", "xsw_dsig_wspd",
)


# The raster entries behind xsarsea_amd.gradients, xsarsea_amd.streaks, xsarsea_amd.ancillary, xsarsea_amd.cells, xsarsea_amd.grid, xsarsea_amd.polar, xsarsea_amd.centre and xsarsea_amd.landmask: their C signature after the context, one letter per
# argument (l int64, i int32, d double, p pointer: an int address, device or host per `mem`, or None).  `load` sets the argtypes
# from it and every row becomes a Context method, e.g. `grad_area_raw(lines, samples, factor, dtype, mem, in_ptr, out_ptr)`.
RASTER_ENTRIES = {
    # (lines, samples, factor, dtype, mem, in, out): f x f box mean, output of the input's dtype
    "xsw_grad_area": "lliiipp",
    # (lines, samples, dtype, mem, take_sqrt, in, out): R2 (or sqrt(R2) with take_sqrt) -> float64 (lines // 2, samples // 2)
    "xsw_grad_r2": "lliiipp",
    # (lines, samples, mem, ampl, g2, g3, c): float64 ampl -> G2 (complex128), G3, c on the (lines // 2, samples // 2) grid
    "xsw_grad_local": "llipppp",
    # (lines, samples, mem, g2, c, window_lines, window_samples, n_rows, rows, n_cols, cols, n_angles, angle_start, angle_step,
    # normalise, weight, ratio): per-window bin sums (divided by the window's pixel count with `normalise`) and used ratios
    # (rows / cols: int32 window-centre indices)
    "xsw_grad_hist": "llippiiipipiddipp",
    # (lines, samples, dtype, mem, in, out): R2(sqrt(sigma0)) -> float64 (lines // 2, samples // 2)
    "xsw_grad_r2_sqrt": "lliipp",
    # (lines, samples, dtype, mem, in, g2, g3, c): local_gradients(sqrt(sigma0)); g2 None skips G2
    "xsw_grad_local_sqrt": "lliipppp",
    # (lines, samples, mem, coarsen, in, out): 3x3 B2 "symm" smoothing of `in` or, with coarsen, of its NaN-skipping 2 x 2 mean
    "xsw_grad_smooth": "lliipp",
    # (lines, samples, mem, in, out): Mean (B4 then B42, "symm") of a float64 raster
    "xsw_grad_mean": "llipp",
    # (lines, samples, mem, r2, g3, c, smooth4, out): (f1, f2, f3, f4, F) as [5, lines, samples] on the half-resolution grid
    "xsw_grad_filter": "llippppp",
    # xsw_grad_hist with a uint8 keep mask on the g2 grid after c (0 = the pixel behaves as a NaN g2)
    "xsw_grad_hist_masked": "llipppiiipipiddipp",
    # (lines, samples, mem, src, threshold, block, and_with, out): float64 src, usable iff >= threshold, reduced by block x
    # block blocks to a uint8 keep mask; and_with (None: absent) is AND-ed in
    "xsw_grad_keep_f64": "llipdipp",
    # (lines, samples, mem, src, block, and_with, out): the same for a uint8 src, usable iff non-zero
    "xsw_grad_keep_u8": "llipipp",
    # (n_lead, n_windows, n_angles, mem, smooth, weight, ratio, index, weight_out, ratio_out): mean over the leading axes,
    # circular smoothing, peak bin of every window
    "xsw_streaks_peak": "lliiippppp",
    # (n_windows, mem, dirs, weight, ratio, anc, min_weight, min_used_ratio, out): the windows' unit vectors with the 180 degree
    # ambiguity removed (NaN thresholds: off)
    "xsw_streaks_resolve": "lippppddp",
    # (lines, samples, mem, anc, n_rows, n_cols, dirs, line_first, line_t, sample_first, sample_t, out): the complex128 a-priori
    # raster from the resolved window directions
    "xsw_streaks_ancillary": "llipiipppppp",
    # (lines, samples, mem, dtype, u, v, n_lat, n_lon, lon0, dlon, periodic, lat0, dlat, n_tie_lines, n_tie_samples, tie_lon, tie_lat,
    # tie_cos, tie_sin, line_first, line_t, sample_first, sample_t, out): the complex128 a-priori raster from the model wind on its
    # uniform grid and the scene's tie points
    "xsw_ancillary_model": "lliippiiddiddiippppppppp",
    # (lines, samples, mem, src_kind, src, keep, cell_lines, cell_samples, n_tie_lines, n_tie_samples, tie_lon, tie_lat, tie_cos, tie_sin,
    # line_first, line_t, sample_first, sample_t, count, wind, wspd, wspd_std, steadiness, longitude, latitude, u, v): per cell of the
    # product grid, from a complex wind raster or co-pol codes (CELLS_*); keep, the tie points and every output may be None
    "xsw_wind_cells": "lliippiiiipppppppp" + "p" * 9,
    # (lines, samples, mem, dtype, x, keep, cell_lines, cell_samples, count, mean, std): the same for a float32 / float64 raster
    "xsw_raster_cells": "lliippiippp",
    # (lines, samples, mem, src_kind, src, keep, n_tie_lines, n_tie_samples, tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t,
    # sample_first, sample_t, lon0, dlon, n_lon, periodic, lat0, dlat, n_lat, sums): every valid pixel of a complex wind raster or of
    # co-pol codes (CELLS_*) adds its fixed-point terms to its bin of the longitude / latitude grid: int64 sums [5, n_lat, n_lon],
    # added to, never zeroed; keep may be None, the tie points and the per-pixel brackets are required
    "xsw_wind_grid": "lliippiipppppppp" + "ddiiddi" + "p",
    # (lines, samples, mem, src_kind, src, keep, n_tie_lines, n_tie_samples, tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t,
    # sample_first, sample_t, lon_c, lat_c, cos_lat_c, sin_lat_c, dr_km, n_r, n_theta, sector_sin, sector_cos, sums): the same pixels
    # binned in n_r rings of dr_km and n_theta sectors around the centre: int64 sums [6, n_r, n_theta], the first five planes added
    # to, the sixth raised to the maximum, never zeroed; sector_sin / sector_cos: the borders of one quadrant's sectors
    "xsw_wind_polar": "lliippiipppppppp" + "dddddii" + "pp" + "p",
    # (lines, samples, mem, src_kind, src, keep, n_tie_lines, n_tie_samples, tie_lon, tie_lat, tie_cos, tie_sin, line_first, line_t,
    # sample_first, sample_t, lon_g, lat_g, cos_lat_g, sin_lat_g, step_km, n_c, r_in_km, r_out_km, sums): the same pixels added to
    # every node of the n_c x n_c lattice of candidate centres around the first guess whose annulus [r_in_km, r_out_km) they lie
    # in: int64 sums [5, n_c, n_c], added to, never zeroed
    "xsw_wind_centre": "lliippiipppppppp" + "dddddidd" + "p",
    # (lines, samples, mem, n_tie_lines, n_tie_samples, tie_lon, tie_lat, line_first, line_t, sample_first, sample_t, n_edges, edges,
    # n_bands, band_start, n_list, band_edges, lat0, h, and_with, invert, out): the uint8 sea / land keep mask (1 = water) from the
    # float64 edges [n_edges, 4] = x1, y1, x2, y2 by the even-odd rule; n_bands = 0 with band_start / band_edges None: every pixel
    # against every edge; edges (with n_edges = 0) and and_with may be None
    "xsw_land_mask": "lliiippppppipipipddpip",
}
assert list(RASTER_ENTRIES) == [n for n in EXPORTS if n.startswith(("xsw_grad_", "xsw_streaks_", "xsw_ancillary_")) or n.endswith(("_cells", "_grid", "_polar", "_centre", "_mask"))]
CELLS_C128, CELLS_C64, CELLS_CODES = 0, 1, 2  # XSW_CELLS_* (include/xsw.h): the source kinds of xsw_wind_cells
DN_U16, DN_F32 = 0, 1  # XSW_DN_* (include/xsw.h): the digital numbers of xsw_calibrate
# letter -> (ctypes type, conversion the wrapper applies: ctypes alone refuses numpy scalars)
_SIG = {"l": (ctypes.c_int64, int), "i": (ctypes.c_int32, int), "d": (ctypes.c_double, float), "p": (ctypes.c_void_p, lambda a: a)}


class XswError(RuntimeError):
    pass


TAB_ABSENT = 1  # XSW_TAB_ABSENT: what xsw_lut_table_read answers for an optional table the install did not build


def co_table_layouts(n_inc, n_w, n_phi):
    """name -> (XSW_TAB_* id, dtype, shape) of every table `xsw_lut_table_read` copies, for a co-pol LUT of this shape: the
    element counts of CoGeometry (csrc/xsw_lutplan.hpp).  `co`, `co32` and `coT` are flat (their slack follows the body)."""
    def up(a, b):
        return -(-a // b)

    ppad, wpad = up(n_phi, 4) * 4, up(n_w, 4) * 4
    nbr, nbc, nbc4 = up(n_w, 4), up(n_phi, 16), up(n_phi, 4)
    ncr, ncc = up(nbr, 8), up(nbc, 2)
    nbands = up(nbr, max(1, 64 // nbc))
    n_pad = (n_inc * n_w + 260) * ppad
    return {
        "co": (0, np.float64, (n_pad,)), "co32": (1, np.float32, (n_pad,)), "coT": (2, np.float64, (n_inc * n_phi * wpad + 512,)),
        "mono_rows": (3, np.int32, (n_inc,)), "tail_min": (4, np.float64, (n_inc, 8, ppad)), "inv_grid": (5, np.float64, (n_inc, 3)),
        "inv_rows": (6, np.uint16, (n_inc, 2048, ppad)), "blk": (7, np.float32, (n_inc, nbr, nbc, 2)),
        "blk4": (8, np.float32, (n_inc, nbr, nbc4, 2)), "cellmm": (9, np.float32, (n_inc, ncr, ncc, 2)),
        "bandmm": (10, np.float32, (n_inc, nbands, 2)), "scalars": (11, np.float64, (3,)),
    }


class LutStruct(ctypes.Structure):
    _fields_ = [("db", ctypes.c_void_p), ("inc", ctypes.c_void_p), ("wspd", ctypes.c_void_p),
                ("phi", ctypes.c_void_p), ("cos_phi", ctypes.c_void_p), ("sin_phi", ctypes.c_void_p),
                ("out_dir", ctypes.c_void_p), ("abs_co", ctypes.c_void_p), ("dual_dir", ctypes.c_void_p),
                ("n_inc", ctypes.c_int32), ("n_wspd", ctypes.c_int32), ("n_phi", ctypes.c_int32)]


class InvertArgs(ctypes.Structure):
    _fields_ = [("lines", ctypes.c_int64), ("samples", ctypes.c_int64), ("dtype", ctypes.c_int32),
                ("out_dtype", ctypes.c_int32), ("mem", ctypes.c_int32), ("sigma0_is_db", ctypes.c_int32),
                ("algo", ctypes.c_int32), ("dual_select", ctypes.c_int32),
                ("inc", ctypes.c_void_p), ("sigma0_co", ctypes.c_void_p), ("sigma0_cr", ctypes.c_void_p),
                ("dsig_cr", ctypes.c_void_p), ("anc", ctypes.c_void_p),
                ("dsig_co", ctypes.c_double), ("dsig_cr_scalar", ctypes.c_double),
                ("out_co", ctypes.c_void_p), ("out_cr", ctypes.c_void_p), ("out_idx", ctypes.c_void_p),
                ("out_code_co", ctypes.c_void_p), ("out_code_cr", ctypes.c_void_p),
                ("stage", ctypes.c_void_p), ("stage_user", ctypes.c_void_p)]


class Table(ctypes.Structure):
    """xsw_table (include/xsw.h): an annotation grid of xsw_calibrate with the brackets of the raster's lines and samples."""
    _fields_ = [("n_lines", ctypes.c_int32), ("n_samples", ctypes.c_int32), ("values", ctypes.c_void_p), ("line_first", ctypes.c_void_p),
                ("line_t", ctypes.c_void_p), ("sample_first", ctypes.c_void_p), ("sample_t", ctypes.c_void_p)]


#: int stage(void *user, int32 which, int64 px0, int64 npx, void *dst)  (xsw_invert_args.stage)
STAGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p)
STAGE_INC, STAGE_SIGMA0_CO, STAGE_SIGMA0_CR, STAGE_DSIG_CR, STAGE_ANC = range(5)


ABI_VERSION = 4  # include/xsw.h: XSW_VERSION


class Stats(ctypes.Structure):
    _fields_ = [("pixels_co", ctypes.c_uint64), ("cand_co", ctypes.c_uint64), ("pixels_exact", ctypes.c_uint64),
                ("pixels_cr", ctypes.c_uint64)]


class ChainStats(ctypes.Structure):
    _fields_ = [("cand_band2", ctypes.c_uint64), ("cand_blocks", ctypes.c_uint64), ("cand_list", ctypes.c_uint64), ("pixels_refined", ctypes.c_uint64)]


class Timing(ctypes.Structure):
    _fields_ = [("launches", ctypes.c_int64), ("first_kernel_ms", ctypes.c_double), ("second_kernel_ms", ctypes.c_double),
                ("last_list_pixels", ctypes.c_int64), ("band2_kernel_ms", ctypes.c_double), ("last_band2_pixels", ctypes.c_int64),
                ("blocks_kernel_ms", ctypes.c_double), ("last_blocks_pixels", ctypes.c_int64)]


_cdll = None


def library_path():
    return _build.LIB


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same soname as the system
    one); if libxsw.so pulled in the system runtime first, a later `import torch` would find "no ROCm-capable
    device".  So when torch is installed but not imported yet, its bundled runtime is loaded first (libxsw.so then
    binds to it); when torch is already imported, or absent, nothing needs doing."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libxsw.so (raises if it has not been built: run `python -m xsarsea_amd._build`)."""
    global _cdll
    if _cdll is None:
        if not os.path.exists(_build.LIB):
            raise XswError(f"{_build.LIB} is missing: build it with `python -m xsarsea_amd._build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _preload_hip_runtime()
        lib = ctypes.CDLL(_build.LIB)
        lib.xsw_last_error.restype = ctypes.c_char_p
        lib.xsw_last_error.argtypes = [ctypes.c_void_p]
        lib.xsw_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        lib.xsw_ctx_destroy.argtypes = [ctypes.c_void_p]
        lib.xsw_set_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.xsw_use_own_stream.argtypes = [ctypes.c_void_p]
        lib.xsw_synchronize.argtypes = [ctypes.c_void_p]
        lib.xsw_lut_upload.argtypes = [ctypes.c_void_p, ctypes.POINTER(LutStruct), ctypes.POINTER(LutStruct)]
        lib.xsw_invert.argtypes = [ctypes.c_void_p, ctypes.POINTER(InvertArgs)]
        lib.xsw_stats_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.xsw_stats_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats)]
        lib.xsw_stats_read_chain.argtypes = [ctypes.c_void_p, ctypes.POINTER(ChainStats)]
        lib.xsw_detrend.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.xsw_lut_interp.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 4 + [ctypes.c_int32] * 3 + \
            [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 3 + [ctypes.c_void_p]
        lib.xsw_gmf_eval.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 4
        lib.xsw_nesz_flatten.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 3
        lib.xsw_lut_build.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(LutStruct)]
        lib.xsw_lut_read.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        lib.xsw_lut_table_read.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t]
        lib.xsw_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.xsw_timing_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(Timing)]
        lib.xsw_expand_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 4
        lib.xsw_expand_codes_on_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 4
        lib.xsw_cross_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 5 + [ctypes.c_void_p] * 4 + \
            [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        lib.xsw_cost_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 4 + \
            [ctypes.c_double] + [ctypes.c_void_p] * 4
        lib.xsw_cost_cr_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 5 + \
            [ctypes.c_double] + [ctypes.c_void_p] * 4
        lib.xsw_uncertainty_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 4 + \
            [ctypes.c_double] + [ctypes.c_void_p] * 4
        lib.xsw_uncertainty_cr_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 5 + \
            [ctypes.c_double] + [ctypes.c_void_p] * 2
        lib.xsw_joint_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 4 + \
            [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double] + [ctypes.c_void_p] * 5
        lib.xsw_uncertainty_joint_from_codes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 4 + \
            [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double] + [ctypes.c_void_p] * 7
        lib.xsw_lut_eval.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 6
        lib.xsw_lut_eval_cr.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 4
        lib.xsw_wspd_solve.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 6
        lib.xsw_wspd_solve_cr.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 5
        lib.xsw_dir_solve.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 13
        lib.xsw_dsig.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 4
        lib.xsw_dsig_flat.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 4
        lib.xsw_dsig_wspd.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 3
        lib.xsw_calibrate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] + \
            [ctypes.POINTER(Table)] * 4 + [ctypes.c_int32, ctypes.c_double] + [ctypes.c_void_p] * 4
        lib.xsw_host_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        lib.xsw_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.xsw_set_host_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
        for name, sig in RASTER_ENTRIES.items():
            getattr(lib, name).argtypes = [ctypes.c_void_p] + [_SIG[k][0] for k in sig]
        if lib.xsw_version() != ABI_VERSION:
            raise XswError(f"{_build.LIB} is version {lib.xsw_version()}, this package binds version {ABI_VERSION}: rebuild it")
        _cdll = lib
    return _cdll


def device_count():
    return load().xsw_device_count()


def land_chunk_edges():
    """xsw_land_chunk_edges: the edges one staging chunk of the land-mask kernels holds."""
    return int(load().xsw_land_chunk_edges())


def device_count_safe():
    """0 when the library is not built (host-only uses such as LUT preparation in a CPU-only session)."""
    try:
        return device_count()
    except (XswError, OSError):
        return 0


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    return ctypes.c_void_p(a.ctypes.data)


def _locked(method):
    """A libxsw context is not thread-safe (include/xsw.h); the Python layer serialises the calls on one context, so
    that threaded callers (dask's threaded scheduler runs the reference's function from several threads) stay correct.
    The lock is re-entrant and is also taken by `windspeed._engine` around "make sure the LUTs are up, then invert"."""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with self.lock:
            return method(self, *args, **kwargs)
    return wrapper


class Context:
    """One device, one stream (include/xsw.h: xsw_ctx)."""

    def __init__(self, device=0):
        self._lib = load()
        h = ctypes.c_void_p()
        rc = self._lib.xsw_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise XswError(f"xsw_ctx_create failed ({rc}): {self._lib.xsw_last_error(None).decode()}")
        self._h = h
        self.device = int(device)
        self.lut_key = (None, None)
        self.lock = threading.RLock()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.xsw_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise XswError(f"{what} failed ({rc}): {self._lib.xsw_last_error(self._h).decode()}")

    @_locked
    def set_stream(self, stream_handle):
        """Launch on this hipStream_t handle (int; 0 = the device's default stream)."""
        self._check(self._lib.xsw_set_stream(self._h, ctypes.c_void_p(stream_handle or 0)), "xsw_set_stream")

    @_locked
    def use_own_stream(self):
        self._check(self._lib.xsw_use_own_stream(self._h), "xsw_use_own_stream")

    @_locked
    def synchronize(self):
        self._check(self._lib.xsw_synchronize(self._h), "xsw_synchronize")

    @staticmethod
    def _lut_struct(db, inc, wspd, phi=None, cos_phi=None, sin_phi=None, out_dir=None, abs_co=None, dual_dir=None):
        keep = [None if db is None else _f64(db), _f64(inc), _f64(wspd)] + [None if v is None else _f64(v) for v in
                                                                            (phi, cos_phi, sin_phi, out_dir, abs_co, dual_dir)]
        n_phi = 0 if phi is None else len(keep[3])
        n_w = len(keep[2])
        expect = (len(keep[1]), n_w) + ((n_phi,) if phi is not None else ())
        if keep[0] is not None and keep[0].shape != expect:
            raise ValueError(f"LUT shape {keep[0].shape} does not match axes {expect}")
        for a, shp, nm in ((keep[4], (n_phi,), "cos_phi"), (keep[5], (n_phi,), "sin_phi"),
                           (keep[6], (2, n_phi, 2), "out_dir"), (keep[7], (n_w, n_phi), "abs_co"),
                           (keep[8], (2, n_w, n_phi, 2), "dual_dir")):
            if a is not None and a.shape != shp:
                raise ValueError(f"{nm} has shape {a.shape}, expected {shp}")
        s = LutStruct(*[_ptr(k) for k in keep], len(keep[1]), n_w, n_phi)
        return s, keep

    @_locked
    def upload_luts(self, co=None, cr=None):
        """co = dict(db[inc,wspd,phi], inc, wspd, phi[, cos_phi, sin_phi]); cr = dict(db[inc,wspd], inc, wspd)."""
        sco = scr = None
        keep = []
        if co is not None:
            sco, k = self._lut_struct(**co)
            keep.append(k)
        if cr is not None:
            scr, k = self._lut_struct(**cr)
            keep.append(k)
        self._check(self._lib.xsw_lut_upload(self._h, ctypes.byref(sco) if sco else None,
                                             ctypes.byref(scr) if scr else None), "xsw_lut_upload")

    @_locked
    def build_lut(self, gmf_id, raw_axes, target):
        """xsw_lut_build: raw_axes = (inc, wspd, phi or None) of the model's own grid; target = dict(inc, wspd[, phi, cos_phi,
        sin_phi, out_dir, abs_co, dual_dir]) of the grid to search on.  The table is built and kept on the device."""
        inc_r, wspd_r = _f64(raw_axes[0]), _f64(raw_axes[1])
        phi_r = None if raw_axes[2] is None else _f64(raw_axes[2])
        st, keep = self._lut_struct(None, **target)
        self._check(self._lib.xsw_lut_build(self._h, int(gmf_id), _ptr(inc_r), len(inc_r), _ptr(wspd_r), len(wspd_r), _ptr(phi_r),
                                            0 if phi_r is None else len(phi_r), ctypes.byref(st)), "xsw_lut_build")
        del keep

    @_locked
    def read_lut(self, shape, cross=False):
        """xsw_lut_read: the context's current dB table as a host array of `shape` (the caller knows the axes)."""
        out = np.empty(shape, dtype=np.float64)
        self._check(self._lib.xsw_lut_read(self._h, int(bool(cross)), _ptr(out)), "xsw_lut_read")
        return out

    @_locked
    def read_lut_table(self, name, lut_shape):
        """xsw_lut_table_read (a diagnostic: the tests' view of what a co-pol install derived): table `name` of
        `co_table_layouts(*lut_shape)` as a host array, or None when the install did not build it."""
        which, dtype, shape = co_table_layouts(*lut_shape)[name]
        out = np.empty(shape, dtype=dtype)
        rc = self._lib.xsw_lut_table_read(self._h, which, _ptr(out), out.nbytes)
        if rc == TAB_ABSENT:
            return None
        self._check(rc, "xsw_lut_table_read")
        return out

    @_locked
    def lut_interp(self, raw, inc_raw, wspd_raw, phi_raw, inc, wspd, phi):
        """xsw_lut_interp: (incidence, wspd[, phi]) table -> finer axes, bit-identical to three interp1d passes."""
        raw, inc_raw, wspd_raw, inc, wspd = map(_f64, (raw, inc_raw, wspd_raw, inc, wspd))
        has_phi = phi_raw is not None
        phi_raw = _f64(phi_raw) if has_phi else None
        phi = _f64(phi) if has_phi else None
        out = np.empty((len(inc), len(wspd)) + ((len(phi),) if has_phi else ()), dtype=np.float64)
        self._check(self._lib.xsw_lut_interp(
            self._h, _ptr(raw), _ptr(inc_raw), _ptr(wspd_raw), _ptr(phi_raw), len(inc_raw), len(wspd_raw),
            len(phi_raw) if has_phi else 0, _ptr(inc), _ptr(wspd), _ptr(phi), len(inc), len(wspd),
            len(phi) if has_phi else 0, _ptr(out)), "xsw_lut_interp")
        return out

    @_locked
    def gmf_eval(self, gmf_id, inc, wspd, phi=None):
        """xsw_gmf_eval on host float64 arrays of one common shape."""
        inc = _f64(inc)
        wspd = _f64(wspd)
        phi = None if phi is None else _f64(phi)
        if wspd.shape != inc.shape or (phi is not None and phi.shape != inc.shape):
            raise ValueError("gmf_eval wants already-broadcast arrays of one shape")
        out = np.empty(inc.shape, dtype=np.float64)
        self._check(self._lib.xsw_gmf_eval(self._h, int(gmf_id), inc.size, MEM_HOST, _ptr(inc), _ptr(wspd), _ptr(phi),
                                           _ptr(out)), "xsw_gmf_eval")
        return out

    @_locked
    def gmf_eval_raw(self, gmf_id, n, mem, inc_ptr, wspd_ptr, phi_ptr, out_ptr):
        """Thin call of xsw_gmf_eval (pointers are ints or None: float64 arrays of n already-broadcast elements; device
        pointers with MEM_DEVICE: asynchronous on the context's stream)."""
        self._check(self._lib.xsw_gmf_eval(self._h, int(gmf_id), int(n), mem, _ptr(inc_ptr), _ptr(wspd_ptr), _ptr(phi_ptr), _ptr(out_ptr)),
                    "xsw_gmf_eval")

    @_locked
    def timing_enable(self, on=True):
        self._check(self._lib.xsw_timing_enable(self._h, int(bool(on))), "xsw_timing_enable")

    @_locked
    def timing(self):
        """xsw_timing_read: dict(launches, first_kernel_ms, second_kernel_ms) summed since the last read."""
        t = Timing()
        self._check(self._lib.xsw_timing_read(self._h, ctypes.byref(t)), "xsw_timing_read")
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    @_locked
    def stats_enable(self, on=True):
        """on = True: the statistics instantiation (every window swept in k_invert_band, every candidate counted); on = 2: the
        production chain with per-kernel counters (`stats_chain`)."""
        self._check(self._lib.xsw_stats_enable(self._h, 2 if on == 2 else int(bool(on))), "xsw_stats_enable")

    @_locked
    def stats_chain(self):
        s = ChainStats()
        self._check(self._lib.xsw_stats_read_chain(self._h, ctypes.byref(s)), "xsw_stats_read_chain")
        return {k: int(getattr(s, k)) for k, _ in ChainStats._fields_}

    @_locked
    def stats(self):
        s = Stats()
        self._check(self._lib.xsw_stats_read(self._h, ctypes.byref(s)), "xsw_stats_read")
        return {k: int(getattr(s, k)) for k, _ in Stats._fields_}

    @_locked
    def invert_raw(self, lines, samples, dtype, out_dtype, mem, inc, sigma0_co, sigma0_cr, dsig_cr, anc, out_co,
                   out_cr, out_idx=None, dsig_co=0.1, dsig_cr_scalar=0.1, sigma0_is_db=False, algo=ALGO_AUTO,
                   dual_select=False, out_code_co=None, out_code_cr=None, stage=None):
        """Thin call of xsw_invert; pointer arguments are ints (device or host addresses) or None.
        stage: python callable (which, px0, npx, dst_address) -> 1 filled / 0 default copy (xsw_invert_args.stage); an
        exception inside it aborts the call and is re-raised here."""
        cb, failure = None, []
        if stage is not None:
            def _cb(_user, which, px0, npx, dst):
                try:
                    return 1 if stage(which, px0, npx, dst) else 0
                except BaseException as exc:  # nothing propagates through the C frames
                    failure.append(exc)
                    return -1
            cb = STAGE_FN(_cb)
        a = InvertArgs(int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)), int(algo),
                       int(bool(dual_select)), inc, sigma0_co, sigma0_cr, dsig_cr, anc, float(dsig_co),
                       float(dsig_cr_scalar), out_co, out_cr, out_idx, out_code_co, out_code_cr,
                       ctypes.cast(cb, ctypes.c_void_p) if cb is not None else None, None)
        rc = self._lib.xsw_invert(self._h, ctypes.byref(a))
        if failure:
            raise failure[0]
        self._check(rc, "xsw_invert")

    @_locked
    def expand_codes_raw(self, n, mem, out_dtype, code_co, code_cr, out_co, out_cr):
        """Thin call of xsw_expand_codes (pointers are ints or None): grid codes -> the complex winds xsw_invert stores."""
        self._check(self._lib.xsw_expand_codes(self._h, int(n), mem, out_dtype, code_co, code_cr, out_co, out_cr), "xsw_expand_codes")

    @_locked
    def cross_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_cr, dsig_cr, out_code_cr, out_cr,
                             dsig_cr_scalar=0.1, sigma0_is_db=False, dual_select=False):
        """Thin call of xsw_cross_from_codes (pointers are ints or None): the cross-pol step of a dual-pol inversion from the
        co-pol grid codes `code_co` (None: cross-pol only) -> the cross-pol codes and / or winds the fused xsw_invert stores."""
        self._check(self._lib.xsw_cross_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)),
                                                   int(bool(dual_select)), inc, code_co, sigma0_cr, dsig_cr, float(dsig_cr_scalar),
                                                   out_code_cr, out_cr), "xsw_cross_from_codes")

    @_locked
    def cost_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_co, anc, out_J, out_Jsig=None, out_Jwind=None,
                            out_residual=None, dsig_co=0.1, sigma0_is_db=False):
        """Thin call of xsw_cost_from_codes (pointers are ints or None): J_co = Jwind + Jsig at the grid point of every co-pol code,
        its two terms and lut_db - sigma0_db, each into a real raster of `out_dtype` (None: not computed)."""
        self._check(self._lib.xsw_cost_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)), inc, code_co,
                                                  sigma0_co, anc, float(dsig_co), out_J, out_Jsig, out_Jwind, out_residual), "xsw_cost_from_codes")

    @_locked
    def cost_cr_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, code_cr, sigma0_cr, dsig_cr, out_J, out_Jsig=None,
                               out_Jwind=None, out_residual=None, dsig_cr_scalar=0.1, sigma0_is_db=False):
        """Thin call of xsw_cost_cr_from_codes: the same for the cross-pol codes `code_cr` (code_co None: cross-pol only; dsig_cr
        None: the scalar broadcast)."""
        self._check(self._lib.xsw_cost_cr_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)), inc, code_co,
                                                     code_cr, sigma0_cr, dsig_cr, float(dsig_cr_scalar), out_J, out_Jsig, out_Jwind, out_residual),
                    "xsw_cost_cr_from_codes")

    @_locked
    def joint_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_co, anc, sigma0_cr, dsig_cr, out_code, out_J=None,
                             out_Jwind=None, out_Jsig_co=None, out_Jsig_cr=None, dsig_co=0.1, dsig_cr_scalar=0.1, sigma0_is_db=False):
        """Thin call of xsw_joint_from_codes (pointers are ints or None): the grid point of the co-pol LUT that minimises
        J = Jwind_co + Jsig_co + Jsig_cr, as uint32 co-pol codes, and J with its three terms there, each into a real raster of
        `out_dtype` (None: not computed); dsig_cr None: the scalar broadcast."""
        self._check(self._lib.xsw_joint_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)), inc, code_co,
                                                   sigma0_co, anc, float(dsig_co), sigma0_cr, dsig_cr, float(dsig_cr_scalar), out_code, out_J,
                                                   out_Jwind, out_Jsig_co, out_Jsig_cr), "xsw_joint_from_codes")

    @_locked
    def uncertainty_joint_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code, sigma0_co, anc, sigma0_cr, dsig_cr, out_wspd_std,
                                         out_dir_std=None, out_corr=None, out_u_std=None, out_v_std=None, out_corr_uv=None, out_flag=None,
                                         dsig_co=0.1, dsig_cr_scalar=0.1, sigma0_is_db=False):
        """Thin call of xsw_uncertainty_joint_from_codes (pointers are ints or None): the error bars of the joint dual-pol solution
        from the curvature of J = Jwind_co + Jsig_co + Jsig_cr around the grid point of every code -- wspd_std (m/s), dir_std
        (degrees), their correlation, and the same covariance in the components of the complex wind (u_std, v_std in m/s,
        corr_uv) -- each into a real raster of `out_dtype`, and the uint8 UNC_* flags (None: not computed); dsig_cr None: the
        scalar broadcast."""
        self._check(self._lib.xsw_uncertainty_joint_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)),
                                                               inc, code, sigma0_co, anc, float(dsig_co), sigma0_cr, dsig_cr,
                                                               float(dsig_cr_scalar), out_wspd_std, out_dir_std, out_corr, out_u_std,
                                                               out_v_std, out_corr_uv, out_flag), "xsw_uncertainty_joint_from_codes")

    @_locked
    def uncertainty_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_co, anc, out_wspd_std, out_dir_std=None,
                                   out_corr=None, out_flag=None, dsig_co=0.1, sigma0_is_db=False):
        """Thin call of xsw_uncertainty_from_codes (pointers are ints or None): the standard deviations of wind speed (m/s) and
        direction (degrees) and their correlation from the curvature of J_co around the grid point of every co-pol code, each into
        a real raster of `out_dtype`, and the uint8 UNC_* flags (None: not computed)."""
        self._check(self._lib.xsw_uncertainty_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)), inc,
                                                         code_co, sigma0_co, anc, float(dsig_co), out_wspd_std, out_dir_std, out_corr, out_flag),
                    "xsw_uncertainty_from_codes")

    @_locked
    def uncertainty_cr_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, code_cr, sigma0_cr, dsig_cr, out_wspd_std,
                                      out_flag=None, dsig_cr_scalar=0.1, sigma0_is_db=False):
        """Thin call of xsw_uncertainty_cr_from_codes: the 1-D analogue for the cross-pol codes `code_cr` (code_co None: cross-pol
        only; dsig_cr None: the scalar broadcast)."""
        self._check(self._lib.xsw_uncertainty_cr_from_codes(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(sigma0_is_db)), inc,
                                                            code_co, code_cr, sigma0_cr, dsig_cr, float(dsig_cr_scalar), out_wspd_std, out_flag),
                    "xsw_uncertainty_cr_from_codes")

    @_locked
    def lut_eval_raw(self, lines, samples, dtype, out_dtype, mem, inc, wspd, phi, out_db, out_dwspd=None, out_dphi=None, fold_phi=True):
        """Thin call of xsw_lut_eval (pointers are ints or None): sigma0 in dB that the context's co-pol table predicts for the wind
        (wspd, phi) at incidence inc, and the derivatives of that interpolant in dB per m/s and dB per degree, each into a real
        raster of `out_dtype` (None: not computed)."""
        self._check(self._lib.xsw_lut_eval(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(fold_phi)), inc, wspd, phi,
                                           out_db, out_dwspd, out_dphi), "xsw_lut_eval")

    @_locked
    def lut_eval_cr_raw(self, lines, samples, dtype, out_dtype, mem, inc, wspd, out_db, out_dwspd=None):
        """Thin call of xsw_lut_eval_cr: the same on the cross-pol table, which has no direction."""
        self._check(self._lib.xsw_lut_eval_cr(self._h, int(lines), int(samples), dtype, out_dtype, mem, inc, wspd, out_db, out_dwspd),
                    "xsw_lut_eval_cr")

    @_locked
    def wspd_solve_raw(self, lines, samples, dtype, out_dtype, mem, inc, sigma0_db, phi, out_wspd, out_sens=None, out_flag=None, fold_phi=True):
        """Thin call of xsw_wspd_solve (pointers are ints or None): the lowest wind speed at which the context's co-pol table gives
        sigma0_db (dB) at incidence inc and direction phi, its sensitivity in m/s per dB, each into a real raster of `out_dtype`,
        and the uint8 SOLVE_* flags (None: not computed)."""
        self._check(self._lib.xsw_wspd_solve(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(fold_phi)), inc, sigma0_db, phi,
                                             out_wspd, out_sens, out_flag), "xsw_wspd_solve")

    @_locked
    def wspd_solve_cr_raw(self, lines, samples, dtype, out_dtype, mem, inc, sigma0_db, out_wspd, out_sens=None, out_flag=None):
        """Thin call of xsw_wspd_solve_cr: the same on the cross-pol table, which has no direction."""
        self._check(self._lib.xsw_wspd_solve_cr(self._h, int(lines), int(samples), dtype, out_dtype, mem, inc, sigma0_db, out_wspd, out_sens,
                                                out_flag), "xsw_wspd_solve_cr")

    @_locked
    def dir_solve_raw(self, lines, samples, dtype, out_dtype, mem, inc, sigma0_db, wspd, near=None, out_phi1=None, out_phi2=None, out_sens1=None,
                      out_sens2=None, out_phi_near=None, out_sens_near=None, out_phi_closest=None, out_count=None, out_flag=None, fold_phi=True):
        """Thin call of xsw_dir_solve (pointers are ints or None): the directions at which the context's co-pol table gives sigma0_db
        (dB) at incidence inc and wind speed wspd -- the first two in scan order, their sensitivities in degrees per dB, the one
        nearest to the reference direction `near` (None: no selection) and the closest node's direction, each into a real raster of
        `out_dtype`; the uint8 number of solutions and the uint8 DIR_* flags (None: not computed)."""
        self._check(self._lib.xsw_dir_solve(self._h, int(lines), int(samples), dtype, out_dtype, mem, int(bool(fold_phi)), inc, sigma0_db, wspd, near,
                                            out_phi1, out_phi2, out_sens1, out_sens2, out_phi_near, out_sens_near, out_phi_closest, out_count,
                                            out_flag), "xsw_dir_solve")

    def expand_codes_on_stream(self, stream, n, out_dtype, code_co, code_cr, out_co, out_cr):
        """xsw_expand_codes_on_stream: device codes -> device winds on `stream` (a HIP stream handle as an int), the context's
        launch stream untouched."""
        self._check(self._lib.xsw_expand_codes_on_stream(self._h, ctypes.c_void_p(int(stream)), int(n), out_dtype, code_co, code_cr, out_co, out_cr),
                    "xsw_expand_codes_on_stream")

    def expand_codes_host(self, codes_co, codes_cr, out_dtype=np.complex128):
        """Grid codes (uint32 arrays of one shape; either may be None) -> (ws_co, ws_cr) on the host, block-wise on the host
        thread pool (xsw_expand_codes with XSW_MEM_HOST reads the context's host tables only: the blocks run side by side; the
        context's lock is held for the whole expansion so that no LUT is installed meanwhile)."""
        ref = codes_co if codes_co is not None else codes_cr
        shape, n = ref.shape, ref.size
        od = XSW_F32 if np.dtype(out_dtype) == np.complex64 else XSW_F64
        cc = None if codes_co is None else np.ascontiguousarray(codes_co, dtype=np.uint32).reshape(-1)
        cr = None if codes_cr is None else np.ascontiguousarray(codes_cr, dtype=np.uint32).reshape(-1)
        o_co = None if cc is None else np.empty(n, out_dtype)
        o_cr = None if cr is None else np.empty(n, out_dtype)
        item = np.dtype(out_dtype).itemsize
        at = lambda a, i, size: None if a is None else ctypes.c_void_p(a.ctypes.data + i * size)

        def work(i):
            m = min(_host.BLOCK, n - i)
            rc = self._lib.xsw_expand_codes(self._h, m, MEM_HOST, od, at(cc, i, 4), at(cr, i, 4), at(o_co, i, item), at(o_cr, i, item))
            if rc != 0:
                raise XswError(f"xsw_expand_codes failed ({rc}): {self._lib.xsw_last_error(self._h).decode()}")

        with self.lock:
            if n:
                list(_host.pool().map(work, range(0, n, _host.BLOCK)))
        return (None if o_co is None else o_co.reshape(shape)), (None if o_cr is None else o_cr.reshape(shape))

    @_locked
    def set_host_threads(self, n):
        """Worker threads of the host-memory paths (0 = default: XSW_HOST_THREADS or 12)."""
        self._check(self._lib.xsw_set_host_threads(self._h, int(n)), "xsw_set_host_threads")

    @_locked
    def pinned_empty(self, shape, dtype):
        """numpy array in page-locked memory of this context (xsw_host_alloc): rasters filled here can be handed to the
        XSW_MEM_HOST_PINNED paths, which DMA straight out of them.  The memory lives until `pinned_free(arr)` or the context closes."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        p = ctypes.c_void_p()
        self._check(self._lib.xsw_host_alloc(self._h, max(nbytes, 1), ctypes.byref(p)), "xsw_host_alloc")
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=nbytes // dtype.itemsize).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    @_locked
    def pinned_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self._check(self._lib.xsw_host_free(self._h, ctypes.c_void_p(p)), "xsw_host_free")

    @_locked
    def invert_host(self, inc, sigma0_co=None, sigma0_cr=None, dsig_cr=None, anc=None, dsig_co=0.1,
                    sigma0_is_db=False, algo="auto", dual_select=False, out_dtype=np.complex128, want_idx=False, want_codes=False,
                    pinned=False, out_co=None, out_cr=None, stage=None, want_complex=True):
        """numpy-in / numpy-out wrapper of xsw_invert for host rasters of one dtype (float32 or float64).
        want_codes: also return the uint32 grid codes (co, cr) as a 4th element.  pinned: the rasters are page-locked
        (`pinned_empty`): XSW_MEM_HOST_PINNED.  out_co / out_cr: C-contiguous arrays of the broadcast shape and `out_dtype` to
        write into (row tiles of one raster inverted by several contexts land in place).  stage: see `invert_raw`.
        want_complex=False (with want_codes): only the grid codes are produced (nothing is expanded on the host)."""
        inc = np.asarray(inc)
        dt = inc.dtype
        if dt not in (np.float32, np.float64):
            raise TypeError("raster dtype must be float32 or float64")
        cdt = np.complex64 if dt == np.float32 else np.complex128
        shape = np.broadcast_shapes(*(np.shape(a) for a in (inc, sigma0_co, sigma0_cr, anc, None if np.isscalar(dsig_cr) else dsig_cr)
                                      if a is not None))
        inc = np.ascontiguousarray(np.broadcast_to(inc, shape))
        n = inc.size
        lines, samples = lines_samples(shape)

        def prep(a, t):
            if a is None:
                return None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a), shape), dtype=t)
            return a

        s_co, s_cr, anc_ = prep(sigma0_co, dt), prep(sigma0_cr, dt), prep(anc, cdt)
        dsig_scalar = 0.1
        dsig_arr = None
        if dsig_cr is not None:
            if np.isscalar(dsig_cr):
                dsig_scalar = float(dsig_cr)
            else:
                dsig_arr = prep(dsig_cr, dt)
        out_dtype = np.dtype(out_dtype)
        # plain np.empty: the library's worker threads write (and so first-touch) their own chunks side by side
        for o in (out_co, out_cr):
            if o is not None and (o.shape != tuple(shape) or o.dtype != out_dtype or not o.flags.c_contiguous):
                raise ValueError("out_co / out_cr must be C-contiguous arrays of the broadcast shape and out_dtype")
        if s_co is not None and out_co is None and want_complex:
            out_co = np.empty(shape, out_dtype)
        if s_cr is not None and out_cr is None and want_complex:
            out_cr = np.empty(shape, out_dtype)
        if s_co is None:
            out_co = None
        if s_cr is None:
            out_cr = None
        idx = np.empty(shape + (3,), dtype=np.int32) if want_idx else None
        codes = (np.empty(shape, np.uint32) if s_co is not None else None,
                 np.empty(shape, np.uint32) if s_cr is not None else None) if want_codes else (None, None)
        if n:
            self.invert_raw(lines, samples, XSW_F32 if dt == np.float32 else XSW_F64,
                            XSW_F32 if out_dtype == np.complex64 else XSW_F64, MEM_HOST_PINNED if pinned else MEM_HOST,
                            _ptr(inc), _ptr(s_co), _ptr(s_cr), _ptr(dsig_arr), _ptr(anc_), _ptr(out_co), _ptr(out_cr),
                            _ptr(idx), dsig_co, dsig_scalar, sigma0_is_db, algo_code(algo), dual_select,
                            _ptr(codes[0]), _ptr(codes[1]), stage)
        if want_codes:
            return out_co, out_cr, idx, codes
        return out_co, out_cr, idx

    @_locked
    def calibrate_raw(self, lines, samples, mem, dn_dtype, out_dtype, dn, sigma0_lut, noise_range, noise_azimuth, incidence, fill, out_sigma0,
                      out_nesz, out_incidence, out_valid):
        """Thin call of xsw_calibrate (pointers are ints or None).  A table is None or (n_lines, n_samples, values, line_first, line_t,
        sample_first, sample_t) with the five arrays as addresses; fill is a number, or None for no fill value."""
        tabs = [None if t is None else Table(int(t[0]), int(t[1]), *t[2:]) for t in (sigma0_lut, noise_range, noise_azimuth, incidence)]
        self._check(self._lib.xsw_calibrate(self._h, int(lines), int(samples), mem, dn_dtype, out_dtype, dn,
                                            *[None if t is None else ctypes.byref(t) for t in tabs], int(fill is not None),
                                            0.0 if fill is None else float(fill), out_sigma0, out_nesz, out_incidence, out_valid), "xsw_calibrate")

    @_locked
    def nesz_flatten_raw(self, lines, samples, dtype, mem, noise_ptr, inc_ptr, out_ptr):
        """Thin call of xsw_nesz_flatten (pointers are ints: device or host addresses)."""
        self._check(self._lib.xsw_nesz_flatten(self._h, int(lines), int(samples), dtype, mem, ctypes.c_void_p(noise_ptr),
                                               ctypes.c_void_p(inc_ptr), ctypes.c_void_p(out_ptr)), "xsw_nesz_flatten")

    @_locked
    def dsig_raw(self, rule, lines, samples, dtype, nesz_dtype, mem, inc_ptr, sigma0_ptr, nesz_ptr, out_ptr):
        """Thin call of xsw_dsig (pointers are ints: device or host addresses; inc_ptr None unless the rule is S1_V2)."""
        self._check(self._lib.xsw_dsig(self._h, int(rule), int(lines), int(samples), dtype, nesz_dtype, mem, _ptr(inc_ptr), _ptr(sigma0_ptr),
                                       _ptr(nesz_ptr), _ptr(out_ptr)), "xsw_dsig")

    @_locked
    def dsig_flat_raw(self, rule, lines, samples, dtype, out_dtype, mem, noise_ptr, inc_ptr, sigma0_ptr, out_ptr):
        """Thin call of xsw_dsig_flat (pointers are ints: device or host addresses)."""
        self._check(self._lib.xsw_dsig_flat(self._h, int(rule), int(lines), int(samples), dtype, out_dtype, mem, _ptr(noise_ptr), _ptr(inc_ptr),
                                            _ptr(sigma0_ptr), _ptr(out_ptr)), "xsw_dsig_flat")

    @_locked
    def dsig_wspd_raw(self, rule, n, mem, u_ptr, snr_ptr, out_ptr):
        """Thin call of xsw_dsig_wspd (float64 values; pointers are ints: device or host addresses)."""
        self._check(self._lib.xsw_dsig_wspd(self._h, int(rule), int(n), mem, _ptr(u_ptr), _ptr(snr_ptr), _ptr(out_ptr)), "xsw_dsig_wspd")

    @_locked
    def nesz_flatten_host(self, noise, inc):
        """xsw_nesz_flatten on host rasters of one dtype (float32 or float64) and one 2-D shape -> float64."""
        noise, inc = np.asarray(noise), np.asarray(inc)
        # one raster dtype on the device: the wider of the two (a float64 incidence is never narrowed to a float32 noise raster)
        dt = np.result_type(noise.dtype, inc.dtype)
        if dt not in (np.float32, np.float64):
            dt = np.dtype(np.float64)
        noise = np.ascontiguousarray(noise, dtype=dt)
        inc = np.ascontiguousarray(inc, dtype=dt)
        if noise.ndim != 2 or inc.shape != noise.shape:
            raise ValueError("noise and inc must be 2-D rasters of one shape")
        out = np.empty(noise.shape, np.float64)
        if noise.size:
            self.nesz_flatten_raw(noise.shape[0], noise.shape[1], XSW_F32 if noise.dtype == np.float32 else XSW_F64, MEM_HOST,
                                  noise.ctypes.data, inc.ctypes.data, out.ctypes.data)
        return out

    @_locked
    def grad_keep_raw(self, lines, samples, mem, src_ptr, threshold, block, and_with_ptr, out_ptr):
        """xsw_grad_keep_f64 or, with threshold None, xsw_grad_keep_u8 (RASTER_ENTRIES)."""
        if threshold is None:
            self.grad_keep_u8_raw(lines, samples, mem, src_ptr, block, and_with_ptr, out_ptr)
        else:
            self.grad_keep_f64_raw(lines, samples, mem, src_ptr, threshold, block, and_with_ptr, out_ptr)

    @_locked
    def detrend_raw(self, lines, samples, dtype, out_dtype, mem, sigma0_ptr, ratio_row, out_ptr):
        """Thin call of xsw_detrend (raster pointers are ints; ratio_row is a host float64 array)."""
        ratio_row = _f64(ratio_row)
        self._check(self._lib.xsw_detrend(self._h, int(lines), int(samples), dtype, out_dtype, mem,
                                          ctypes.c_void_p(sigma0_ptr), _ptr(ratio_row), ctypes.c_void_p(out_ptr)),
                    "xsw_detrend")

    @_locked
    def detrend_host(self, sigma0, ratio_row, out_dtype=np.float64):
        sigma0 = np.ascontiguousarray(sigma0)
        if sigma0.dtype not in (np.float32, np.float64):
            sigma0 = sigma0.astype(np.float64)
        ratio_row = _f64(ratio_row)
        lines, samples = int(np.prod(sigma0.shape[:-1])), sigma0.shape[-1]
        if ratio_row.shape != (samples,):
            raise ValueError("ratio_row must have one value per sample")
        out = np.empty(sigma0.shape, out_dtype)
        self._check(self._lib.xsw_detrend(self._h, lines, samples, XSW_F32 if sigma0.dtype == np.float32 else XSW_F64,
                                          XSW_F32 if out.dtype == np.float32 else XSW_F64, MEM_HOST,
                                          _ptr(sigma0), _ptr(ratio_row), _ptr(out)), "xsw_detrend")
        return out



def _raw_method(name, sig):
    convert = [_SIG[k][1] for k in sig]

    def method(self, *args):
        if len(args) != len(convert):
            raise TypeError(f"{name} takes {len(convert)} arguments after the context, not {len(args)}")
        self._check(getattr(self._lib, name)(self._h, *[f(a) for f, a in zip(convert, args)]), name)
    method.__name__ = name[len("xsw_"):] + "_raw"
    method.__doc__ = f"Thin call of {name}: see RASTER_ENTRIES for the arguments."
    return _locked(method)


for _name, _sig in RASTER_ENTRIES.items():
    setattr(Context, _name[len("xsw_"):] + "_raw", _raw_method(_name, _sig))


_default_ctx = {}
_default_ctx_lock = threading.Lock()


def default_context(device=0, replica=0):
    """Process-wide context per device (created on first use).  replica > 0: further contexts on the same device
    (`options.devices = [0, 0]`: the single-process multi-device path rehearsed on one GPU)."""
    key = (int(device), int(replica))
    with _default_ctx_lock:
        if key not in _default_ctx:
            _default_ctx[key] = Context(device)
        return _default_ctx[key]


def contexts_for(devices):
    """One context per entry of `devices` (a device listed twice gets two contexts)."""
    seen = {}
    out = []
    for d in devices:
        k = seen.get(d, 0)
        seen[d] = k + 1
        out.append(default_context(d, k))
    return out
