"""xsarsea_amd: MI355X-native (gfx950) wind-inversion hot path of xsarsea.

Drop-in for `xsarsea.windspeed.invert_from_model`, `xsarsea.sigma0_detrend` and `xsarsea.gradients` (plus `streaks`, the link from its histograms to the inversion's a-priori wind, `ancillary`, that wind from a model grid, `cells`, the retrieved wind on a product grid, `grid`, that wind on a longitude / latitude grid, `polar`, that wind in rings and sectors around a cyclone's centre, `centre`, that centre found in the wind field itself, `calibrate`, sigma0, NESZ and incidence from a product's digital numbers, and `landmask`, the sea / land keep mask from coastline polygons): same signatures,
same container conventions, results identical to the reference's CPU path; the per-pixel work runs
in hand-written HIP kernels behind the C ABI of include/xsw.h (no CPU fallback).  See DESIGN.md.
"""
__version__ = "0.1.0"
__all__ = ["sigma0_detrend", "windspeed", "gradients", "streaks", "ancillary", "TiePoints", "ancillary_from_model", "cells", "WindCells", "RasterCells",
           "wind_cells", "raster_cells", "grid", "WindGrid", "wind_grid", "polar", "WindPolar", "wind_polar", "centre", "CentreSpec", "CentreScores", "CentreFix",
           "wind_centre_scores", "find_centre", "calibrate", "AnnotationGrid", "Calibrated",
           "calibrate_dn", "raster_from_grid", "landmask", "Coastline", "land_mask", "options", "dir_meteo_to_sample", "dir_sample_to_meteo", "dir_meteo_to_oceano",
           "dir_oceano_to_meteo", "dir_to_180", "dir_to_360", "read_sarwing_owi"]

from . import ancillary, calibrate, cells, centre, gradients, grid, landmask, options, polar, streaks, windspeed
from .ancillary import TiePoints, ancillary_from_model
from .calibrate import AnnotationGrid, Calibrated, calibrate_dn, raster_from_grid
from .cells import RasterCells, WindCells, raster_cells, wind_cells
from .centre import CentreFix, CentreScores, CentreSpec, find_centre, wind_centre_scores
from .grid import WindGrid, wind_grid
from .landmask import Coastline, land_mask
from .polar import WindPolar, wind_polar
from .detrend import (dir_meteo_to_oceano, dir_meteo_to_sample, dir_oceano_to_meteo, dir_sample_to_meteo, dir_to_180,
                      dir_to_360, read_sarwing_owi, sigma0_detrend)
