"""windspeed: wind retrieval from sigma0 and models (public names of `xsarsea.windspeed`)."""
__all__ = ["invert_from_model", "available_models", "get_model", "register_cmod7", "register_pickle_luts", "register_nc_luts",
           "register_luts", "nesz_flattening", "GmfModel", "Model", "gmfs", "gmfs_impl", "get_dsig", "get_dsig_wspd", "dsig_from_nesz", "invert_copol_codes", "CopolCodes", "InversionCost", "InversionUncertainty",
           "simulate_sigma0", "SimulatedSigma0", "retrieve_wspd", "RetrievedWspd",
           "retrieve_dir", "RetrievedDir", "retrieve_wind", "invert_joint", "JointInversion", "JointUncertainty"]

from . import gmfs, gmfs_impl
from .cmod7 import register_cmod7
from .crosspol import CopolCodes, InversionCost, InversionUncertainty, JointInversion, JointUncertainty, invert_copol_codes, invert_joint
from .forward import SimulatedSigma0, simulate_sigma0
from .gmfs import GmfModel
from .models import Model, available_models, get_model, register_luts, register_nc_luts
from .pickle_luts import register_pickle_luts
from .retrieve import RetrievedWspd, retrieve_wspd
from .retrieve_dir import RetrievedDir, retrieve_dir, retrieve_wind
from .utils import dsig_from_nesz, get_dsig, get_dsig_wspd, nesz_flattening
from .windspeed import invert_from_model
