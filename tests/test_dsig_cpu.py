"""Host side of the dsig_cr step: `dsig_from_nesz` as the composition it stands for, the binding's symbol list and the
name -> rule tables (no GPU; the device kernels are covered by tests/test_gpu_dsig.py)."""
import warnings

import numpy as np
import pytest

from conftest import golden

DSIG_NAMES = ("gmf_s1_v2", "gmf_rs2_v2", "sarwing_lut_cmodms1ahw", "nc_lut_cmodms1ahw")
DSIG_WSPD_NAMES = ("dsig_wspd_rs2_v3", "dsig_wspd_s1_ew_rec_v3", "dsig_wspd_rcm_v3")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture
def host_flattening():
    from xsarsea_amd import options
    old = options.nesz_on_device
    options.nesz_on_device = "host"
    yield
    options.nesz_on_device = old


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", DSIG_NAMES)
def test_dsig_from_nesz_is_get_dsig_on_the_flattened_noise(host_flattening, name, dtype):
    """On the golden noise rasters, with a sigma0 derived from them (negative, zero and NaN pixels included): bit-equal to
    get_dsig on the reference's own flattened noise, and `out_dtype=np.float32` is the `.astype` of that."""
    from xsarsea_amd.windspeed import dsig_from_nesz, get_dsig
    d = golden("crosspol_prep.npz")
    noise, inc = d["nesz_noise"].astype(dtype), d["nesz_inc"].astype(dtype)
    flat = d["nesz_flat" if dtype == np.float64 else "nesz_flat32"]
    rng = np.random.default_rng(11)
    s = (d["nesz_noise"] * rng.gamma(2.0, 2.0, noise.shape) - 0.5 * d["nesz_noise"]).astype(dtype)  # a tenth or so negative
    s[3, 5], s[7, 1] = 0.0, np.nan
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = get_dsig(name, inc, s, flat)
        got = dsig_from_nesz(name, inc, s, noise)
        got32 = dsig_from_nesz(name, inc, s, noise, out_dtype=np.float32)
    assert want.dtype == np.float64 and np.isfinite(want).any() and (s < 0).any()
    assert _same(got, want)
    assert _same(got32, want.astype(np.float32))


def test_dsig_from_nesz_errors(host_flattening):
    from xsarsea_amd.windspeed import dsig_from_nesz
    d = golden("crosspol_prep.npz")
    with pytest.raises(IndexError):
        dsig_from_nesz("gmf_rs2_v2", d["nesz_inc"][0], d["nesz_noise"][0], d["nesz_noise"][0])
    with pytest.raises(ValueError):
        dsig_from_nesz("nope", d["nesz_inc"], d["nesz_noise"], d["nesz_noise"])


def test_binding_lists_the_dsig_symbols():
    from xsarsea_amd import _lib
    for sym in ("xsw_dsig", "xsw_dsig_flat", "xsw_dsig_wspd"):
        assert sym in _lib.EXPORTS
    for method in ("dsig_raw", "dsig_flat_raw", "dsig_wspd_raw"):
        assert callable(getattr(_lib.Context, method))


def test_rule_tables_cover_the_seven_names():
    """Exactly the reference's four get_dsig names (the two cmodms1ahw names share a rule) and its three get_dsig_wspd names,
    numbered as include/xsw.h numbers them, and the host route knows the same ones."""
    from xsarsea_amd import _lib
    from xsarsea_amd.windspeed import utils
    assert set(_lib.DSIG_RULES) == set(DSIG_NAMES) and set(_lib.DSIG_WSPD_RULES) == set(DSIG_WSPD_NAMES)
    assert _lib.DSIG_RULES == {"gmf_s1_v2": 0, "gmf_rs2_v2": 1, "sarwing_lut_cmodms1ahw": 2, "nc_lut_cmodms1ahw": 2}
    assert [_lib.DSIG_WSPD_RULES[n] for n in DSIG_WSPD_NAMES] == [0, 1, 2]
    assert set(utils._DSIG_WSPD) == set(DSIG_WSPD_NAMES)
    for n in DSIG_NAMES:
        assert np.isfinite(utils.get_dsig(n, 30.0, 2.0, 1.0))
    with pytest.raises(ValueError):
        utils.get_dsig("nope", 30.0, 2.0, 1.0)
