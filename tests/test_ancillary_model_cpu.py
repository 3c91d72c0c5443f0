"""CPU: the restatement of xsarsea_amd.ancillary (tests/ancillary_model_ref.py) against the notebook's own three expressions and on
hand-built cases, and the public call's host checks, which all precede the first device call."""
import os
import re

import numpy as np
import pytest

import ancillary_model_ref as aref
from conftest import REPO
from xsarsea_amd import _lib, ancillary

def notebook(u, v, heading):
    """docs/examples/windspeed_retrieval_L1.ipynb of the reference, with detrend.dir_meteo_to_sample written out."""
    ancillary_wind_direction = (90. - np.rad2deg(np.arctan2(v, u)) + 180) % 360
    ancillary_wind_speed = np.sqrt(u**2 + v**2)
    return ancillary_wind_speed * np.exp(1j * (np.pi / 2 - np.deg2rad(ancillary_wind_direction - heading)))


def scene_on_nodes(n_lat, n_lon, lon0=-12.0, dlon=0.25, lat0=40.0, dlat=0.125):
    """A raster whose tie grid is the raster itself and whose pixel (l, s) sits on model node (l, s): interpolation is trivial
    (the steps are dyadic, so the node coordinates and the cell coordinates are exact)."""
    lon, lat = lon0 + dlon * np.arange(n_lon), lat0 + dlat * np.arange(n_lat)
    return lon, lat, np.arange(n_lat, dtype=float), np.arange(n_lon, dtype=float), np.tile(lon, (n_lat, 1)), np.tile(lat[:, None], (1, n_lon))


def test_restatement_is_the_notebooks_three_expressions():
    """Bound 1e-13 |wind|: the notebook path rounds a handful of degree values below 1024, each within 2**-43 deg ~ 2e-15 rad
    (2e6 such points gave a maximum of 3.0e-15); the closed form rounds a few times at 1.1e-16.  Exactly 0 where u = v = 0."""
    rng = np.random.default_rng(7)
    n_lat, n_lon = 200, 300
    u, v = rng.normal(0, 12, (n_lat, n_lon)), rng.normal(0, 12, (n_lat, n_lon))
    u[3, 5] = v[3, 5] = 0.0
    u[10, :20] = 0.0
    v[20, :20] = 0.0
    u[0, 0] = v[0, 0] = 0.0
    u[-1, -1] = 0.0
    heading = rng.uniform(-360, 360, (n_lat, n_lon))
    heading[3, 6], heading[10, 1], heading[20, 1] = 0.0, 90.0, -180.0
    lon, lat, tl, ts, glon, glat = scene_on_nodes(n_lat, n_lon)
    got = aref.ancillary_from_model(u, v, lon, lat, tl, ts, glon, glat, heading, tl, ts)
    want = notebook(u, v, heading)
    err, size = np.abs(got - want), np.abs(want)
    print(f"max |delta| / |wind| = {np.max(err[size > 0] / size[size > 0]):.3g} (bound 1e-13)")
    assert not np.isnan(got.real).any() and not np.isnan(got.imag).any()
    assert (err <= 1e-13 * size).all()
    calm = (u == 0) & (v == 0)
    assert calm.sum() == 2 and (got[calm] == 0).all() and (want[calm] == 0).all()
    assert ((u == 0) & (v != 0)).sum() >= 20 and ((v == 0) & (u != 0)).sum() >= 20


def test_sign_is_the_gmfs_from_sense():
    lon, lat, tl, ts, glon, glat = scene_on_nodes(2, 2)
    u, v, zero = np.full((2, 2), 5.0), np.zeros((2, 2)), np.zeros((2, 2))
    east = aref.ancillary_from_model(u, v, lon, lat, tl, ts, glon, glat, zero, tl, ts)
    assert (east == -5.0).all()  # heading 0: the line axis points north, the sample axis east; a wind blowing to the east comes from +sample
    north = aref.ancillary_from_model(v, u, lon, lat, tl, ts, glon, glat, zero, tl, ts)
    assert (north == -5.0j).all()
    turned = aref.ancillary_from_model(u, v, lon, lat, tl, ts, glon, glat, zero + 90.0, tl, ts)  # the line axis points east
    assert np.abs(turned - (-5.0j)).max() < 1e-15


def unit_square():
    """Model nodes (lat, lon) in {0, 1} x {0, 1}; a 3 x 3 raster over it from a 2 x 2 tie grid, heading 0: out = -(u + 1j v)."""
    u = np.array([[1.0, 2.0], [3.0, 4.0]])
    args = dict(model_lon=[0.0, 1.0], model_lat=[0.0, 1.0], tie_line=[0.0, 2.0], tie_sample=[0.0, 2.0], tie_lon=[[0.0, 1.0], [0.0, 1.0]],
                tie_lat=[[0.0, 0.0], [1.0, 1.0]], tie_heading=np.zeros((2, 2)), line=np.arange(3.0), sample=np.arange(3.0))
    return u, args


def test_midway_is_the_mean_and_a_node_is_the_node():
    u, args = unit_square()
    out = aref.ancillary_from_model(u, 10 * u, **args)
    assert out[1, 1] == -(2.5 + 25j)                                  # midway between the four nodes
    assert out[0, 0] == -(1 + 10j) and out[0, 2] == -(2 + 20j) and out[2, 0] == -(3 + 30j) and out[2, 2] == -(4 + 40j)
    assert out[0, 1] == -(1.5 + 15j) and out[1, 0] == -(2 + 20j)      # midway along one axis
    out32 = aref.ancillary_from_model(u.astype(np.float32), (10 * u).astype(np.float32), **args)
    assert aref.same_bits(out32, out)


def random_scene(rng, n_lat=7, n_lon=9, L=23, S=31, lon_span=(9.5, 18.5), lat_span=(-3.5, 4.5)):
    """Regional grid lon 10 .. 18, lat -3 .. 3; a tilted scene that leaves it on every side."""
    u, v = rng.normal(0, 12, (n_lat, n_lon)), rng.normal(0, 12, (n_lat, n_lon))
    tl, ts = np.array([0.0, 7.0, L - 1.0]), np.array([0.0, 4.0, 19.0, S - 1.0])
    fl, fs = tl[:, None] / (L - 1), ts[None, :] / (S - 1)
    glon = lon_span[0] + (lon_span[1] - lon_span[0]) * fs + 0.4 * fl
    glat = lat_span[1] - (lat_span[1] - lat_span[0]) * fl + 0.3 * fs
    heading = -168.0 + 5 * fl + 3 * fs
    return u, v, 10.0 + np.arange(n_lon), -3.0 + np.arange(n_lat), tl, ts, glon, glat, heading, np.arange(float(L)), np.arange(float(S))


def test_descending_latitude_is_the_flipped_grid():
    u, v, lon, lat, *rest = random_scene(np.random.default_rng(3))
    up = aref.ancillary_from_model(u, v, lon, lat, *rest)
    down = aref.ancillary_from_model(u[::-1], v[::-1], lon, lat[::-1], *rest)
    assert aref.same_bits(down, up) and np.isnan(up.real).any() and not np.isnan(up.real).all()
    # the C entry's own signed dlat gives the same raster to rounding (its cell coordinate is the mirrored one, rounded anew)
    tl, ts, glon, glat, heading, line, sample = rest
    h = np.deg2rad(heading)
    lf, lt = aref.bracket(tl, line)
    sf, st = aref.bracket(ts, sample)
    signed = aref.core(u[::-1], v[::-1], lon[0], 1.0, False, lat[-1], -1.0, glon, glat, np.cos(h), np.sin(h), lf, lt, sf, st)
    ok = ~np.isnan(up.real) & ~np.isnan(signed.real)
    assert ok.sum() > 0.5 * ok.size and np.abs(signed[ok] - up[ok]).max() < 1e-12 * np.abs(u).max()


def periodic_grid():
    rng = np.random.default_rng(5)
    return rng.normal(0, 12, (3, 8)), rng.normal(0, 12, (3, 8)), 45.0 * np.arange(8), np.array([-10.0, 0.0, 10.0])


def test_periodic_grid_closes_at_its_seam():
    u, v, lon, lat = periodic_grid()
    one = lambda x: aref.ancillary_from_model(u, v, lon, lat, [0.0], [0.0], [[x]], [[0.0]], [[0.0]], [0.0], [0.0])[0, 0]
    t = 350.0 / 45.0 - 7.0
    want = -complex((1.0 - t) * u[1, 7] + t * u[1, 0], (1.0 - t) * v[1, 7] + t * v[1, 0])
    assert one(350.0) == want                                   # between node 7 (315) and node 0
    for turn in (-360.0, 360.0):  # the reduced cell coordinate is rounded anew: the same blend to rounding
        assert abs(one(350.0 + turn) - want) < 1e-13 * abs(want)
    assert one(0.0) == one(360.0) == one(-360.0) == -complex(u[1, 0], v[1, 0])
    assert one(315.0) == -complex(u[1, 7], v[1, 7])


def test_antimeridian_tie_grid_is_made_continuous():
    u, v, lon, lat = periodic_grid()
    tl, ts = np.array([0.0, 8.0]), np.array([0.0, 5.0, 10.0, 15.0, 20.0])
    across = np.tile(np.array([170.0, 175.0, 180.0, 185.0, 190.0]), (2, 1))
    wrapped = np.where(across > 180.0, across - 360.0, across)
    assert wrapped[0, -1] == -170.0
    glat, heading = np.tile(np.array([[-4.0], [6.0]]), (1, 5)), np.full((2, 5), 12.0)
    line, sample = np.arange(9.0), np.arange(21.0)
    a = aref.ancillary_from_model(u, v, lon, lat, tl, ts, across, glat, heading, line, sample)
    b = aref.ancillary_from_model(u, v, lon, lat, tl, ts, wrapped, glat, heading, line, sample)
    assert aref.same_bits(a, b) and not np.isnan(a.real).any()
    np.testing.assert_array_equal(aref.continuous(wrapped), across)
    np.testing.assert_array_equal(ancillary.TiePoints(tl, ts, wrapped, glat, heading).longitude, across)
    col = np.array([[179.0, -179.0], [-178.0, 178.0]])  # the first column crosses too
    np.testing.assert_array_equal(aref.continuous(col), [[179.0, 181.0], [182.0, 178.0]])
    np.testing.assert_array_equal(ancillary.TiePoints([0, 1], [0, 1], col, col * 0, col * 0).longitude, aref.continuous(col))


def test_outside_a_regional_grid_is_nan_and_the_last_node_is_not():
    u, args = unit_square()
    args.update(tie_lon=[[-1.0, 1.0], [-1.0, 1.0]], tie_lat=[[-1.0, -1.0], [1.0, 1.0]])  # the 3 x 3 pixels sit at -1, 0, 1
    out = aref.ancillary_from_model(u, 10 * u, **args)
    assert np.isnan(out[0].real).all() and np.isnan(out[:, 0].imag).all()
    assert out[1, 1] == -(1 + 10j) and out[1, 2] == -(2 + 20j) and out[2, 1] == -(3 + 30j) and out[2, 2] == -(4 + 40j)  # 2, 2: the last node of both axes
    args.update(tie_lon=[[0.0, 1.0 + 2**-40], [0.0, 1.0 + 2**-40]], tie_lat=[[0.0, 0.0], [1.0, 1.0]])
    out = aref.ancillary_from_model(u, 10 * u, **args)
    assert np.isnan(out[:, 2].real).all() and not np.isnan(out[:, :2].real).any()


def test_a_nan_node_is_nan_at_weight_zero_as_well():
    u, args = unit_square()
    u[0, 1] = np.nan
    out = aref.ancillary_from_model(u, np.ones((2, 2)), **args)
    assert np.isnan(out[0, 0].real) and np.isnan(out[2, 0].real)   # on node (0, 0) and on node (1, 0): the NaN node weighs 0
    assert np.isnan(out.real).all() and np.isnan(out.imag).all()   # both parts hold u
    out = aref.ancillary_from_model(np.ones((2, 2)), np.ones((2, 2)), **args)
    assert not np.isnan(out.real).any()


def test_cancelling_headings_are_nan():
    one, z = np.ones((1, 2)), np.zeros((1, 2))
    out = aref.core(np.ones((2, 2)), np.ones((2, 2)), 0.0, 1.0, False, 0.0, 1.0, 0.5 * one, 0.5 * one, np.array([[1.0, -1.0]]), z,
                    np.array([0], np.int32), np.zeros(1), np.array([0, 0, 0], np.int32), np.array([0.0, 0.5, 1.0]))
    assert out[0, 0] == -(1 + 1j) and out[0, 2] == (1 + 1j) and np.isnan(out[0, 1].real) and np.isnan(out[0, 1].imag)


# ---------------------------------------------------------------------------------------------------- the public call's host checks
def public_args():
    u, v, lon, lat, tl, ts, glon, glat, heading, line, sample = random_scene(np.random.default_rng(11))
    return dict(model_u=u, model_v=v, model_lon=lon, model_lat=lat, tie_points=ancillary.TiePoints(tl, ts, glon, glat, heading),
                line=line, sample=sample), (tl, ts, glon, glat, heading)


@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the checks must have refused the call before."""
    def touched(*a, **k):
        raise AssertionError("a device call was reached before the host checks refused the arguments")
    monkeypatch.setattr(ancillary, "_Call", touched)
    monkeypatch.setattr(_lib, "default_context", touched)


def test_shape_and_coordinates_exclude_each_other(no_device):
    args, _ = public_args()
    with pytest.raises(ValueError, match="exactly one"):
        ancillary.ancillary_from_model(**args, shape=(23, 31))
    del args["line"], args["sample"]
    with pytest.raises(ValueError, match="exactly one"):
        ancillary.ancillary_from_model(**args)
    with pytest.raises(ValueError):
        ancillary.ancillary_from_model(**args, line=np.arange(23.0))


def test_raster_outside_the_tie_span_is_refused(no_device):
    args, _ = public_args()
    for key, bad in (("line", np.arange(24.0)), ("sample", np.arange(31.0) - 0.5)):
        with pytest.raises(ValueError, match="extrapolated"):
            ancillary.ancillary_from_model(**{**args, key: bad})
    del args["line"], args["sample"]
    with pytest.raises(ValueError, match="extrapolated"):
        ancillary.ancillary_from_model(**args, shape=(24, 31))
    tp = ancillary.TiePoints([4.0], [0.0, 30.0], [[10.0, 11.0]], [[0.0, 0.0]], [[0.0, 0.0]])  # a single tie line
    with pytest.raises(ValueError):
        ancillary.ancillary_from_model(**{**args, "tie_points": tp}, line=[4.0, 4.0], sample=np.arange(31.0))
    with pytest.raises(ValueError, match="extrapolated"):
        ancillary.ancillary_from_model(**{**args, "tie_points": tp}, shape=(1, 31))


@pytest.mark.parametrize("axis", ["model_lon", "model_lat"])
def test_non_uniform_model_axis_is_refused(no_device, axis):
    args, _ = public_args()
    moved = np.array(args[axis], dtype=float)
    moved[3] += 0.01 * (moved[1] - moved[0])
    with pytest.raises(ValueError, match="not uniform"):
        ancillary.ancillary_from_model(**{**args, axis: moved})
    with pytest.raises(ValueError, match="not uniform"):
        aref.uniform(moved, axis)
    with pytest.raises(ValueError):
        ancillary.ancillary_from_model(**{**args, axis: np.asarray(args[axis])[:1]})
    if axis == "model_lon":
        with pytest.raises(ValueError, match="ascend"):
            ancillary.ancillary_from_model(**{**args, axis: np.asarray(args[axis])[::-1]})


@pytest.mark.parametrize("axis", ["model_lon", "model_lat"])
def test_a_node_moved_by_a_ten_thousandth_of_a_step_is_accepted(axis):
    args, _ = public_args()
    moved = np.array(args[axis], dtype=float)
    moved[3] += 1e-4 * (moved[1] - moved[0])
    assert ancillary._uniform_axis(moved, axis)[2] == len(moved) and aref.uniform(moved, axis)[2] == len(moved)
    try:  # every host check passes: the call gets as far as the device
        out = ancillary.ancillary_from_model(**{**args, axis: moved})
    except _lib.XswError:
        assert _lib.device_count_safe() == 0
    else:
        assert out.shape == (23, 31)


def test_model_fields_of_different_shape_or_dtype_are_refused(no_device):
    args, _ = public_args()
    for bad in (args["model_v"][:, :-1], args["model_v"].astype(np.float32), args["model_v"][None]):
        with pytest.raises(ValueError):
            ancillary.ancillary_from_model(**{**args, "model_v": bad})
    with pytest.raises(ValueError, match="float32 or float64"):
        ancillary.ancillary_from_model(**{**args, "model_u": args["model_u"].astype(np.float16), "model_v": args["model_v"].astype(np.float16)})
    with pytest.raises(ValueError, match="do not match the axes"):
        ancillary.ancillary_from_model(**{**args, "model_u": args["model_u"].T.copy(), "model_v": args["model_v"].T.copy()})


def test_tie_grids_are_checked():
    _, (tl, ts, glon, glat, heading) = public_args()
    for k in range(3):
        grids = [glon.copy(), glat.copy(), heading.copy()]
        grids[k][1, 2] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            ancillary.TiePoints(tl, ts, *grids)
        grids[k] = grids[k][:, :-1]
        with pytest.raises(ValueError, match=r"\[line, sample\]"):
            ancillary.TiePoints(tl, ts, *grids)
    with pytest.raises(ValueError, match=r"\[line, sample\]"):
        ancillary.TiePoints(tl, ts, glon.T, glat.T, heading.T)
    with pytest.raises(ValueError, match="ascending"):
        ancillary.TiePoints(tl[::-1], ts, glon, glat, heading)
    with pytest.raises(ValueError, match="NaN"):
        ancillary.TiePoints([0.0, np.nan, 22.0], ts, glon, glat, heading)
    with pytest.raises(ValueError):
        aref.ancillary_from_model(np.ones((7, 9)), np.ones((7, 9)), np.arange(9.0), np.arange(7.0), tl, ts, glon, glat * np.nan, heading, [0.0], [0.0])


def test_public_names():
    import xsarsea_amd
    assert xsarsea_amd.TiePoints is ancillary.TiePoints and xsarsea_amd.ancillary_from_model is ancillary.ancillary_from_model
    assert {"ancillary", "TiePoints", "ancillary_from_model"} <= set(xsarsea_amd.__all__)


def test_brackets_and_tables_agree_with_the_restatement():
    """What the public call hands to the kernel, against the restatement's own host steps."""
    from xsarsea_amd import streaks
    ties, coords = np.array([2.0, 3.5, 9.0, 9.25]), np.array([2.0, 2.5, 3.5, 8.0, 9.0, 9.125, 9.25])
    for t, c in ((ties, coords), (ties[:1], ties[:1])):
        f, w = streaks.bracket(t, c)
        rf, rw = aref.bracket(t, c)
        np.testing.assert_array_equal(f, rf)
        np.testing.assert_array_equal(w, rw)


# ------------------------------------------------------------------------------------------------------------- header and library
def test_header_declares_the_entry_and_the_binding_has_one_letter_per_argument():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+xsw_ancillary_model\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/xsw.h does not declare xsw_ancillary_model"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[0].startswith("xsw_ctx")
    sig = _lib.RASTER_ENTRIES["xsw_ancillary_model"]
    assert len(sig) == len(params) - 1 == 24
    for letter, p in zip(sig, params[1:]):
        want = "p" if "*" in p else {"int64_t": "l", "int32_t": "i", "double": "d"}[p.split()[0]]
        assert letter == want, p
    assert "xsw_ancillary_model" in _lib.EXPORTS and hasattr(_lib.Context, "ancillary_model_raw")
    assert hasattr(_lib.load(), "xsw_ancillary_model")
