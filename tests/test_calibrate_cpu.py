"""CPU: the restatement of xsarsea_amd.calibrate (tests/calibrate_ref.py) on closed forms, against the geolocation the other
restatements compute, its fill / valid rules; the public calls' host checks, which all precede the first device call; the
declarations; and the launch tests/calibrate_cases.py states against strip_grid (csrc/xsw_plan.hpp, compiled on the host)."""
import ctypes
import os
import re

import numpy as np
import pytest

import calibrate_cases as cc
import calibrate_ref as cref
import grid_cases as gc
import grid_ref as gref
from conftest import REPO
from test_host_plan import ask, source_define  # noqa: F401  (ask: the fixture that compiles xsw_plan.hpp)
from xsarsea_amd import AnnotationGrid, Calibrated, TiePoints, _lib, calibrate, calibrate_dn, raster_from_grid


def flat(value, line=(0.0, 9.0), sample=(0.0, 19.0)):
    return np.array(line), np.array(sample), np.full((len(line), len(sample)), float(value))


# ------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("k", [0, 4, 9])
def test_a_power_of_two_lut_gives_the_exact_quotient(k):
    """A = 2**k everywhere: every blend is exact, g = 2**-2k, and sigma0 == dn**2 / A**2 to the bit; no noise table, nesz == 0."""
    rng = np.random.default_rng(k)
    dn = rng.integers(1, 65536, (10, 20)).astype(np.uint16)
    dn[0, 0], dn[9, 19] = 65535, 1
    for d in (dn, dn.astype(np.float32)):
        got = cref.calibrate(d, flat(2.0 ** k), dtype=np.float64)
        want = dn.astype(np.float64) ** 2 / 4.0 ** k
        assert got["sigma0"].dtype == np.float64 and np.array_equal(got["sigma0"], want) and (got["nesz"] == 0.0).all()
        assert got["valid"].all() and got["incidence"] is None
        f32 = cref.calibrate(d, flat(2.0 ** k), dtype=np.float32)
        assert f32["sigma0"].dtype == np.float32 and np.array_equal(f32["sigma0"], want.astype(np.float32))
    noisy = cref.calibrate(dn, flat(2.0 ** k), noise_range=flat(6.0), noise_azimuth=flat(0.5), dtype=np.float64)
    assert np.array_equal(noisy["nesz"], np.full(dn.shape, 3.0 / 4.0 ** k)) and np.array_equal(noisy["sigma0"], (dn.astype(np.float64) ** 2 - 3.0) / 4.0 ** k)


def test_a_lut_linear_in_sample_reproduces_itself_where_the_weights_are_dyadic():
    """Nodes at samples 0, 64, 192 and lines 0, 8: every bracket weight is a multiple of 2**-7, every product and sum exact."""
    gs, gl = np.array([0.0, 64.0, 192.0]), np.array([0.0, 8.0])
    f = lambda line, sample: 3.0 + 0.5 * sample + 0.25 * line
    grid = (gl, gs, f(gl[:, None], gs[None, :]))
    line, sample = np.arange(9.0), np.arange(193.0)
    got = cref.blend(grid, line, sample)
    assert np.array_equal(got, f(line[:, None], sample[None, :]))
    assert np.array_equal(cref.raster_from_grid(grid, line, sample, np.float32), f(line[:, None], sample[None, :]).astype(np.float32))
    # a jump stated by two neighbouring nodes: pixel 64 reads the first alone, pixel 65 the second
    jump = (np.array([0.0]), np.array([0.0, 64.0, 65.0, 192.0]), np.array([[1.0, 2.0, 10.0, 12.0]]))
    row = cref.blend(jump, np.zeros(1), sample)[0]
    assert row[64] == 2.0 and row[65] == 10.0 and row[63] == 1.0 + 63.0 / 64.0 and row[192] == 12.0


def test_geolocation_is_the_tie_point_blend_of_the_other_restatements():
    """raster_from_grid on the tie points' latitude and (continuous) longitude equals, bit for bit, the per-pixel geolocation
    of xsw_ancillary_model's steps 1-2: tests/ancillary_model_ref.py forms it inside `core`; tests/grid_ref.py (`geolocate`,
    on ancillary_model_ref's bracket) is the same expression, returned."""
    tl, ts, lon, lat, heading = gc.ties()
    tp = TiePoints(tl, ts, lon, lat, heading)
    line, sample = np.arange(float(gc.L)), np.arange(float(gc.S))
    lf, lt = gref.bracket(tl, line)
    sf, st = gref.bracket(ts, sample)
    plon, plat, _, _ = gref.geolocate(tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading, lf, lt, sf, st)
    assert cref.same_bits(cref.raster_from_grid((tl, ts, tp.latitude), line, sample, np.float64), plat)
    assert cref.same_bits(cref.raster_from_grid((tl, ts, tp.longitude), line, sample, np.float64), plon)
    assert plat.std() > 0.05


# ------------------------------------------------------------------------------------------------------------ fill and valid
def test_fill_and_valid_rules():
    dn = np.array([[0, 1, 7, 50, 65535]], np.uint16)
    lut, noise = flat(2.0, (0.0,), (0.0, 4.0)), flat(25.0, (0.0,), (0.0, 4.0))
    inc = (np.array([0.0]), np.array([0.0, 4.0]), np.array([[20.0, 40.0]]))
    got = cref.calibrate(dn, lut, noise_range=noise, incidence=inc, dtype=np.float64)
    assert np.isnan(got["sigma0"][0, 0]) and np.array_equal(got["sigma0"][0, 1:], [-6.0, 6.0, 618.75, (65535.0 ** 2 - 25.0) / 4.0])
    assert np.array_equal(got["valid"], [[0, 0, 1, 1, 1]]) and got["valid"].dtype == np.uint8
    assert np.array_equal(got["nesz"], np.full((1, 5), 6.25)) and np.array_equal(got["incidence"], [[20.0, 25.0, 30.0, 35.0, 40.0]])
    other = cref.calibrate(dn, lut, noise_range=noise, fill=7, dtype=np.float64)   # another fill value: 0 is a number again
    assert other["sigma0"][0, 0] == -6.25 and np.isnan(other["sigma0"][0, 2]) and np.array_equal(other["valid"], [[0, 0, 0, 1, 1]])
    off = cref.calibrate(dn, lut, noise_range=noise, fill=None, dtype=np.float64)
    assert not np.isnan(off["sigma0"]).any() and np.array_equal(off["valid"], [[0, 0, 1, 1, 1]]) and off["incidence"] is None
    f32 = cref.calibrate(np.array([[0.0, np.nan, 0.5, 16777216.0]], np.float32), flat(1.0, (0.0,), (0.0, 3.0)), fill=0.5, dtype=np.float64)
    assert np.array_equal(np.isnan(f32["sigma0"]), [[False, True, True, False]]) and np.array_equal(f32["valid"], [[0, 0, 0, 1]])
    assert f32["sigma0"][0, 3] == 2.0 ** 48


def test_scenes_hold_what_they_are_there_for():
    for name in cc.SCENES:
        dn = cc.digital_numbers(name)                        # (asserts the properties)
        assert dn.shape == (cc.L, cc.SAMPLES[name]) and dn.dtype == (np.float32 if name == "f32" else np.uint16)
        full, bare = cc.case(name), cc.case(name, ())
        assert full["incidence"] is not None and bare["incidence"] is None and not (bare["nesz"] != 0).any()
        assert not cref.same_bits(full["sigma0"], bare["sigma0"])
    assert len(set(cc.COMBOS)) == 8 and () in cc.COMBOS and cc.TABLES in cc.COMBOS
    assert cref.same_bits(cc.case("vec")["sigma0"], cc.case("f32")["sigma0"])     # uint16 and float32 numbers of one value


# -------------------------------------------------------------------------------------------------------- the public calls' host checks
@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the checks must have refused the call before."""
    def touched(*a, **k):
        raise AssertionError("a device call was reached before the host checks refused the arguments")
    monkeypatch.setattr(calibrate, "_Call", touched)
    monkeypatch.setattr(_lib, "default_context", touched)


def grid(value=500.0, line=(0.0, 22.0), sample=(0.0, 30.0)):
    return AnnotationGrid(*flat(value, line, sample))


DN = np.ones((23, 31), np.uint16)


def test_annotation_grids_are_checked():
    for bad in (([0.0, 0.0], [0.0, 1.0]), ([1.0, 0.0], [0.0, 1.0]), ([0.0, 1.0], [0.0, 2.0, 1.0])):
        with pytest.raises(ValueError, match="ascending"):
            AnnotationGrid(bad[0], bad[1], np.ones((len(bad[0]), len(bad[1]))))
    with pytest.raises(ValueError, match=r"\[line, sample\]"):
        AnnotationGrid([0.0, 1.0], [0.0, 1.0, 2.0], np.ones((3, 2)))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="NaN or an infinity"):
            AnnotationGrid([0.0, 1.0], [0.0, 1.0], np.array([[1.0, bad], [1.0, 1.0]]))
    with pytest.raises(ValueError, match="NaN"):
        AnnotationGrid([0.0, np.nan], [0.0, 1.0], np.ones((2, 2)))
    with pytest.raises(ValueError, match="non-empty"):
        AnnotationGrid([], [0.0, 1.0], np.ones((0, 2)))
    g = AnnotationGrid([-3], [5], [[2]])                       # one node each, integers widened
    assert g.shape == (1, 1) and g.values.dtype == np.float64 and g.line.dtype == np.float64

    class Labelled:
        def __init__(self, values):
            self.values = np.asarray(values)
    g = AnnotationGrid(Labelled([0.0, 4.0]), Labelled([0.0, 2.0]), Labelled([[1.0, 2.0], [3.0, 4.0]]))
    assert g.values[1, 0] == 3.0


def test_digital_numbers_tables_and_options_are_checked(no_device):
    for bad in (DN.astype(np.int16), DN.astype(np.int32), DN.astype(np.float64), DN.astype(np.uint8), DN.astype(bool)):
        with pytest.raises(TypeError, match="uint16 or float32"):
            calibrate_dn(bad, grid())
    for bad in (DN[0], DN[None]):
        with pytest.raises(ValueError, match=r"\[L, S\]"):
            calibrate_dn(bad, grid())
    for bad in (None, flat(500.0), np.ones((2, 2))):
        with pytest.raises(TypeError, match="AnnotationGrid"):
            calibrate_dn(DN, bad)
    for key in ("noise_range", "noise_azimuth", "incidence"):
        with pytest.raises(TypeError, match="AnnotationGrid"):
            calibrate_dn(DN, grid(), **{key: flat(1.0)})
    for bad in (0.0, -2.0):
        with pytest.raises(ValueError, match="positive"):
            calibrate_dn(DN, grid(bad))
    for key in ("noise_range", "noise_azimuth"):
        with pytest.raises(ValueError, match="negative"):
            calibrate_dn(DN, grid(), **{key: grid(-1.0)})
    for bad in ("float16", np.int32, "complex64", "nothing"):
        with pytest.raises(ValueError, match="float32 or float64"):
            calibrate_dn(DN, grid(), dtype=bad)
    for bad in (65536, -1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="whole number"):
            calibrate_dn(DN, grid(), fill=bad)
    for bad in ("0", [0], True, 1j):
        with pytest.raises(TypeError, match="fill"):
            calibrate_dn(DN, grid(), fill=bad)
    with pytest.raises(ValueError, match="GPU"):
        calibrate_dn(DN, grid(), device="cpu")


def test_spans_and_coordinates_are_checked(no_device):
    short = dict(line=(0.0, 21.0)), dict(sample=(1.0, 30.0)), dict(sample=(0.0, 29.5))
    for kw in short:
        for key in ("sigma0_lut", "noise_range", "noise_azimuth", "incidence"):
            args = {"sigma0_lut": grid(), key: grid(**kw)}
            with pytest.raises(ValueError, match="extrapolated"):
                calibrate_dn(DN, args.pop("sigma0_lut"), **args)
    for key, bad in (("line", np.arange(23.0) + 1.0), ("sample", np.arange(31.0) - 2.0)):
        with pytest.raises(ValueError, match="extrapolated"):
            calibrate_dn(DN, grid(), **{key: bad})
    for key, bad in (("line", np.arange(22.0)), ("sample", np.arange(32.0)), ("line", np.arange(23.0)[None])):
        with pytest.raises(ValueError, match="do not match"):
            calibrate_dn(DN, grid(), **{key: bad})
    with pytest.raises(ValueError, match="NaN"):
        calibrate_dn(DN, grid(), line=np.where(np.arange(23) == 4, np.nan, np.arange(23.0)))


def test_raster_from_grid_is_checked(no_device):
    g = grid()
    for kw in (dict(), dict(shape=(23, 31), line=np.arange(23), sample=np.arange(31)), dict(shape=(23, 31), line=np.arange(23))):
        with pytest.raises(ValueError, match="exactly one"):
            raster_from_grid(g, **kw)
    for kw in (dict(line=np.arange(23)), dict(sample=np.arange(31))):
        with pytest.raises(ValueError, match="go together"):
            raster_from_grid(g, **kw)
    for bad in ((23,), (23, 31, 2), (-1, 31)):
        with pytest.raises(ValueError, match=r"\(L, S\)"):
            raster_from_grid(g, shape=bad)
    for kw in (dict(shape=(24, 31)), dict(shape=(23, 32)), dict(line=[-0.5, 3.0], sample=[0.0])):
        with pytest.raises(ValueError, match="extrapolated"):
            raster_from_grid(g, **kw)
    with pytest.raises(TypeError, match="AnnotationGrid"):
        raster_from_grid(flat(1.0), shape=(2, 2))
    with pytest.raises(ValueError, match="float32 or float64"):
        raster_from_grid(g, shape=(23, 31), dtype="float16")
    with pytest.raises(ValueError, match="GPU"):
        raster_from_grid(g, shape=(23, 31), device="cpu")


def test_good_arguments_reach_the_device(monkeypatch):
    reached = []

    def device(*arrays):
        reached.append(arrays)
        raise RuntimeError("the device")
    monkeypatch.setattr(calibrate, "_Call", device)
    calls = (lambda: calibrate_dn(DN, grid()),
             lambda: calibrate_dn(DN.astype(np.float32), grid(), noise_range=grid(3.0), noise_azimuth=grid(0.0), incidence=grid(30.0), fill=None,
                                  dtype=np.float64, nesz=False, valid=True),
             lambda: calibrate_dn(DN, grid(line=(-5.0, 40.0), sample=(-1.0, 31.0)), fill=65535, line=np.arange(23) + 2.5, sample=np.arange(31.0)),
             lambda: raster_from_grid(grid(), shape=(23, 31)),
             lambda: raster_from_grid(grid(), line=[0.0, 0.5, 22.0], sample=[30.0], dtype="float64"))
    for call in calls:
        with pytest.raises(RuntimeError, match="the device"):
            call()
    assert len(reached) == len(calls)


# --------------------------------------------------------------------------------------------------------------- declarations
def test_public_names_and_the_result_container():
    import xsarsea_amd
    assert xsarsea_amd.calibrate is calibrate and xsarsea_amd.calibrate_dn is calibrate.calibrate_dn
    assert {"calibrate", "AnnotationGrid", "Calibrated", "calibrate_dn", "raster_from_grid"} <= set(xsarsea_amd.__all__)
    assert {"AnnotationGrid", "Calibrated", "calibrate_dn", "raster_from_grid"} <= set(calibrate.__all__)
    c = Calibrated(1, None, 3, None)
    assert (c.sigma0, c["nesz"], c["incidence"], c.valid) == (1, None, 3, None)
    assert "jump" in AnnotationGrid.__doc__


def test_header_declares_the_entry_and_the_binding_matches():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+xsw_calibrate\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/xsw.h does not declare xsw_calibrate"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[0].startswith("xsw_ctx") and len(params) == 17 and sum(p.startswith("const xsw_table *") for p in params) == 4
    assert params[-1].startswith("uint8_t *")
    fields = re.search(r"typedef\s+struct\s+xsw_table\s*\{(.*?)\}\s*xsw_table\s*;", txt, flags=re.S).group(1)
    names = re.findall(r"\*?\s*(\w+)\s*[,;]", fields)
    assert names == [n for n, _ in _lib.Table._fields_] == ["n_lines", "n_samples", "values", "line_first", "line_t", "sample_first", "sample_t"]
    assert ctypes.sizeof(_lib.Table) == 2 * 4 + 5 * 8
    assert re.search(r"XSW_DN_U16\s*=\s*0\s*,\s*XSW_DN_F32\s*=\s*1", txt) and (_lib.DN_U16, _lib.DN_F32) == (0, 1)
    assert "xsw_calibrate" in _lib.EXPORTS and hasattr(_lib.Context, "calibrate_raw")
    lib = _lib.load()
    assert hasattr(lib, "xsw_calibrate") and len(lib.xsw_calibrate.argtypes) == 17
    assert int(re.search(r"#\s*define\s+XSW_VERSION\s+(\d+)", txt).group(1)) == 4 == _lib.ABI_VERSION


def test_the_unit_is_built_and_the_kernel_uses_no_scratch():
    from xsarsea_amd import _build
    assert os.path.basename(_build.SRC_CALIBRATE) == "xsw_calibrate.hip" and os.path.exists(_build.SRC_CALIBRATE)
    rows = [r for r in _build.kernel_resources() if "k_calibrate" in r["kernel"]]
    assert len(rows) >= 9
    for r in rows:
        assert r["scratch_bytes"] == 0 and r["lds_bytes"] == 0, r
    # uint16 -> float32 on the vector path: sigma0 alone, and with one further table, run at four waves per SIMD or more
    # (the names are demangled where the toolchain has a demangler, mangled where it has none)
    lean = [r for r in rows if re.search(r"k_calibrate<unsigned short, float, true, (1|3|5|9)>|k_calibrateItfLb1ELi(1|3|5|9)E", r["kernel"])]
    assert len(lean) == 4 and all(r["waves_per_simd_by_vgpr"] >= 4 for r in lean), lean


# --------------------------------------------------------------------------------------------------------------------- launch
def test_the_stated_launch_is_strip_grid_with_the_kernels_constants(ask):  # noqa: F811
    min_lines, in_flight = source_define("XSW_CAL_MIN_LINES"), source_define("XSW_CAL_LINES")
    assert (min_lines, in_flight) == (32, 4)
    shapes = [(cc.L, s) for s in sorted(set(cc.SAMPLES.values()))] + [(1, 1), (31, 4), (33, 1025), (4097, 1024), (20000, 20000), (60, 260)]
    for (lines, samples), (gx, gy, rows) in zip(shapes, ask(*[("grid", lines, -(-samples // 4), 0) for lines, samples in shapes])):
        lpb = max(rows, min_lines)
        strips = -(-lines // lpb)
        assert cc.launch(lines, samples) == (gx, strips, lpb, lines - (strips - 1) * lpb), (lines, samples)
        assert gx == -(-samples // 1024) and strips <= gy and strips <= 65535
    assert cc.launch(cc.L, 2100) == (3, 3, 32, 11) and cc.launch(cc.L, 2099) == (3, 3, 32, 11)
    assert cc.launch(20000, 20000)[2] > min_lines      # the measured size: strip_grid's own strip length
