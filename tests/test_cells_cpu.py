"""CPU: the restatement of xsarsea_amd.cells (tests/cells_ref.py) against exact and extended-precision references and on
hand-checkable cells, the public calls' host checks (which all precede the first device call), and the round trip
model wind -> a-priori raster -> cells -> (u, v) on the restatements alone."""
import math
import os
import re

import numpy as np
import pytest

import ancillary_model_ref as aref
import cells_ref as cref
from conftest import REPO
from xsarsea_amd import TiePoints, _lib, cells
from xsarsea_amd.windspeed.crosspol import CopolCodes

U = 2.0 ** -53

# Round trip model (u, v) -> ancillary_model_ref -> cells_ref -> (u, v), one heading, a constant field (`round_trip`): the
# largest |float64 chain - longdouble chain| over both components and every cell measured here is 1.78e-15 m/s (a wind of
# 13.6 m/s: 1.2 units of 2**-53 |wind|); the bound is 4 x that.  test_gpu_cells.py holds the device chain to the same constant.
ROUND_TRIP_MEASURED = 1.78e-15
ROUND_TRIP_BOUND = 4 * ROUND_TRIP_MEASURED


# --------------------------------------------------------------------------------------------------------------- the sums
@pytest.mark.parametrize("n", [1, 2, 9, 63, 64, 65, 130, 255, 256, 257, 527, 1480, 10000])
def test_ordered_sum_is_within_the_bound_of_any_order(n):
    """|sum - exact| <= (N - 1) 2**-53 sum|x| holds for any order of N - 1 additions (each rounds within 2**-53 of a partial sum
    that is at most sum|x|, to first order); math.fsum is exact."""
    rng = np.random.default_rng(n)
    for x in (rng.normal(0, 10, n), rng.uniform(5, 11, n), rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)):
        got, exact = cref.ordered_sum(x), math.fsum(x)
        bound = (n - 1) * U * math.fsum(np.abs(x))
        assert abs(got - exact) <= bound
        assert cref._sum_rows(x[None, :])[0] == got  # the batched form


def test_batched_sums_equal_the_literal_order_bit_for_bit():
    """cells_ref._sum_rows leaves out the folds that add only padding; cell_sums gathers the cells of a raster: both must equal
    the literal 256-accumulator statement on every cell, clipped ones included."""
    rng = np.random.default_rng(1)
    for n in list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 777]:
        v = rng.normal(0, 3, (3, n))
        v[1, ::3] = 0.0
        v[2] = -np.abs(v[2])
        want = np.array([cref.ordered_sum(r) for r in v])
        assert np.array_equal(cref._sum_rows(v).view(np.uint64), want.view(np.uint64)), n
    x = rng.normal(0, 3, (23, 31))
    for cell in ((3, 3), (5, 7), (23, 31), (40, 40), (1, 1), (4, 31), (23, 2)):
        got = cref.cell_sums(x, cell)
        nl, ns = -(-23 // cell[0]), -(-31 // cell[1])
        assert got.shape == (nl, ns)
        for i in range(nl):
            for j in range(ns):
                blk = x[i * cell[0]:(i + 1) * cell[0], j * cell[1]:(j + 1) * cell[1]]
                assert got[i, j] == cref.ordered_sum(blk.ravel()), (cell, i, j)  # p = r * w + c with the clipped width


def speeds(rng, shape):
    """Winds of 8 +- 3 m/s from every direction."""
    return rng.normal(8.0, 3.0, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))


@pytest.mark.parametrize("cell", [(3, 3), (10, 13), (40, 37), (100, 100)])
def test_means_and_std_against_extended_precision(cell):
    """Sums against math.fsum within (N - 1) 2**-53 sum|x| (N the cell's pixels).  std against the two-pass value in longdouble:
    var = (Sq - Ss**2 / n) / (n - 1) subtracts two numbers of size Sq that were each summed over N pixels, so its error is led
    by the cancellation term N 2**-53 Sq / (n - 1); the roundings of q, s and of the last operations add a few units more in
    the worst case (3 N + 7 in all), but random roundings stay far below, and the test holds var to the cancellation term alone."""
    rng = np.random.default_rng(cell[0])
    L, S = 2 * cell[0] + 1, 2 * cell[1] + 3
    w = speeds(rng, (L, S))
    w[rng.uniform(size=w.shape) < 0.1] = np.nan
    got = cref.wind(w, cell)
    worst = 0.0
    for i in range(got["count"].shape[0]):
        for j in range(got["count"].shape[1]):
            blk = w[i * cell[0]:(i + 1) * cell[0], j * cell[1]:(j + 1) * cell[1]].ravel()
            N, v = len(blk), blk[~np.isnan(blk.real)]
            n = len(v)
            assert got["count"][i, j] == n
            s = np.abs(v)
            for part, x in (("real", v.real), ("imag", v.imag)):
                assert abs(getattr(got["wind"][i, j], part) * n - math.fsum(x)) <= ((N - 1) * U + 2 * U) * math.fsum(np.abs(x))  # + the division
            assert abs(got["wspd"][i, j] * n - math.fsum(s)) <= ((N - 1) * U + 5 * U) * math.fsum(s)  # + sqrt(q) (2), numpy's abs, the division, the product
            if n < 2:
                assert np.isnan(got["wspd_std"][i, j])
                continue
            ld = np.hypot(v.real.astype(np.longdouble), v.imag.astype(np.longdouble))
            var_ref = ((ld - ld.mean()) ** 2).sum() / (n - 1)
            std_ref = float(np.sqrt(var_ref))
            bound_var = N * U * float((ld * ld).sum()) / (n - 1)
            std = got["wspd_std"][i, j]
            assert 0.3 < std_ref < 8.0
            err = abs(std * std - float(var_ref))
            worst = max(worst, err / bound_var)
            assert err <= bound_var + 4 * U * float(var_ref)  # the rounding of sqrt and of its square
            assert abs(std - std_ref) <= bound_var / (2 * std_ref) * 1.01 + 2 * U * std_ref
    print(f"cell {cell}: largest |var - var_ref| = {worst:.3g} of N 2**-53 Sq / (n - 1)")


def test_real_raster_against_extended_precision():
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        x = rng.uniform(0.01, 0.3, (45, 50)).astype(dtype)
        x[rng.uniform(size=x.shape) < 0.05] = np.nan
        keep = rng.uniform(size=x.shape) < 0.9
        got = cref.real(x, (10, 13), keep)
        for i in range(5):
            for j in range(4):
                blk, k = x[i * 10:(i + 1) * 10, j * 13:(j + 1) * 13].ravel().astype(np.float64), keep[i * 10:(i + 1) * 10, j * 13:(j + 1) * 13].ravel()
                v = blk[k & ~np.isnan(blk)]
                N, n = len(blk), len(v)
                assert got["count"][i, j] == n
                assert abs(got["mean"][i, j] * n - math.fsum(v)) <= (N + 1) * U * math.fsum(np.abs(v))
                ld = v.astype(np.longdouble)
                var_ref = float(((ld - ld.mean()) ** 2).sum() / (n - 1))
                assert abs(got["std"][i, j] ** 2 - var_ref) <= N * U * float((ld * ld).sum()) / (n - 1) + 4 * U * var_ref


def test_hand_checkable_cells():
    w = np.full((4, 10), 3.0 + 4.0j)
    w[:, 5:] = np.where(np.arange(4)[:, None] % 2 == 0, 3.0 + 4.0j, -3.0 - 4.0j)   # cell 1: two opposite winds, half each
    r = cref.wind(w, (4, 5))
    assert r["count"].tolist() == [[20, 20]]
    assert r["wind"][0, 0] == 3.0 + 4.0j and r["wspd"][0, 0] == 5.0 and r["wspd_std"][0, 0] == 0.0 and r["steadiness"][0, 0] == 1.0
    assert r["wind"][0, 1] == 0.0 and r["wspd"][0, 1] == 5.0 and r["wspd_std"][0, 1] == 0.0 and r["steadiness"][0, 1] == 0.0
    # n = 0 and n = 1; the three kinds of invalid pixel; keep
    w = np.full((2, 6), 1.0 - 2.0j)
    w[:, :2] = [[np.nan + 0j, complex(np.nan, np.nan)], [complex(1.0, np.nan), np.nan]]
    w[0, 3] = w[1, 2] = w[1, 3] = np.nan
    keep = np.ones((2, 6), np.uint8)
    keep[:, 4:] = 0
    r = cref.wind(w, (2, 2), keep)
    assert r["count"].tolist() == [[0, 1, 0]]
    for name in ("wspd", "wspd_std", "steadiness"):
        assert np.isnan(r[name][0, 0]) and np.isnan(r[name][0, 2])
    assert np.isnan(r["wind"].real[0, [0, 2]]).all() and np.isnan(r["wind"].imag[0, [0, 2]]).all()
    assert r["wind"][0, 1] == 1.0 - 2.0j and r["wspd"][0, 1] == np.sqrt(5.0) and np.isnan(r["wspd_std"][0, 1]) and r["steadiness"][0, 1] == 1.0
    calm = cref.wind(np.zeros((2, 2), np.complex128), (2, 2))
    assert calm["wspd"][0, 0] == 0.0 and np.isnan(calm["steadiness"][0, 0]) and calm["wspd_std"][0, 0] == 0.0
    x = np.array([[1.0, 2.0, 3.0, np.nan], [4.0, 5.0, 6.0, np.nan]])
    r = cref.real(x, (2, 3))
    assert r["count"].tolist() == [[6, 0]] and r["mean"][0, 0] == 3.5 and r["std"][0, 0] == np.sqrt(3.5) and np.isnan(r["mean"][0, 1]) and np.isnan(r["std"][0, 1])
    np.testing.assert_array_equal(cref.centres(np.arange(10.0), 4), [1.5, 5.5, 8.5])
    np.testing.assert_array_equal(cells._centres(None, 10, 4, "line"), [1.5, 5.5, 8.5])
    np.testing.assert_array_equal(cells._centres(10.0 * np.arange(7), 7, 7, "line"), [30.0])


def test_east_and_north_components_undo_the_ancillary_rotation():
    """Heading 0: the line axis points north, the sample axis east; a wind blowing to the east is -speed in antenna convention."""
    z = np.zeros((1, 1))
    for w, want in ((-5.0 + 0j, (5.0, 0.0)), (-5.0j, (0.0, 5.0)), (3.0 + 4.0j, (-3.0, -4.0))):
        g = cref.geo(np.full((1, 1), w), [0.0], [0.0], z + 10.0, z + 50.0, z, [0.0], [0.0])
        assert (g["u"][0, 0], g["v"][0, 0]) == want and g["longitude"][0, 0] == 10.0 and g["latitude"][0, 0] == 50.0
    g = cref.geo_core(np.full((1, 1), 1.0 + 0j), np.zeros((1, 2)), np.zeros((1, 2)), np.array([[1.0, -1.0]]), np.zeros((1, 2)), [0], [0.0], [0], [0.5])
    assert np.isnan(g["u"][0, 0]) and np.isnan(g["v"][0, 0])  # cancelling headings


# ---------------------------------------------------------------------------------------------------------------- round trip
def round_trip_scene():
    rng = np.random.default_rng(21)
    L, S = 60, 90
    tl, ts = np.array([0.0, 25.0, L - 1.0]), np.array([0.0, 30.0, 61.0, S - 1.0])
    fl, fs = tl[:, None] / (L - 1), ts[None, :] / (S - 1)
    glon = 11.0 + 5.5 * fs + 0.4 * fl
    glat = 2.5 - 4.0 * fl + 0.3 * fs
    heading = np.full((3, 4), -167.25)
    u0, v0 = 9.75, -9.5
    return dict(L=L, S=S, tl=tl, ts=ts, glon=glon, glat=glat, heading=heading, u0=u0, v0=v0, mlon=10.0 + np.arange(9), mlat=-3.0 + np.arange(7),
                u=np.full((7, 9), u0), v=np.full((7, 9), v0), cell=(13, 20))


def round_trip_longdouble(sc):
    """The chain of `round_trip` with every operation in longdouble and plain sums: blend, rotation, cell mean, blend, rotation back."""
    ld = np.longdouble
    tl, ts = sc["tl"].astype(ld), sc["ts"].astype(ld)
    h = np.deg2rad(sc["heading"].astype(ld))
    grids = [sc["glon"].astype(ld), sc["glat"].astype(ld), np.cos(h), np.sin(h)]

    def blend(line, sample):
        i0 = np.clip(np.searchsorted(sc["tl"], line, side="right") - 1, 0, len(tl) - 2)
        j0 = np.clip(np.searchsorted(sc["ts"], sample, side="right") - 1, 0, len(ts) - 2)
        wl = ((line.astype(ld) - tl[i0]) / (tl[i0 + 1] - tl[i0]))[:, None]
        ws = ((sample.astype(ld) - ts[j0]) / (ts[j0 + 1] - ts[j0]))[None, :]
        f = lambda g: (1 - wl) * ((1 - ws) * g[i0][:, j0] + ws * g[i0][:, j0 + 1]) + wl * ((1 - ws) * g[i0 + 1][:, j0] + ws * g[i0 + 1][:, j0 + 1])
        lon, lat, c, s = (f(g) for g in grids)
        nh = np.sqrt(c * c + s * s)
        return lon, lat, c / nh, s / nh

    lon, lat, ch, sh = blend(np.arange(float(sc["L"])), np.arange(float(sc["S"])))
    x, y = (lon - ld(sc["mlon"][0])) / ld(1.0), (lat - ld(sc["mlat"][0])) / ld(1.0)
    tx, ty = x - np.floor(x), y - np.floor(y)
    node = lambda g0: (1 - ty) * ((1 - tx) * ld(g0) + tx * ld(g0)) + ty * ((1 - tx) * ld(g0) + tx * ld(g0))
    uu, vv = node(sc["u0"]), node(sc["v0"])
    re, im = -(uu * ch - vv * sh), -(uu * sh + vv * ch)
    cl, cs = sc["cell"]
    cline, csample = cref.centres(np.arange(float(sc["L"])), cl), cref.centres(np.arange(float(sc["S"])), cs)
    mean = lambda a: np.array([[a[i:i + cl, j:j + cs].sum() / ld(a[i:i + cl, j:j + cs].size) for j in range(0, sc["S"], cs)] for i in range(0, sc["L"], cl)])
    mre, mim = mean(re), mean(im)
    _, _, ch, sh = blend(cline, csample)
    return -(mre * ch + mim * sh), -(mim * ch - mre * sh)


def round_trip(sc):
    """(u, v) per cell from the two restatements in float64."""
    line, sample = np.arange(float(sc["L"])), np.arange(float(sc["S"]))
    raster = aref.ancillary_from_model(sc["u"], sc["v"], sc["mlon"], sc["mlat"], sc["tl"], sc["ts"], sc["glon"], sc["glat"], sc["heading"], line, sample)
    assert not np.isnan(raster.real).any()
    r = cref.wind(raster, sc["cell"])
    g = cref.geo(r["wind"], sc["tl"], sc["ts"], sc["glon"], sc["glat"], sc["heading"], cref.centres(line, sc["cell"][0]), cref.centres(sample, sc["cell"][1]))
    return g["u"], g["v"]


def test_round_trip_returns_the_models_components():
    sc = round_trip_scene()
    u, v = round_trip(sc)
    ul, vl = round_trip_longdouble(sc)
    assert u.shape == (5, 5)
    dev = max(float(np.abs(u - ul).max()), float(np.abs(v - vl).max()))
    print(f"largest |float64 chain - longdouble chain| = {dev:.3g} m/s (measured {ROUND_TRIP_MEASURED:g}, bound {ROUND_TRIP_BOUND:g})")
    assert float(np.abs(ul - sc["u0"]).max()) < 1e-17 and float(np.abs(vl - sc["v0"]).max()) < 1e-17  # the chain in longdouble is the identity
    assert dev <= ROUND_TRIP_BOUND
    assert np.abs(u - sc["u0"]).max() <= ROUND_TRIP_BOUND and np.abs(v - sc["v0"]).max() <= ROUND_TRIP_BOUND


# ---------------------------------------------------------------------------------------------- the public calls' host checks
@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the checks must have refused the call before."""
    def touched(*a, **k):
        raise AssertionError("a device call was reached before the host checks refused the arguments")
    monkeypatch.setattr(cells, "_Call", touched)
    monkeypatch.setattr(_lib, "default_context", touched)


def tie_points():
    tl, ts = np.array([0.0, 7.0, 22.0]), np.array([0.0, 4.0, 19.0, 30.0])
    return TiePoints(tl, ts, 10.0 + 0.1 * ts[None, :] + 0 * tl[:, None], 3.0 - 0.1 * tl[:, None] + 0 * ts[None, :], np.full((3, 4), 12.0))


def test_cell_entries_are_checked(no_device):
    w, x = np.ones((23, 31), np.complex128), np.ones((23, 31))
    codes = CopolCodes(x, np.zeros((23, 31), np.uint32), None)
    for call in (lambda c: cells.wind_cells(w, c), lambda c: cells.raster_cells(x, c), lambda c: codes.cells(c)):
        for bad in ((0, 3), (3, -1), (3,), (1, 2, 3), 5, (2 ** 31, 1)):
            with pytest.raises(ValueError):
                call(bad)
        for bad in ((2.5, 3), (3, "a"), (np.float64(2.0), 3)):
            with pytest.raises(TypeError, match="integers"):
                call(bad)


def test_rank_and_dtype_are_checked(no_device):
    w = np.ones((23, 31), np.complex128)
    for bad in (w[0], w[None]):
        with pytest.raises(ValueError, match="2-D"):
            cells.wind_cells(bad, (3, 3))
        with pytest.raises(ValueError, match="2-D"):
            cells.raster_cells(bad.real, (3, 3))
    for bad in (w.real, w.astype(np.complex64).real, np.ones((23, 31), np.int32)):
        with pytest.raises(TypeError, match="complex128 or complex64"):
            cells.wind_cells(bad, (3, 3))
    for bad in (w, np.ones((23, 31), np.float16), np.ones((23, 31), np.int64)):
        with pytest.raises(TypeError, match="float32 or float64"):
            cells.raster_cells(bad, (3, 3))
    with pytest.raises(TypeError, match="uint32 or int32"):
        CopolCodes(w.real, np.zeros((23, 31), np.int64), None).cells((3, 3))
    with pytest.raises(ValueError, match="2-D"):
        CopolCodes(w.real[0], np.zeros(31, np.uint32), None).cells((3, 3))


def test_keep_is_checked(no_device):
    w = np.ones((23, 31), np.complex128)
    for call in (lambda **k: cells.wind_cells(w, (3, 3), **k), lambda **k: cells.raster_cells(w.real, (3, 3), **k),
                 lambda **k: CopolCodes(w.real, np.zeros((23, 31), np.uint32), None).cells((3, 3), **k)):
        with pytest.raises(ValueError, match="shape"):
            call(keep=np.ones((23, 30), bool))
        with pytest.raises(ValueError, match="shape"):
            call(keep=np.ones(23 * 31, np.uint8))
        for bad in (np.ones((23, 31)), np.ones((23, 31), np.int32)):
            with pytest.raises(TypeError, match="bool or uint8"):
                call(keep=bad)


def test_tie_points_and_coordinates_are_checked(no_device):
    w = np.ones((23, 31), np.complex128)
    tp = tie_points()
    with pytest.raises(TypeError, match="TiePoints"):
        cells.wind_cells(w, (3, 3), tie_points=(tp.line, tp.sample))
    for key, bad in (("line", np.arange(23.0) + 1.0), ("sample", np.arange(31.0) - 2.0)):
        with pytest.raises(ValueError, match="extrapolated"):
            cells.wind_cells(w, (3, 3), tie_points=tp, **{key: bad})   # a centre leaves the tie span
    with pytest.raises(ValueError, match="extrapolated"):
        cells.wind_cells(np.ones((25, 31), np.complex128), (1, 3), tie_points=tp)
    for key, bad in (("line", np.arange(22.0)), ("sample", np.arange(32.0)), ("line", np.arange(23.0)[None])):
        with pytest.raises(ValueError, match="do not match"):
            cells.wind_cells(w, (3, 3), **{key: bad})
        with pytest.raises(ValueError, match="do not match"):
            cells.raster_cells(w.real, (3, 3), **{key: bad})
    with pytest.raises(ValueError, match="NaN"):
        cells.wind_cells(w, (3, 3), line=np.where(np.arange(23) == 4, np.nan, np.arange(23.0)))
    one = TiePoints([4.0], tp.sample, tp.longitude[:1], tp.latitude[:1], tp.ground_heading[:1])  # a single tie line: one cell row only
    with pytest.raises(ValueError):
        cells.wind_cells(w, (12, 3), tie_points=one, line=np.full(23, 4.0))


def test_checks_pass_the_centres_not_the_pixels(monkeypatch):
    """A raster whose outer pixels leave the tie span while every cell centre is inside gets as far as the device."""
    reached = []

    def device(*arrays):
        reached.append(arrays)
        raise RuntimeError("the device")
    monkeypatch.setattr(cells, "_Call", device)
    with pytest.raises(RuntimeError, match="the device"):
        cells.wind_cells(np.ones((23, 31), np.complex128), (3, 3), tie_points=tie_points(), line=np.arange(23.0) - 0.5, sample=np.arange(31.0) - 0.5)
    assert len(reached) == 1


def test_public_names():
    import xsarsea_amd
    assert xsarsea_amd.wind_cells is cells.wind_cells and xsarsea_amd.raster_cells is cells.raster_cells
    assert xsarsea_amd.WindCells is cells.WindCells and xsarsea_amd.RasterCells is cells.RasterCells
    assert {"cells", "wind_cells", "raster_cells", "WindCells", "RasterCells"} <= set(xsarsea_amd.__all__)
    assert callable(CopolCodes.cells)
    r = cells.WindCells(*range(7))
    assert r.direction is None and r["wspd"] == 2
    east = cells.WindCells(*range(7), u=np.array([5.0, 0.0, -3.0]), v=np.array([0.0, 5.0, 0.0]))
    np.testing.assert_allclose(east.direction, [270.0, 180.0, 90.0])  # blowing to the east: from the west


# ------------------------------------------------------------------------------------------------------------- header and library
@pytest.mark.parametrize("entry,count", [("xsw_wind_cells", 27), ("xsw_raster_cells", 11)])
def test_header_declares_the_entries_and_the_bindings_have_one_letter_per_argument(entry, count):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"include/xsw.h does not declare {entry}"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[0].startswith("xsw_ctx")
    sig = _lib.RASTER_ENTRIES[entry]
    assert len(sig) == len(params) - 1 == count
    for letter, p in zip(sig, params[1:]):
        want = "p" if "*" in p else {"int64_t": "l", "int32_t": "i", "double": "d"}[p.split()[0]]
        assert letter == want, p
    assert entry in _lib.EXPORTS and hasattr(_lib.Context, entry[len("xsw_"):] + "_raw")
    assert hasattr(_lib.load(), entry)
    assert (_lib.CELLS_C128, _lib.CELLS_C64, _lib.CELLS_CODES) == tuple(int(re.search(rf"XSW_CELLS_{k}\s*=\s*(\d+)", txt).group(1)) for k in ("C128", "C64", "CODES"))
