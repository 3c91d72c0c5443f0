"""CPU: xsarsea_amd.landmask without a device.  The restatement (tests/landmask_ref.py) against closed forms; every case of
tests/landmask_cases.py held to its property; the package's host plan against brute force, through a numpy emulation of the banded
kernel's walk and through the coverage property itself; `Coastline` parsing, the public call's refusals, the declarations and
the build."""
import os
import re

import numpy as np
import pytest

import landmask_cases as lc
import landmask_ref as lref
from conftest import REPO
from xsarsea_amd import Coastline, TiePoints, _build, _lib, land_mask, landmask

CHUNK = 1024  # xsw_land_chunk_edges(): asserted below


def all_cases():
    return list(lc.small_cases(CHUNK).values())


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv("XSW_LAND_BANDS", raising=False)
    monkeypatch.delenv("XSW_LAND_PATH", raising=False)


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_against_closed_forms():
    # a unit square and the pixels on and around it, by hand
    e = lref.edges_of([lc.box(0.0, 0.0, 1.0, 1.0)])
    px, py = np.meshgrid([-0.5, 0.0, 0.5, 1.0, 1.5], [-0.5, 0.0, 0.5, 1.0, 1.5])
    want = np.zeros((5, 5), bool)
    want[1:3, 1:3] = True  # half-open: the southern and western sides belong, the northern and eastern do not
    assert np.array_equal(lref.land(px, py, e), want)
    # a triangle of area 5.5 in a box of area 30: strictly inside / outside by the sign of three cross products, away from its sides
    tri = np.array([[0.0, 0.0], [4.0, 1.0], [1.0, 3.0]])
    rng = np.random.default_rng(0)
    px, py = rng.uniform(-1, 5, 4000), rng.uniform(-1, 4, 4000)
    cross = [(b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0]) for a, b in zip(tri, np.roll(tri, -1, axis=0))]
    inside = (cross[0] > 0) & (cross[1] > 0) & (cross[2] > 0)
    assert 0.15 < inside.mean() < 0.22 and np.array_equal(lref.land(px, py, lref.edges_of([tri])), inside)
    # the ring's direction and a repeated closing vertex change nothing; a whole turn in the input neither
    for ring in (tri[::-1], np.concatenate([tri, tri[:1]]), tri + [360.0, 0.0]):
        ex = lref.turn_copies(lref.edges_of([ring]), px)
        assert np.array_equal(lref.land(px, py, ex), inside)
    case = lc.small_cases(CHUNK)["exact_hits"]
    assert np.array_equal(case.want(), lc.exact_expected()) and np.array_equal(lc.exact_expected(), lc.exact_expected_in_integers())
    px, py = case.positions()
    l, s = np.meshgrid(np.arange(lc.L), np.arange(lc.S), indexing="ij")
    assert np.array_equal(px, 8.0 + s / 64.0 + l / 256.0) and np.array_equal(py, 36.0 + l / 8.0)  # the blend is exact


def test_every_case_has_its_property():
    assert _lib.land_chunk_edges() == CHUNK
    arch = lc.small_cases(CHUNK)["archipelago"]
    p64 = landmask.plan(arch.coastline(), arch.tie_points(), n_bands=64)
    for case in all_cases():
        lc.check_case(case, CHUNK, plan_at_64=p64 if case.name == "archipelago" else None)
    for name, ring in lc.antimeridian().items():
        assert (ring.want() == 0).any(), name  # each ring alone puts land into the raster


def test_strip_case_geometry_and_land_shares():
    case = lc.strip_case()
    lc.check_strip_geometry(case)
    for rows in (lc.strip_rows(1), lc.strip_rows(-1)):
        px, py = case.positions(rows)
        assert 0.1 < lref.land(px, py, case.ref_edges(px)).mean() < 0.9
    px, py = case.positions(lc.strip_rows(0))
    both = lref.land(px, py, case.ref_edges(px))
    assert both[:, :1024].any() and both[:, 1024:].any() and not both[:, :1024].all()  # both workgroup columns hold land


# ---------------------------------------------------------------------------------------------------------------- the host plan
def emulate(plan, px, py):
    """The banded kernel's walk in numpy: a pixel meets the list of its own band only, in the list's order, and stops at the first
    edge with xmax < px."""
    band = plan.band_of(py)
    land = np.zeros(px.shape, bool)
    for b in np.unique(band):
        sel = band == b
        x, y = px[sel], py[sel]
        par, walking = np.zeros(x.shape, bool), np.ones(x.shape, bool)
        for e in plan.band_edges[plan.band_start[b]:plan.band_start[b + 1]]:
            x1, y1, x2, y2 = plan.edges[e]
            walking &= ~(max(x1, x2) < x)
            par ^= walking & lref.hits(x, y, x1, y1, x2, y2)
        land[sel] = par
    return land


def check_plan(case, plan, px, py, want_land):
    assert plan.band_start[0] == 0 and (np.diff(plan.band_start) >= 0).all() and plan.band_start[-1] == len(plan.band_edges)
    assert plan.band_start.dtype == np.int32 and plan.band_edges.dtype == np.int32 and plan.edges.dtype == np.float64
    assert not len(plan.band_edges) or (0 <= plan.band_edges.min() and plan.band_edges.max() < len(plan.edges))
    xmax = np.maximum(plan.edges[:, 0], plan.edges[:, 2])
    for b in range(plan.n_bands):
        assert (np.diff(xmax[plan.band_edges[plan.band_start[b]:plan.band_start[b + 1]]]) <= 0).all()
    assert np.array_equal(emulate(plan, px, py), want_land), (case.name, plan.n_bands)
    # coverage: every (pixel, edge) hit is in the list of the pixel's band and of both neighbouring bands
    listed = np.zeros((plan.n_bands, len(plan.edges)), bool)
    listed[np.repeat(np.arange(plan.n_bands), np.diff(plan.band_start)), plan.band_edges] = True
    band = plan.band_of(py)
    for e, (x1, y1, x2, y2) in enumerate(plan.edges):
        hit_bands = np.unique(band[lref.hits(px, py, x1, y1, x2, y2)])
        for b in hit_bands:
            assert listed[max(b - 1, 0):b + 2, e].all(), (case.name, plan.n_bands, e, b)


@pytest.mark.parametrize("n_bands", lc.BANDS + (None,))
def test_plan_walk_equals_brute_force(monkeypatch, n_bands):
    for case in all_cases():
        px, py = case.positions()
        plan = landmask.plan(case.coastline(), case.tie_points(), n_bands=n_bands)
        assert plan.n_bands == (n_bands or plan.n_bands) and 1 <= plan.n_bands <= landmask.MAX_BANDS
        check_plan(case, plan, px, py, case.want() == 0)
    # the strip: the second, the last and every 97th workgroup row's first line
    case = lc.strip_case()
    rows = np.unique(np.concatenate([lc.strip_rows(1), lc.strip_rows(-1), np.arange(0, lc.STRIP_SHAPE[0], 97 * lc.STRIP_GRID[2])]))
    px, py = case.positions(rows)
    check_plan(case, landmask.plan(case.coastline(), case.tie_points(), n_bands=n_bands), px, py, lref.land(px, py, case.ref_edges(px)))


def test_band_rule_and_the_forced_count(monkeypatch):
    arch = lc.small_cases(CHUNK)["archipelago"]
    coast, tp = arch.coastline(), arch.tie_points()
    p = landmask.plan(coast, tp)
    extent = p.span[3] - p.span[2]
    assert p.n_bands == min(max(-(-len(p.edges) // landmask.EDGES_PER_BAND), 1), int(extent / landmask.MIN_BAND_HEIGHT)) and p.n_bands > 64
    assert p.lat0 == p.span[2] and p.h == extent / p.n_bands and p.turns == [0]
    assert len(p.edges) < len(coast.edges)  # the box's southern and western sides are dropped
    monkeypatch.setenv("XSW_LAND_BANDS", "7")
    assert landmask.plan(coast, tp).n_bands == 7 and landmask.plan(coast, tp, n_bands=3).n_bands == 3
    for bad in ("0", "65537", "many", "-2"):
        monkeypatch.setenv("XSW_LAND_BANDS", bad)
        with pytest.raises(ValueError, match="XSW_LAND_BANDS"):
            landmask.plan(coast, tp)
    monkeypatch.delenv("XSW_LAND_BANDS")
    far = lc.small_cases(CHUNK)["north"]
    p = landmask.plan(far.coastline(), far.tie_points())
    assert len(p.edges) == 0 and p.n_bands == 1 and len(p.band_edges) == 0
    anti = lc.small_cases(CHUNK)["antimeridian"]
    p = landmask.plan(anti.coastline(), anti.tie_points())
    assert p.turns == [0, 1] and p.span[0] < 150.0 < 389.0 < p.span[1]
    one = lc.small_cases(CHUNK)["single_tie_line"]
    p = landmask.plan(one.coastline(), one.tie_points())
    assert p.h > 0 and np.isfinite(p.h)


# ---------------------------------------------------------------------------------------------------------------- Coastline
class GeoStandIn:
    def __init__(self, geo):
        self.__geo_interface__ = geo


def test_coastline_parsing():
    sq = [(0.0, 0.0), (2.0, 0.0), (2.0, 1.0), (0.0, 1.0)]
    c = Coastline([sq])
    assert c.n_rings == 1 and c.bbox == (0.0, 0.0, 2.0, 1.0) and c.edges.dtype == np.float64
    assert c.edges.tolist() == [[2.0, 0.0, 2.0, 1.0], [0.0, 1.0, 0.0, 0.0]]  # the two horizontal sides never count: dropped
    assert np.array_equal(Coastline([sq + sq[:1]]).edges, c.edges)            # a repeated closing vertex
    assert np.array_equal(Coastline([np.array(sq)]).edges, c.edges) and np.array_equal(Coastline(np.array(sq)).edges, c.edges)
    dup = Coastline([[sq[0], sq[1], sq[1], sq[2], sq[3]]])
    assert np.array_equal(dup.edges, c.edges)                                 # a zero-length edge
    hole = [(0.5, 0.25), (1.5, 0.25), (1.0, 0.75)]
    poly = {"type": "Polygon", "coordinates": [sq + sq[:1], hole + hole[:1]]}
    want = Coastline([sq, hole])
    assert want.n_rings == 2 and len(want.edges) == 4
    for obj in (GeoStandIn(poly), [GeoStandIn(poly)], poly,
                GeoStandIn({"type": "MultiPolygon", "coordinates": [[sq], [hole]]}),
                GeoStandIn({"type": "GeometryCollection", "geometries": [{"type": "Polygon", "coordinates": [sq]}, GeoStandIn({"type": "Polygon", "coordinates": [hole]})]}),
                GeoStandIn({"type": "Feature", "geometry": poly, "properties": {}}),
                GeoStandIn({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": poly}, {"type": "Feature", "geometry": None}]}),
                [sq, GeoStandIn({"type": "Polygon", "coordinates": [hole]})]):
        got = Coastline(obj)
        assert got.n_rings == 2 and np.array_equal(got.edges, want.edges)
    # across the antimeridian, given wrapped: made continuous along the ring
    c = Coastline([[(175.0, 2.0), (-175.0, 2.0), (-175.0, -2.0), (175.0, -2.0)]])
    assert c.bbox == (175.0, -2.0, 185.0, 2.0) and c.edges.tolist() == [[185.0, 2.0, 185.0, -2.0], [175.0, -2.0, 175.0, 2.0]]
    empty = Coastline([])
    assert empty.n_rings == 0 and empty.bbox is None and empty.edges.shape == (0, 4)
    # exactly 360 degrees is a global file; more is refused
    Coastline([[(-180.0, 0.0), (0.0, 0.0), (180.0, 0.0), (180.0, 10.0), (0.0, 10.0), (-180.0, 10.0)]])
    with pytest.raises(ValueError, match="360"):
        Coastline([[(-180.0, 0.0), (0.0, 0.0), (170.0, 0.0), (170.0, 1.0)], [(190.0, 0.0), (200.0, 0.0), (200.0, 1.0)]])
    for bad in ([[(0.0, 0.0), (1.0, 1.0)]], [[(0.0, 0.0), (1.0, 1.0), (0.0, 0.0)]], [[(0.0, 0.0), (1.0, np.nan), (2.0, 0.0)]],
                [[(0.0, 0.0), (np.inf, 1.0), (2.0, 0.0)]], [np.zeros((4, 1))], [np.zeros(4)]):
        with pytest.raises(ValueError):
            Coastline(bad)
    with pytest.raises(ValueError, match="Point"):
        Coastline(GeoStandIn({"type": "Point", "coordinates": [0.0, 0.0]}))


# --------------------------------------------------------------------------------------------------------- the public call
def test_every_refusal_comes_before_the_library(monkeypatch):
    reached = []

    def device(*_a, **_k):
        reached.append(1)
        raise RuntimeError("the device")

    monkeypatch.setattr(_lib, "default_context", device)
    case = lc.small_cases(CHUNK)["archipelago"]
    coast, tp = case.coastline(), case.tie_points()
    ok = dict(shape=(lc.L, lc.S))
    with pytest.raises(TypeError, match="Coastline"):
        land_mask(case.rings, tp, **ok)
    with pytest.raises(TypeError, match="TiePoints"):
        land_mask(coast, (case.tie_lon, case.tie_lat), **ok)
    for kw in (dict(), dict(shape=(lc.L, lc.S), line=np.arange(lc.L), sample=np.arange(lc.S)), dict(line=np.arange(lc.L)), dict(shape=(lc.L,)),
               dict(shape=(-1, 4)), dict(shape=(38, lc.S)), dict(line=np.arange(lc.L), sample=np.arange(lc.S) + 0.5),
               dict(line=np.array([np.nan]), sample=np.arange(lc.S)), dict(line=np.zeros((2, 2)), sample=np.arange(lc.S))):
        with pytest.raises(ValueError):
            land_mask(coast, tp, **kw)
    with pytest.raises(ValueError, match="single tie-point"):
        single = lc.small_cases(CHUNK)["single_tie_line"]
        land_mask(coast, single.tie_points(), line=[5.0, 5.0], sample=np.arange(lc.S))
    with pytest.raises(TypeError, match="and_with"):
        land_mask(coast, tp, and_with=np.ones((lc.L, lc.S), np.float32), **ok)
    with pytest.raises(ValueError, match="and_with"):
        land_mask(coast, tp, and_with=np.ones((lc.L, lc.S + 1), bool), **ok)
    monkeypatch.setenv("XSW_LAND_PATH", "lanes")
    with pytest.raises(ValueError, match="XSW_LAND_PATH"):
        land_mask(coast, tp, **ok)
    monkeypatch.delenv("XSW_LAND_PATH")
    monkeypatch.setenv("XSW_LAND_BANDS", "0")
    with pytest.raises(ValueError, match="XSW_LAND_BANDS"):
        land_mask(coast, tp, **ok)
    monkeypatch.delenv("XSW_LAND_BANDS")
    assert not reached
    with pytest.raises(RuntimeError, match="the device"):  # a good call reaches the library
        land_mask(coast, tp, **ok)
    assert reached


# ------------------------------------------------------------------------------------------------------------ declarations
def test_public_names():
    import xsarsea_amd
    assert xsarsea_amd.landmask is landmask and xsarsea_amd.land_mask is landmask.land_mask and xsarsea_amd.Coastline is landmask.Coastline
    assert {"landmask", "Coastline", "land_mask"} <= set(xsarsea_amd.__all__) and {"Coastline", "land_mask", "plan", "LandPlan"} <= set(landmask.__all__)


def test_header_declares_the_entries_and_the_binding_matches():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "xsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+xsw_land_mask\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/xsw.h does not declare xsw_land_mask"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _lib.RASTER_ENTRIES["xsw_land_mask"]
    assert params[0].startswith("xsw_ctx") and len(params) == 1 + len(sig) == 23

    def letter(p):
        return "p" if "*" in p else {"int64_t": "l", "int32_t": "i", "double": "d"}[p.split()[0]]

    assert "".join(letter(p) for p in params[1:]) == sig
    assert re.search(r"\bint32_t\s+xsw_land_chunk_edges\s*\(\s*void\s*\)\s*;", txt)
    assert {"xsw_land_mask", "xsw_land_chunk_edges"} <= set(_lib.EXPORTS) and hasattr(_lib.Context, "land_mask_raw")
    assert int(re.search(r"#\s*define\s+XSW_VERSION\s+(\d+)", txt).group(1)) == 4 == _lib.ABI_VERSION


def test_the_unit_is_built_and_the_kernels_use_no_scratch():
    assert os.path.basename(_build.SRC_LANDMASK) == "xsw_landmask.hip" and os.path.exists(_build.SRC_LANDMASK)
    assert _build.build() == _build.LIB and os.path.exists(_build.LIB)
    rows = [r for r in _build.kernel_resources() if "k_land_mask" in r["kernel"]]
    direct = [r for r in rows if "k_land_mask_direct" in r["kernel"]]
    assert len(rows) == 4 and len(direct) == 2  # with and without and_with
    chunk_bytes = 32 * _lib.land_chunk_edges()
    for r in rows:
        assert r["scratch_bytes"] == 0 and chunk_bytes <= r["lds_bytes"] <= chunk_bytes + 256, r
        assert 4 * r["lds_bytes"] <= 160 * 1024  # four workgroups fit a CU's LDS
    with open(os.path.join(REPO, "profiles", "landmask_kernel_resources.tsv")) as f:
        table = [ln.split("\t") for ln in f.read().splitlines() if ln and not ln.startswith("#")][1:]
    assert len(table) == 4 and all(t[4] == "0" for t in table)
    figures = lambda r: (r["vgpr"], r["agpr"], r["sgpr"], r["lds_bytes"], r["scratch_bytes"], r["waves_per_simd_by_vgpr"], "direct" in r["kernel"])
    assert sorted(figures(r) for r in rows) == sorted(tuple(int(v) for v in t[:6]) + ("direct" in t[6],) for t in table)
