"""The land-mask cases shared by tests/test_landmask_cpu.py and tests/test_gpu_landmask.py.  Each case is a coastline (rings, or
objects with `__geo_interface__`), a tie-point grid and a raster; `Case.want()` is the restatement's mask (tests/landmask_ref.py),
computed once per case and left unchanged.  `check_case` holds every case to the property it is there for; the CPU test runs it.

Geometry of the kernels (csrc/xsw_landmask.hip): a thread owns four consecutive samples, a workgroup 1024 samples (256 threads)
of the lines strip_grid gives it, in line groups of four.  The small raster of 37 x 300 is therefore one workgroup column of 75
threads, a full wave (samples 0 .. 255) and an 11-lane one (samples 256 .. 299), and one line per workgroup; the strip raster
brings a second workgroup column, five lines per workgroup and a short last workgroup."""
import numpy as np

import landmask_ref as lref

L, S = 37, 300
TIE_LINE = np.array([0.0, 4.0, 36.0])             # non-uniform, dyadic weights; raster line 4 is a tie line
TIE_SAMPLE = np.array([0.0, 70.0, 256.0, 299.0])  # raster column 256 is a tie column
BANDS = (1, 7, 64, 1000)                          # the forced band counts (None: the plan's own rule)


def strip_grid(rows, cols, wg_per_cu=16):
    """csrc/xsw_plan.hpp: strip_grid, restated."""
    gx = (cols + 255) // 256
    gy = (256 * wg_per_cu + gx - 1) // gx
    gy = max(1, min(gy, rows, 65535))
    rpb = (rows + gy - 1) // gy
    gy = (rows + rpb - 1) // rpb
    return gx, gy, rpb


def land_grid(lines, samples):
    """The launch grid of xsw_land_mask: strip_grid on the raster of sample quads."""
    return strip_grid(lines, (samples + 3) // 4)


class Case:
    def __init__(self, name, rings, tie_line, tie_sample, tie_lon, tie_lat, line, sample, source=None, small=True):
        self.name, self.rings, self.source = name, rings, rings if source is None else source
        self.tie_line, self.tie_sample = np.asarray(tie_line, np.float64), np.asarray(tie_sample, np.float64)
        self.tie_lon, self.tie_lat = np.asarray(tie_lon, np.float64), np.asarray(tie_lat, np.float64)
        self.line, self.sample = np.asarray(line, np.float64), np.asarray(sample, np.float64)
        self.small = small  # the forced band counts run on the small cases
        self._want = self._pos = None

    @property
    def shape(self):
        return len(self.line), len(self.sample)

    def positions(self, lines=None):
        """px, py of the raster (of the given line indices only)."""
        if lines is not None:
            return lref.lonlat(self.tie_line, self.tie_sample, self.tie_lon, self.tie_lat, self.line[lines], self.sample)
        if self._pos is None:
            self._pos = lref.lonlat(self.tie_line, self.tie_sample, self.tie_lon, self.tie_lat, self.line, self.sample)
        return self._pos

    def ref_edges(self, px):
        return lref.turn_copies(lref.edges_of(self.rings), px)

    def want(self):
        if self._want is None:
            px, py = self.positions()
            self._want = (~lref.land(px, py, self.ref_edges(px))).astype(np.uint8)
            self._want.flags.writeable = False
        return self._want

    def coastline(self):
        from xsarsea_amd import Coastline
        return Coastline(self.source)

    def tie_points(self):
        from xsarsea_amd import TiePoints
        return TiePoints(self.tie_line, self.tie_sample, self.tie_lon, self.tie_lat, np.zeros(self.tie_lon.shape))

    def raster(self):
        """The public call's raster arguments."""
        return dict(line=self.line, sample=self.sample)


def scene():
    """Tie grids of the small raster: lon 10 .. 12.3, lat 3.25 .. 1.5, the latitude tilted along the samples."""
    lon = 10.0 + 2.2 * TIE_SAMPLE[None, :] / 299.0 + 0.1 * TIE_LINE[:, None] / 36.0
    lat = 3.25 - 1.6 * TIE_LINE[:, None] / 36.0 - 0.15 * TIE_SAMPLE[None, :] / 299.0
    return lon, lat


def small_case(name, rings, source=None, lon_lat=None, line=None, sample=None):
    lon, lat = scene() if lon_lat is None else lon_lat
    return Case(name, rings, TIE_LINE, TIE_SAMPLE, lon, lat, np.arange(L) if line is None else line, np.arange(S) if sample is None else sample,
                source=source)


def star(cx, cy, r, n, lobes, phase=0.0):
    t = phase + 2.0 * np.pi * np.arange(n) / n
    rr = r * (1.0 + 0.35 * np.cos(lobes * t))
    return np.stack([cx + rr * np.cos(t), cy + rr * np.sin(t)], axis=1)


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def archipelago():
    rings = [star(10.6, 2.9, 0.35, 200, 5), star(11.6, 2.7, 0.40, 500, 7, 0.3), star(12.1, 3.1, 0.25, 300, 3, 1.0),
             star(10.9, 2.3, 0.30, 700, 9, 0.2), box(9.0, 0.0, 13.0, 2.0)]
    return small_case("archipelago", rings)


# ---- exact hits: dyadic tie tables.  lon = 8 + s / 64 + l / 256, lat = 36 + l / 8 on tie lines 0, 4, 36 and tie samples 0, 64,
# 320, 576 (spacings 4, 32 and 64, 256: powers of two): every weight and every node is a short dyadic number, so every product
# and sum of the blend is exact.
EXACT_TIE_SAMPLE = np.array([0.0, 64.0, 320.0, 576.0])
EXACT_VERTICES = ((5, 10), (5, 200), (30, 200), (30, 10))  # (line, sample) of the quadrilateral's vertices


def exact_lonlat(l, s):
    l, s = np.asarray(l, np.float64), np.asarray(s, np.float64)
    return 8.0 + s / 64.0 + l / 256.0, 36.0 + l / 8.0 + 0.0 * s


def exact_scene():
    return exact_lonlat(TIE_LINE[:, None], EXACT_TIE_SAMPLE[None, :])


def exact_hits():
    ring = np.array([exact_lonlat(l, s) for l, s in EXACT_VERTICES], dtype=np.float64)
    lon, lat = exact_scene()
    return Case("exact_hits", [ring], TIE_LINE, EXACT_TIE_SAMPLE, lon, lat, np.arange(L), np.arange(S))


def exact_expected():
    """The closed form.  The map pixel -> (lon, lat) is affine, so the quadrilateral is the pixel rectangle lines 5 .. 30, samples
    10 .. 200 and a pixel on a side is exactly on it (a == b: no hit from that side).  Half-open in latitude: line 5 (the lower
    latitude) belongs, line 30 does not; a pixel on the western side is land (only the eastern side counts, from the east), one on
    the eastern side is water.  Of the four corners only (5, 10) is land."""
    out = np.ones((L, S), np.uint8)
    out[5:30, 10:200] = 0
    return out


def exact_expected_in_integers():
    """The statement in whole numbers: X = 256 (lon - 8) = 4 s + l, Y = 8 (lat - 36) = l."""
    l, s = np.meshgrid(np.arange(L), np.arange(S), indexing="ij")
    X, Y = 4 * s + l, l
    v = [(4 * b + a, a) for a, b in EXACT_VERTICES]
    land = np.zeros((L, S), bool)
    for (x1, y1), (x2, y2) in zip(v, v[1:] + v[:1]):
        straddle = (y1 > Y) != (y2 > Y)
        east = X < min(x1, x2)
        a, b = (X - x1) * (y2 - y1), (Y - y1) * (x2 - x1)
        mid = ~east & (X <= max(x1, x2)) & ((a < b) if y2 > y1 else (a > b))
        land ^= straddle & (east | mid)
    return (~land).astype(np.uint8)


def nothing_near():
    """name -> (case, all land?)."""
    return {"enclosing": (small_case("enclosing", [box(0.0, -5.0, 20.0, 10.0)]), True),
            "east": (small_case("east", [star(14.0, 2.5, 0.8, 40, 3)]), False),
            "west": (small_case("west", [star(8.0, 2.5, 0.8, 40, 3)]), False),
            "north": (small_case("north", [star(11.0, 5.0, 0.8, 40, 3)]), False),
            "south": (small_case("south", [star(11.0, 0.0, 0.8, 40, 3)]), False),
            "no_edges": (small_case("no_edges", []), False)}


class PolygonStandIn:
    """What shapely's Polygon exposes, and nothing else."""

    def __init__(self, exterior, interiors):
        self.__geo_interface__ = {"type": "Polygon", "coordinates": [[tuple(p) for p in r] + [tuple(r[0])] for r in [exterior] + list(interiors)]}


def lake_and_island(as_polygon=False):
    rings = [star(11.2, 2.4, 0.9, 90, 4), star(11.2, 2.4, 0.5, 60, 3, 0.5), star(11.25, 2.4, 0.2, 30, 5)]
    return small_case("lake_and_island" + ("_polygon" if as_polygon else ""), rings,
                      source=[PolygonStandIn(rings[0], rings[1:])] if as_polygon else None)


def comb(chunk):
    """5 x 300: one ring, a spine south of the scene with chunk + 76 teeth that cross every latitude of it: 2 (chunk + 76) edges
    in every band, more than two staging chunks of `chunk` edges."""
    n = chunk + 76
    pitch = 2.4 / n
    left = 9.95 + pitch * np.arange(n)
    right = left + 0.5 * pitch
    pts = [(left[0], 0.0), (right[-1], 0.0)]
    for t in range(n - 1, -1, -1):
        pts += [(right[t], 4.0), (left[t], 4.0)]
        if t:
            pts += [(left[t], 1.0), (right[t - 1], 1.0)]
    return small_case("comb", [np.array(pts)], line=np.arange(5.0))


def antimeridian():
    """Tie longitudes 150 -> 380, given wrapped.  name -> ring: one across +-180 given with the jump, one at -170, one at 20."""
    wrapped = np.array([150.0, -160.0, -30.0, 20.0])[None, :] + np.array([0.0, 1.5, 9.0])[:, None]
    lat = np.array([8.0, 5.5, -8.0])[:, None] - 0.7 * TIE_SAMPLE[None, :] / 299.0
    rings = {"across": np.array([[175.0, 3.0], [-175.0, 3.0], [-175.0, -3.0], [175.0, -3.0]]), "at_minus_170": box(-173.0, 1.0, -167.0, 7.0),
             "at_20": box(15.0, -7.5, 29.5, -1.0)}
    cases = {name: small_case("antimeridian_" + name, [r], lon_lat=(wrapped, lat)) for name, r in rings.items()}
    cases["all"] = small_case("antimeridian", list(rings.values()), lon_lat=(wrapped, lat))
    return cases


def degenerate():
    """Coastlines: a ring with duplicate consecutive vertices, a ring with a horizontal edge through pixel latitudes (the exact
    tie tables: latitude 36 + 10 / 8 is that of line 10), three collinear points.  Rasters: L = 1, S = 1, one pixel, L = 0."""
    dup = star(11.2, 2.4, 0.7, 24, 3)
    dup = np.concatenate([dup[:5], dup[4:5], dup[4:]])
    x0, y0 = exact_lonlat(10, 40)
    x1, y1 = exact_lonlat(20, 120)
    horizontal = np.array([[x0, y0], [x1 + 1.0, y0], [x1, y1], [x0 - 0.25, y1]])
    out = [small_case("duplicate_vertices", [dup]),
           Case("horizontal_edge", [horizontal], TIE_LINE, EXACT_TIE_SAMPLE, *exact_scene(), np.arange(L), np.arange(S)),
           small_case("collinear", [np.array([[10.2, 1.6], [11.2, 2.4], [12.2, 3.2]])])]
    arch = archipelago().rings
    out += [small_case("one_line", arch, line=np.array([7.0])), small_case("one_sample", arch, sample=np.array([131.5])),
            small_case("one_pixel", arch, line=np.array([36.0]), sample=np.array([299.0])), small_case("no_lines", arch, line=np.empty(0))]
    lon, lat = scene()
    out.append(Case("single_tie_line", arch, [5.0], TIE_SAMPLE, lon[1:2], lat[1:2], [5.0], np.arange(S)))
    return out


# ---- strip: 8197 x 1030.  The raster of sample quads is 8197 x 258: two workgroup columns (the second holds samples 1024 ..
# 1029: one thread of four samples and one of two; 1030 is no multiple of four, so bytes are stored one by one), 1640 workgroup
# rows of five lines (a line group of four and one more line), a last one of two lines.
STRIP_SHAPE = (8197, 1030)
STRIP_GRID = (2, 1640, 5, 2)  # gx, gy, lines per workgroup, lines of the last workgroup
STRIP_TIE_LINE = np.array([0.0, 5.0, 6.5, 7.0, 8.0, 4000.0, 8195.5, 8196.0])
STRIP_TIE_SAMPLE = np.array([0.0, 700.25, 1029.0])


def strip_rows(block):
    gx, gy, rpb, _ = STRIP_GRID
    b = block % gy
    return np.arange(b * rpb, min((b + 1) * rpb, STRIP_SHAPE[0]))


def strip():
    Lb, Sb = STRIP_SHAPE
    rng = np.random.default_rng(6)
    lon = 10.0 + 2.3 * STRIP_TIE_SAMPLE[None, :] / 1029.0 + 0.1 * STRIP_TIE_LINE[:, None] / 8196.0 + rng.uniform(-0.01, 0.01, (8, 3))
    lat = 3.25 - 1.6 * STRIP_TIE_LINE[:, None] / 8196.0 - 0.15 * STRIP_TIE_SAMPLE[None, :] / 1029.0 + rng.uniform(-0.01, 0.01, (8, 3))
    rings = [np.array([[11.0, 5.0], [13.0, 5.0], [13.0, 0.0], [11.4, 0.0]]), star(10.4, 2.5, 0.25, 6, 2), box(12.0, 2.0, 12.2, 2.4)]
    return Case("strip", rings, STRIP_TIE_LINE, STRIP_TIE_SAMPLE, lon, lat, np.arange(Lb), np.arange(Sb), small=False)


def check_strip_geometry(case):
    Lb, Sb = case.shape
    gx, gy, rpb = land_grid(Lb, Sb)
    assert (gx, gy, rpb, Lb - (gy - 1) * rpb) == STRIP_GRID and rpb > 4 and Sb % 4
    assert len(lref.edges_of(case.rings)) <= 64
    first, _ = lref.bracket(case.tie_line, case.line)
    changes = {int(l) for l in np.nonzero(np.diff(first))[0] + 1}
    second, last = strip_rows(1), strip_rows(-1)
    assert {int(l - second[0]) for l in second[:4] if int(l) in changes} >= {2, 3}   # inside the second row's line group of four
    assert any(int(l) in changes for l in last[1:])


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def small_cases(chunk):
    """Every case of the small rasters, by name (built once per process)."""
    def make():
        cases = [archipelago(), exact_hits(), lake_and_island(), lake_and_island(True), comb(chunk)]
        cases += [c for c, _ in nothing_near().values()] + list(antimeridian().values()) + degenerate()
        return {c.name: c for c in cases}
    return cached(("small", chunk), make)


def strip_case():
    return cached("strip", strip)


def check_case(case, chunk, plan_at_64=None):
    """The property the case is there for, on the restatement's mask.  plan_at_64: the package's plan at 64 bands (archipelago)."""
    want = case.want()
    land = want == 0
    name = case.name
    if name == "archipelago":
        assert len(lref.edges_of(case.rings)) == 1704
        assert 0.2 < land.mean() < 0.8
        for cols in (slice(0, 256), slice(256, 300)):  # the full wave's samples and the 11-lane one's
            assert land[:, cols].any() and not land[:, cols].all()
        if plan_at_64 is not None:
            _, py = case.positions()
            assert all(len(np.unique(plan_at_64.band_of(py[l]))) > 1 for l in range(L))  # one line is one workgroup row
    elif name == "exact_hits":
        assert np.array_equal(want, exact_expected()) and np.array_equal(want, exact_expected_in_integers())
        assert [int(land[l, s]) for l, s in EXACT_VERTICES] == [1, 0, 0, 0]
        px, py = case.positions()
        e = lref.edges_of(case.rings)
        assert all((py == y).any() for y in e[:, 1])
        sides = e[e[:, 1] != e[:, 3]]
        assert len(sides) == 2 and all((px == min(x1, x2)).any() and (px == max(x1, x2)).any() for x1, _, x2, _ in sides)
    elif name == "enclosing":
        px, py = case.positions()
        e = lref.edges_of(case.rings)
        assert land.all() and not ((e[:, 0] > px.min()) & (e[:, 0] < px.max()) & (e[:, 1] > py.min()) & (e[:, 1] < py.max())).any()
    elif name in ("east", "west", "north", "south", "no_edges", "collinear"):
        assert not land.any()
    elif name.startswith("lake_and_island"):
        px, py = case.positions()
        layers = [lref.land(px, py, lref.edges_of([r])) for r in case.rings]
        assert (layers[0] & ~layers[1]).any() and (layers[1] & ~layers[2]).any() and layers[2].any()  # island, lake, islet
        assert np.array_equal(land, layers[0] ^ layers[1] ^ layers[2])
    elif name == "comb":
        assert case.shape == (5, 300) and (lref.edges_of(case.rings)[:, 1] != lref.edges_of(case.rings)[:, 3]).sum() > 2 * chunk
        assert all(0.2 < land[l].mean() < 0.8 for l in range(5))
    elif name.startswith("antimeridian"):
        assert land.any() and not land.all()
    elif name == "duplicate_vertices":
        assert 0.05 < land.mean() < 0.9
    elif name == "horizontal_edge":
        _, py = case.positions()
        y = lref.edges_of(case.rings)[0, 1]
        assert (py == y).any() and land.any() and land[10, 40:120].all() and not land[20].any()  # half-open: the lower latitude belongs
    elif name in ("one_line", "one_sample"):
        assert land.any() and not land.all()
    elif name == "one_pixel":
        assert want.shape == (1, 1)
    elif name == "no_lines":
        assert want.shape == (0, S)
    elif name == "single_tie_line":
        assert want.shape == (1, S) and land.any() and not land.all()
    else:
        raise AssertionError(f"case {name} has no property")
