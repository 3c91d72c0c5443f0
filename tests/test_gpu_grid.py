"""xsarsea_amd.grid on the MI355X against its CPU restatement (tests/grid_ref.py).  Every comparison is bit for bit: the int64
`sums` equal, and every finished field through `cells_ref.same_bits` (NaN where and only where the restatement has NaN, every
other value equal as uint64).  The scene and the five grids are tests/grid_cases.py's, which asserts what each grid is there for
on the restatement before anything runs here; each runs from complex128, complex64 and co-pol codes, on the default path and on
both forced ones (XSW_GRID_PATH = lds / direct, read at every call), through device tensors and through numpy arrays."""
import functools
import warnings

import numpy as np
import pytest

import grid_cases as gc
import grid_ref as gref
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from test_host_plan import source_define
from xsarsea_amd import TiePoints, WindGrid, _lib, wind_grid, windspeed
from xsarsea_amd.grid import GridSpec
from xsarsea_amd.windspeed.crosspol import CopolCodes

pytestmark = pytest.mark.gpu

FIELDS = gref.NAMES


@pytest.fixture(params=["default", "lds", "direct"])
def path(request, monkeypatch):
    if request.param == "default":
        monkeypatch.delenv("XSW_GRID_PATH", raising=False)
    else:
        monkeypatch.setenv("XSW_GRID_PATH", request.param)
    return request.param


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def up(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))  # a copy: the cached cases are read-only


def on(torch, route):
    return (lambda a: up(torch, a)) if route == "device" else (lambda a: None if a is None else np.array(a))


def tie_points():
    return TiePoints(*gc.ties())


def spec(name):
    g = gc.GRIDS[name]
    return dict(lon=g[:3], lat=g[3:])


def assert_same(got, want_sums, want_fields, what):
    s = host(got.sums)
    assert s.dtype == np.int64 and np.array_equal(s, want_sums), f"{what}: {int((s != want_sums).sum())} sums differ"
    for name in FIELDS:
        g = host(got[name])
        assert gref.same_bits(g, want_fields[name]), f"{what} {name}: {int((g != want_fields[name]).sum())} bins differ (NaN counted)"


# ------------------------------------------------------------------------------------------------------------ complex sources
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("name", sorted(gc.GRIDS))
def test_wind_grid(torch, path, name, dtype, route):
    w, keep = gc.scene(dtype)
    want_sums, want = gc.case(name, dtype)
    put = on(torch, route)
    got = wind_grid(put(w), tie_points(), keep=put(keep), **spec(name))
    if route == "device":
        assert isinstance(got.sums, torch.Tensor) and got.sums.is_cuda and got.sums.dtype == torch.int64 and got.u.is_cuda and got.u.dtype == torch.float64
    else:
        assert isinstance(got.sums, np.ndarray) and isinstance(got.u, np.ndarray)
    assert tuple(got.sums.shape) == (5, gc.GRIDS[name][5], gc.GRIDS[name][2]) and got.spec.periodic == (name == "periodic")
    assert_same(got, want_sums, want, f"{name} {np.dtype(dtype).name} {path} {route}")
    if name == "fine":
        assert np.isnan(host(got.wspd_std)).all()
    if name == "desc":  # no keep: the NULL pointer's path
        assert np.array_equal(host(wind_grid(put(w), tie_points(), **spec(name)).sums), gref.sums(w, *gc.ties(), gc.GRIDS[name]))
        ok = want_sums[0] > 0
        d = host(got.direction)
        off = (d[ok] - (270.0 - np.degrees(np.arctan2(want["v"][ok], want["u"][ok]))) + 180.0) % 360.0 - 180.0
        assert np.isnan(d[~ok]).all() and np.abs(off).max() < 1e-9  # the one value not pinned to the bit


# ---------------------------------------------------------------------------------------------------------------------- codes
@functools.lru_cache(maxsize=None)
def codes_scene():
    """(inc, raw uint32 codes, their LUT, the complex128 expansion on the host) of a small LUT inversion over the scene's
    raster, with NaN pixels and two codes of no grid point, as tests/test_gpu_cells.py::test_cells_from_codes makes them."""
    inc, s_vv, _, _, anc = synthetic_scene(gc.L, gc.S, np.float64, 31)   # its first three columns have a NaN incidence
    anc[5, 10:20] = np.nan
    anc[42:49, 27:36] = complex(np.nan, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
    raw = host(cc.codes).view(np.uint32).copy()
    assert ((raw & 0x80000000) != 0).sum() > gc.L * 3
    raw[20, 30] = 0x80000005          # a code of no LUT: bit 31
    raw[21, 31] = 0x3FFFFFFF          # and one whose index lies beyond this LUT's plane
    wh = host(CopolCodes(inc, raw, cc.lut_co).wind())
    assert wh.dtype == np.complex128 and np.isnan(wh[20, 30].real) and np.isnan(wh[21, 31].real) and (~np.isnan(wh.real)).mean() > 0.8
    for a in (inc, raw, wh):
        a.setflags(write=False)
    return inc, raw, cc.lut_co, wh


@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", sorted(gc.GRIDS))
def test_grid_from_codes(torch, path, name, route):
    inc, raw, lut, wh = codes_scene()
    _, keep = gc.scene()
    want_sums = gref.sums(wh, *gc.ties(), gc.GRIDS[name], keep=keep)
    assert want_sums[0].sum() > (1000 if name == "partial" else 15000)
    put = on(torch, route)
    codes = CopolCodes(put(inc), up(torch, raw.view(np.int32)) if route == "device" else np.array(raw), lut)
    got = codes.grid(tie_points(), keep=put(keep), **spec(name))
    assert (hasattr(got.sums, "is_cuda") and got.sums.is_cuda) == (route == "device")
    assert_same(got, want_sums, gref.finish(want_sums), f"codes {name} {path} {route}")
    other = wind_grid(put(wh), tie_points(), keep=put(keep), **spec(name))   # the complex128 expansion
    assert np.array_equal(host(other.sums), host(got.sums))


# --------------------------------------------------------------------------------------------------------------------- strips
def launch_of(lines, samples):
    """(workgroup columns, line strips, lines per strip) of k_wind_grid's launch: strip_grid (tests/test_host_plan.py restates
    it) with strips of XSW_GRID_MIN_LINES lines or more."""
    gx = -(-samples // 256)
    gy = max(1, min(-(-256 * 16 // gx), lines, 65535))
    lpb = max(-(-lines // gy), source_define("XSW_GRID_MIN_LINES"))
    return gx, -(-lines // lpb), lpb


STRIP_GRID = (179.0, 0.25, 8, 8.0, 0.25, 16)


@functools.lru_cache(maxsize=None)
def strip_case():
    """A raster beyond one strip and one workgroup column: 46 full strips and a short one, two full workgroup columns and a
    ragged third; a coarse grid, so every workgroup merges through its table and the strips meet in global memory."""
    lines, samples = 46 * source_define("XSW_GRID_MIN_LINES") + 28, 2 * 256 + 188
    rng = np.random.default_rng(8)
    tl, ts = np.array([0.0, 0.37 * lines, lines - 1.0]), np.array([0.0, 0.2 * samples, 0.7 * samples, samples - 1.0])
    l, s = tl[:, None], ts[None, :]
    ties = (tl, ts, gc.wrap(179.1 + 0.0018 * s + 0.0002 * l), 9.0 + 0.0012 * l - 0.0003 * s, -12.0 + 0.001 * l + 0.002 * s)
    w = rng.normal(0.0, 12.0, (lines, samples)) + 1j * rng.normal(0.0, 12.0, (lines, samples))
    w[rng.uniform(size=w.shape) < 0.05] = np.nan
    keep = rng.uniform(size=w.shape) < 0.9
    want = gref.sums(w, *ties, STRIP_GRID, keep=keep)
    assert (want[0] > 0).sum() >= 30 and want[0].sum() > 0.8 * lines * samples
    return w, keep, ties, want


def test_beyond_one_strip_and_one_workgroup_column(torch, path):
    w, keep, ties, want = strip_case()
    lines, samples = w.shape
    gx, gy, lpb = launch_of(lines, samples)
    assert gx == 3 and samples % 256 and gy >= 2 and lines % lpb and 1400 < lines < 1600 and 600 < samples < 800, (gx, gy, lpb)
    got = wind_grid(up(torch, w), TiePoints(*ties), keep=up(torch, keep), lon=STRIP_GRID[:3], lat=STRIP_GRID[3:])
    assert_same(got, want, gref.finish(want), f"strips {path}")


# --------------------------------------------------------------------------------------------------------------- accumulating
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", ["coarse", "fine"])
def test_accumulating_in_any_order(torch, path, name, route):
    from test_grid_cpu import second_scene
    a, keep = gc.scene()
    b, ties_b = second_scene()
    put = on(torch, route)
    tp_a, tp_b = tie_points(), TiePoints(*ties_b)
    whole, _ = gc.case(name)
    want = gref.sums(b, *ties_b, gc.GRIDS[name], into=whole.copy())
    assert not np.array_equal(want, whole)
    ab = wind_grid(put(b), tp_b, into=wind_grid(put(a), tp_a, keep=put(keep), **spec(name)), **spec(name))
    first = wind_grid(put(b), tp_b, **spec(name))
    ba = wind_grid(put(a), tp_a, keep=put(keep), into=first, **spec(name))
    assert ba is first
    assert_same(ab, want, gref.finish(want), f"A then B, {name} {path} {route}")
    assert_same(ba, want, gref.finish(want), f"B then A, {name} {path} {route}")
    # the two row halves of one scene, each with its own lines; then merged from two grids
    top = wind_grid(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), **spec(name))
    both = wind_grid(put(a[48:]), tp_a, line=np.arange(48, gc.L), keep=put(keep[48:]), into=top, **spec(name))
    assert_same(both, whole, gc.case(name)[1], f"row halves, {name} {path} {route}")
    lower = wind_grid(put(a[48:]), tp_a, line=np.arange(48, gc.L), keep=put(keep[48:]), **spec(name))
    upper = wind_grid(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), **spec(name))
    upper += lower
    assert_same(upper, whole, gc.case(name)[1], f"merged halves, {name} {path} {route}")
    # the same call twice
    again = wind_grid(put(a), tp_a, keep=put(keep), **spec(name))
    assert np.array_equal(host(again.sums), whole) and np.array_equal(host(wind_grid(put(a), tp_a, keep=put(keep), **spec(name)).sums), host(again.sums))


# --------------------------------------------------------------------------------------------------------- further properties
def test_keep_alone_empties_a_bin(torch, path):
    w, keep = gc.scene()
    g = gc.GRIDS["coarse"]
    p = gc.pixels()
    inside, i, j = gref.bins(p["lon"], p["lat"], g)
    whole, _ = gc.case("coarse")
    jj, ii = np.unravel_index(np.argmax(whole[0]), whole[0].shape)
    k2 = np.array(keep)
    k2[inside & (j == jj) & (i == ii)] = False
    want = gref.sums(w, *gc.ties(), g, keep=k2)
    assert whole[0][jj, ii] > 3000 and want[0][jj, ii] == 0 and (want[0] > 0).sum() == 14
    for put in (on(torch, "device"), on(torch, "numpy")):
        got = wind_grid(put(w), tie_points(), keep=put(k2), **spec("coarse"))
        assert_same(got, want, gref.finish(want), "keep")
        assert host(got.count)[jj, ii] == 0 and np.isnan(host(got.u)[jj, ii])


def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):
    """`wind` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns while the
    producer is still in flight and its sums are those of the filled values."""
    dev = torch.device("cuda", 0)
    w, keep = gc.scene()
    want, fields = gc.case("desc")
    decoy = np.where(np.isnan(w.real), w, w * 0.5)
    assert not np.array_equal(gref.sums(decoy, *gc.ties(), gc.GRIDS["desc"], keep=keep), want)
    tp = tie_points()
    buf, src, tk = up(torch, decoy), up(torch, w), up(torch, keep)
    wind_grid(src, tp, keep=tk, **spec("desc"))   # once on landed values: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = wind_grid(buf, tp, keep=tk, **spec("desc"))
        u, wspd_std = out.u, out.wspd_std
        _in_flight(done)
        got = _read_back(torch, P, out.sums, u, wspd_std)
    assert np.array_equal(got[0], want) and gref.same_bits(got[1], fields["u"]) and gref.same_bits(got[2], fields["wspd_std"])


def test_bad_path_and_mixed_containers_are_refused(torch, monkeypatch):
    w, keep = gc.scene()
    tp = tie_points()
    with pytest.raises(ValueError, match="container kind"):
        wind_grid(up(torch, w), tp, keep=keep, **spec("coarse"))
    with pytest.raises(ValueError, match="container kind"):
        wind_grid(up(torch, w), tp, into=WindGrid(np.zeros((5, 6, 8), np.int64), GridSpec(*spec("coarse").values())), **spec("coarse"))
    with pytest.raises(ValueError, match="container kind"):
        WindGrid(np.zeros((5, 6, 8), np.int64), GridSpec(*spec("coarse").values())).merge(wind_grid(up(torch, w), tp, **spec("coarse")))
    monkeypatch.setenv("XSW_GRID_PATH", "lanes")
    with pytest.raises(ValueError, match="XSW_GRID_PATH"):
        wind_grid(up(torch, w), tp, **spec("coarse"))


def test_raw_entry_refusals_and_host_sums_are_added_to(monkeypatch):
    """The raw entry on host buffers: `sums` is copied up, added to and copied down; bad arguments give XSW_EINVAL and leave
    `sums` alone, a bad XSW_GRID_PATH among them (read by the library at every call)."""
    monkeypatch.delenv("XSW_GRID_PATH", raising=False)
    ctx = _lib.default_context(0)
    w, keep = gc.scene()
    g = gc.GRIDS["coarse"]
    want, _ = gc.case("coarse")
    tl, ts, lon, lat, heading = gc.ties()
    h = np.deg2rad(heading)
    tables = [np.ascontiguousarray(a, np.float64) for a in (gref.continuous(lon), lat, np.cos(h), np.sin(h))]
    lf, lt = gref.bracket(tl, np.arange(float(gc.L)))
    sf, st = gref.bracket(ts, np.arange(float(gc.S)))
    br = [np.ascontiguousarray(lf, np.int32), np.ascontiguousarray(lt, np.float64), np.ascontiguousarray(sf, np.int32), np.ascontiguousarray(st, np.float64)]
    k8 = np.ascontiguousarray(keep).view(np.uint8)
    sums = np.full((5, 6, 8), 7, np.int64)

    def args(**o):
        t = [None] * 4 if o.get("no_ties") else [a.ctypes.data for a in tables]
        return (gc.L, gc.S, _lib.MEM_HOST, o.get("kind", _lib.CELLS_C128), w.ctypes.data, k8.ctypes.data, 3, 4, *t, *[a.ctypes.data for a in br],
                g[0], o.get("dlon", g[1]), o.get("n_lon", g[2]), o.get("periodic", 0), g[3], o.get("dlat", g[4]), g[5], sums.ctypes.data)
    ctx.wind_grid_raw(*args())
    assert np.array_equal(sums, want + 7)
    for bad in (dict(dlon=0.0), dict(dlon=-0.25), dict(dlat=0.0), dict(dlat=float("nan")), dict(n_lon=0), dict(periodic=2), dict(kind=3), dict(no_ties=True)):
        with pytest.raises(_lib.XswError):
            ctx.wind_grid_raw(*args(**bad))
    monkeypatch.setenv("XSW_GRID_PATH", "lanes")
    with pytest.raises(_lib.XswError, match="XSW_GRID_PATH"):
        ctx.wind_grid_raw(*args())
    assert np.array_equal(sums, want + 7)
