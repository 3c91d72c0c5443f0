"""xsarsea_amd.polar on the MI355X against its CPU restatement (tests/polar_ref.py).  Every comparison is bit for bit: the int64
`sums` equal, and every finished field through `cells_ref.same_bits`.  The scene and the five cases are tests/polar_cases.py's,
which asserts what each case is there for on the restatement before anything runs here; each runs from complex128, complex64
and co-pol codes, on the default path and on both forced ones (XSW_GRID_PATH = lds / direct, read at every call), through device
tensors and through numpy arrays."""
import functools

import numpy as np
import pytest

import polar_cases as pc
import polar_ref as pref
from test_gpu_grid import codes_scene, host, launch_of, on, strip_case, up
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from xsarsea_amd import TiePoints, WindPolar, _lib, wind_polar
from xsarsea_amd.polar import PolarSpec
from xsarsea_amd.windspeed.crosspol import CopolCodes

pytestmark = pytest.mark.gpu

FIELDS = pref.NAMES


@pytest.fixture(params=["default", "lds", "direct"])
def path(request, monkeypatch):
    if request.param == "default":
        monkeypatch.delenv("XSW_GRID_PATH", raising=False)
    else:
        monkeypatch.setenv("XSW_GRID_PATH", request.param)
    return request.param


def tie_points(name):
    return TiePoints(*pc.ties(name))


def assert_same(got, want_sums, want_fields, what):
    s = host(got.sums)
    assert s.dtype == np.int64 and np.array_equal(s, want_sums), f"{what}: {int((s != want_sums).sum())} sums differ"
    for name in FIELDS:
        g = host(got[name])
        assert pref.same_bits(g, want_fields[name]), f"{what} {name}: {int((g != want_fields[name]).sum())} bins differ (NaN counted)"


# ------------------------------------------------------------------------------------------------------------ complex sources
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_wind_polar(torch, path, name, dtype, route):
    w, keep = pc.scene(dtype)
    want_sums, want = pc.case(name, dtype)
    kw = pc.spec(name)
    put = on(torch, route)
    got = wind_polar(put(w), tie_points(name), keep=put(keep), **kw)
    if route == "device":
        assert isinstance(got.sums, torch.Tensor) and got.sums.is_cuda and got.sums.dtype == torch.int64 and got.vt.is_cuda and got.vt.dtype == torch.float64
    else:
        assert isinstance(got.sums, np.ndarray) and isinstance(got.vt, np.ndarray)
    assert tuple(got.sums.shape) == (6, kw["radius"][1], kw["sectors"])
    assert_same(got, want_sums, want, f"{name} {np.dtype(dtype).name} {path} {route}")
    if name == "antimeridian":   # the centre in its other form: the same spec, the same sums
        twin = wind_polar(put(w), tie_points(name), keep=put(keep), **pc.ANTIMERIDIAN_TWIN)
        assert twin.spec == got.spec and np.array_equal(host(twin.sums), want_sums)
    if name == "offscene":  # no keep: the NULL pointer's path
        assert np.array_equal(host(wind_polar(put(w), tie_points(name), **kw).sums), pref.sums(w, *pc.ties(name), **kw))
    if name == "quadrants":
        ok = want_sums[0] > 0
        a = host(got.inflow_angle)
        assert np.isnan(a[~ok]).all() and np.abs(a[ok] - np.degrees(np.arctan2(-want["vr"][ok], want["vt"][ok]))).max() < 1e-9  # the one value not pinned
        prof, ref = got.ring_profile(), WindPolar(np.array(want_sums), got.spec).ring_profile()
        assert all(pref.same_bits(prof[k], ref[k]) for k in ref) and got.vmax_rmax() == WindPolar(np.array(want_sums), got.spec).vmax_rmax()
        assert got.vmax_rmax()[0] == 200.0 and pref.same_bits(got.wind_radii((5.0, 14.0)), WindPolar(np.array(want_sums), got.spec).wind_radii((5.0, 14.0)))


# ---------------------------------------------------------------------------------------------------------------------- codes
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_polar_from_codes(torch, path, name, route):
    inc, raw, lut, wh = codes_scene()
    _, keep = pc.scene()
    kw = pc.spec(name)
    want_sums = pref.sums(wh, *pc.ties(name), **kw, keep=keep)
    assert want_sums[0].sum() > dict(quadrants=15000, fine=15000, axes=8000, offscene=1500, antimeridian=400)[name]
    put = on(torch, route)
    codes = CopolCodes(put(inc), up(torch, raw.view(np.int32)) if route == "device" else np.array(raw), lut)
    got = codes.polar(tie_points(name), keep=put(keep), **kw)
    assert (hasattr(got.sums, "is_cuda") and got.sums.is_cuda) == (route == "device")
    assert_same(got, want_sums, pref.finish(want_sums), f"codes {name} {path} {route}")
    other = wind_polar(put(wh), tie_points(name), keep=put(keep), **kw)   # the complex128 expansion
    assert np.array_equal(host(other.sums), host(got.sums))


# --------------------------------------------------------------------------------------------------------------------- strips
STRIP_POLAR = dict(centre=(179.88013, 9.80007), radius=(25.0, 6), sectors=8)


@functools.lru_cache(maxsize=None)
def strip_want():
    """tests/test_gpu_grid.py's raster beyond one strip and two workgroup columns, in coarse rings: every workgroup merges through
    its table and the strips meet in global memory."""
    w, keep, ties, _ = strip_case()
    want = pref.sums(w, *ties, **STRIP_POLAR, keep=keep)
    assert (want[0] > 256).sum() >= 30 and want[0].sum() > 0.7 * w.size
    return want


def test_beyond_one_strip_and_one_workgroup_column(torch, path):
    w, keep, ties, _ = strip_case()
    want = strip_want()
    lines, samples = w.shape
    gx, gy, lpb = launch_of(lines, samples)
    assert gx == 3 and samples % 256 and gy >= 2 and lines % lpb and 1400 < lines < 1600 and 600 < samples < 800, (gx, gy, lpb)
    got = wind_polar(up(torch, w), TiePoints(*ties), keep=up(torch, keep), **STRIP_POLAR)
    assert_same(got, want, pref.finish(want), f"strips {path}")


# --------------------------------------------------------------------------------------------------------------- accumulating
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", ["quadrants", "fine"])
def test_accumulating_in_any_order(torch, path, name, route):
    from test_grid_cpu import second_scene
    a, keep = pc.scene()
    b, ties_b = second_scene()
    kw = pc.spec(name)
    put = on(torch, route)
    tp_a, tp_b = tie_points(name), TiePoints(*ties_b)
    whole, fields = pc.case(name)
    want = pref.sums(b, *ties_b, **kw, into=whole.copy())
    assert want[0].sum() > whole[0].sum() + 5000
    ab = wind_polar(put(b), tp_b, into=wind_polar(put(a), tp_a, keep=put(keep), **kw), **kw)
    first = wind_polar(put(b), tp_b, **kw)
    ba = wind_polar(put(a), tp_a, keep=put(keep), into=first, **kw)
    assert ba is first
    assert_same(ab, want, pref.finish(want), f"A then B, {name} {path} {route}")
    assert_same(ba, want, pref.finish(want), f"B then A, {name} {path} {route}")
    # the two row halves of one scene, each with its own lines; then merged from two results, in either order
    top = wind_polar(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), **kw)
    both = wind_polar(put(a[48:]), tp_a, line=np.arange(48, pc.L), keep=put(keep[48:]), into=top, **kw)
    assert_same(both, whole, fields, f"row halves, {name} {path} {route}")
    bottom_first = wind_polar(put(a[48:]), tp_a, line=np.arange(48, pc.L), keep=put(keep[48:]), **kw)
    wind_polar(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), into=bottom_first, **kw)
    assert_same(bottom_first, whole, fields, f"row halves the other way, {name} {path} {route}")
    lower = wind_polar(put(a[48:]), tp_a, line=np.arange(48, pc.L), keep=put(keep[48:]), **kw)
    upper = wind_polar(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), **kw)
    assert host(lower.sums)[5].max() != host(upper.sums)[5].max()
    upper += lower
    assert_same(upper, whole, fields, f"merged halves, {name} {path} {route}")


# --------------------------------------------------------------------------------------------------------- further properties
def test_keep_alone_empties_a_bin(torch, path):
    w, keep = pc.scene()
    kw = pc.spec("quadrants")
    p = pc.pixels("quadrants")
    whole, _ = pc.case("quadrants")
    kk, ss = np.unravel_index(np.argmax(whole[0]), whole[0].shape)
    k2 = np.array(keep)
    k2[p["ok"] & (p["kr"] == kk) & (p["sector"] == ss)] = False
    want = pref.sums(w, *pc.ties("quadrants"), **kw, keep=k2)
    assert whole[0][kk, ss] > 2000 and want[0][kk, ss] == 0 and (want[0] > 0).sum() == (whole[0] > 0).sum() - 1 and (want[:, kk, ss] == 0).all()
    for put in (on(torch, "device"), on(torch, "numpy")):
        got = wind_polar(put(w), tie_points("quadrants"), keep=put(k2), **kw)
        assert_same(got, want, pref.finish(want), "keep")
        assert host(got.count)[kk, ss] == 0 and np.isnan(host(got.vt)[kk, ss]) and np.isnan(host(got.vmax)[kk, ss])


def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):
    """`wind` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns while the
    producer is still in flight and its sums are those of the filled values."""
    dev = torch.device("cuda", 0)
    name = "axes"
    w, keep = pc.scene()
    want, fields = pc.case(name)
    kw = pc.spec(name)
    decoy = np.where(np.isnan(w.real), w, w * 0.5)
    assert not np.array_equal(pref.sums(decoy, *pc.ties(name), **kw, keep=keep), want)
    tp = tie_points(name)
    buf, src, tk = up(torch, decoy), up(torch, w), up(torch, keep)
    wind_polar(src, tp, keep=tk, **kw)   # once on landed values: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = wind_polar(buf, tp, keep=tk, **kw)
        vt, vmax = out.vt, out.vmax
        _in_flight(done)
        got = _read_back(torch, P, out.sums, vt, vmax)
    assert np.array_equal(got[0], want) and pref.same_bits(got[1], fields["vt"]) and pref.same_bits(got[2], fields["vmax"])


def test_bad_path_and_mixed_containers_are_refused(torch, monkeypatch):
    w, keep = pc.scene()
    tp = tie_points("quadrants")
    kw = pc.spec("quadrants")
    host_result = lambda: WindPolar(np.zeros((6, 6, 4), np.int64), PolarSpec(**kw))
    with pytest.raises(ValueError, match="container kind"):
        wind_polar(up(torch, w), tp, keep=keep, **kw)
    with pytest.raises(ValueError, match="container kind"):
        wind_polar(up(torch, w), tp, into=host_result(), **kw)
    with pytest.raises(ValueError, match="container kind"):
        host_result().merge(wind_polar(up(torch, w), tp, **kw))
    monkeypatch.setenv("XSW_GRID_PATH", "lanes")
    with pytest.raises(ValueError, match="XSW_GRID_PATH"):
        wind_polar(up(torch, w), tp, **kw)


def test_raw_entry_refusals_and_host_sums_are_accumulated_into(monkeypatch):
    """The raw entry on host buffers: `sums` is copied up, accumulated into and copied down -- planes 0-4 added to, plane 5 raised
    to the maximum; bad arguments give XSW_EINVAL and leave `sums` alone, a bad XSW_GRID_PATH among them (read by the library at
    every call)."""
    monkeypatch.delenv("XSW_GRID_PATH", raising=False)
    ctx = _lib.default_context(0)
    name = "quadrants"
    w, keep = pc.scene()
    kw = pc.spec(name)
    want, _ = pc.case(name)
    (lon_c, lat_c), (dr, n_r), n_theta = kw["centre"], kw["radius"], kw["sectors"]
    cos_c, sin_c, ssin, scos = pref.tables(lat_c, n_theta)
    tl, ts, lon, lat, heading = pc.ties(name)
    tie = pref.tie_tables(tl, ts, lon, lat, heading, np.arange(float(pc.L)), np.arange(float(pc.S)))
    tables = [np.ascontiguousarray(a, np.float64) for a in tie[:4]]
    br = [np.ascontiguousarray(a, t) for a, t in zip(tie[4:], (np.int32, np.float64, np.int32, np.float64))]
    borders = [np.ascontiguousarray(ssin), np.ascontiguousarray(scos)]
    k8 = np.ascontiguousarray(keep).view(np.uint8)
    floor = int(np.median(want[5][want[5] > 0]))     # between the largest speeds of the bins: some keep it, some exceed it
    sums = np.full((6, n_r, n_theta), 7, np.int64)
    sums[5] = floor
    start = sums.copy()
    expect = want + 7
    expect[5] = np.maximum(want[5], floor)
    assert (want[5] > floor).any() and (want[5] < floor).any()

    def args(**o):
        t = [None] * 4 if o.get("no_ties") else [a.ctypes.data for a in tables]
        b = [None] * 2 if o.get("no_borders") else [a.ctypes.data for a in borders]
        return (pc.L, pc.S, _lib.MEM_HOST, o.get("kind", _lib.CELLS_C128), w.ctypes.data, k8.ctypes.data, len(tl), len(ts), *t, *[a.ctypes.data for a in br],
                o.get("lon_c", lon_c), o.get("lat_c", lat_c), cos_c, sin_c, o.get("dr", dr), o.get("n_r", n_r), o.get("n_theta", n_theta), *b, sums.ctypes.data)
    for bad in (dict(dr=0.0), dict(dr=-1.0), dict(dr=float("nan")), dict(lat_c=89.5), dict(lat_c=float("nan")), dict(lon_c=float("inf")), dict(n_r=0),
                dict(n_theta=0), dict(n_theta=6), dict(n_theta=364), dict(kind=3), dict(no_ties=True), dict(no_borders=True)):
        with pytest.raises(_lib.XswError):
            ctx.wind_polar_raw(*args(**bad))
    monkeypatch.setenv("XSW_GRID_PATH", "lanes")
    with pytest.raises(_lib.XswError, match="XSW_GRID_PATH"):
        ctx.wind_polar_raw(*args())
    assert np.array_equal(sums, start)
    monkeypatch.delenv("XSW_GRID_PATH")
    ctx.wind_polar_raw(*args())
    assert np.array_equal(sums, expect)
