"""xsarsea_amd.centre on the MI355X against its CPU restatement (tests/centre_ref.py).  Every comparison is bit for bit: the int64
`sums` equal, and every finished field through `cells_ref.same_bits`.  The scene and the cases are tests/centre_cases.py's, which
asserts what each case is there for on the restatement before anything runs here; each runs from complex128, complex64 and
co-pol codes, on the staged path and on the direct one (XSW_CENTRE_PATH, read at every call), through device tensors and through
numpy arrays.  The restatement has neither the staged path's cull nor its pre-test on the squared radius."""
import functools
import warnings

import numpy as np
import pytest

import centre_cases as cc
import centre_ref as cref
import polar_cases as pc
import polar_ref as pref
from test_gpu_grid import codes_scene, host, launch_of, on, strip_case, up
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from xsarsea_amd import CentreScores, TiePoints, _lib, find_centre, wind_centre_scores, windspeed
from xsarsea_amd.centre import CentreSpec
from xsarsea_amd.windspeed.crosspol import CopolCodes

pytestmark = pytest.mark.gpu

FIELDS = cref.NAMES


@pytest.fixture(params=["staged", "direct"])
def path(request, monkeypatch):
    if request.param == "staged":
        monkeypatch.delenv("XSW_CENTRE_PATH", raising=False)
    else:
        monkeypatch.setenv("XSW_CENTRE_PATH", request.param)
    return request.param


def tie_points(name):
    return TiePoints(*cc.ties(name))


def assert_same(got, want_sums, want_fields, what):
    s = host(got.sums)
    assert s.dtype == np.int64 and np.array_equal(s, want_sums), f"{what}: {int((s != want_sums).sum())} sums differ"
    for name in FIELDS:
        g = host(got[name])
        assert pref.same_bits(g, want_fields[name]), f"{what} {name}: {int((g != want_fields[name]).sum())} candidates differ (NaN counted)"


# ------------------------------------------------------------------------------------------------------------ complex sources
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_wind_centre_scores(torch, path, name, dtype, route):
    w, keep = pc.scene(dtype)
    want_sums, want = cc.case(name, dtype)
    kw = cc.spec(name)
    put = on(torch, route)
    got = wind_centre_scores(put(w), tie_points(name), keep=put(keep), **kw)
    if route == "device":
        assert isinstance(got.sums, torch.Tensor) and got.sums.is_cuda and got.sums.dtype == torch.int64 and got.vt.is_cuda and got.vt.dtype == torch.float64
    else:
        assert isinstance(got.sums, np.ndarray) and isinstance(got.vt, np.ndarray)
    assert tuple(got.sums.shape) == (5, kw["n"], kw["n"])
    assert_same(got, want_sums, want, f"{name} {np.dtype(dtype).name} {path} {route}")
    if name == "one_antimeridian":   # the first guess in its other form: the same spec
        assert got.spec == CentreSpec(**cc.spec("one_antimeridian_twin"))
    if name == "offscene":  # no keep: the NULL pointer's path
        assert np.array_equal(host(wind_centre_scores(put(w), tie_points(name), **kw).sums), cref.sums(w, *cc.ties(name), **kw))
    if name in ("small", "ring", "offscene"):   # the choice, from device sums as from host sums
        for criterion in ("vt", "calm", "steady"):
            fix = got.best(criterion)
            assert (fix.i, fix.j, fix.score) == cref.best(want_sums, kw["first_guess"][1], criterion), criterion


@pytest.mark.parametrize("name", cc.ONES)
def test_one_candidate_equals_wind_polar_added_over_sectors(torch, path, name):
    """The device's own wind_polar, one ring of r_out_km: its planes 0-4 added over the sectors."""
    from xsarsea_amd import wind_polar
    w, keep = pc.scene()
    kw = cc.spec(name)
    got = wind_centre_scores(up(torch, w), tie_points(name), keep=up(torch, keep), **kw)
    ring = wind_polar(up(torch, w), tie_points(name), keep=up(torch, keep), centre=kw["first_guess"], radius=(kw["annulus"][1], 1), sectors=8)
    assert np.array_equal(host(got.sums)[:, 0, 0], host(ring.sums)[:5, 0, :].sum(axis=1)) and host(got.count)[0, 0] > 300


# ---------------------------------------------------------------------------------------------------------------------- codes
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_centre_scores_from_codes(torch, path, name, route):
    inc, raw, lut, wh = codes_scene()
    _, keep = pc.scene()
    kw = cc.spec(name)
    want_sums = cref.sums(wh, *cc.ties(name), **kw, keep=keep)
    assert want_sums[0].sum() > 100
    put = on(torch, route)
    codes = CopolCodes(put(inc), up(torch, raw.view(np.int32)) if route == "device" else np.array(raw), lut)
    got = codes.centre_scores(tie_points(name), keep=put(keep), **kw)
    assert (hasattr(got.sums, "is_cuda") and got.sums.is_cuda) == (route == "device")
    assert_same(got, want_sums, cref.finish(want_sums), f"codes {name} {path} {route}")
    other = wind_centre_scores(put(wh), tie_points(name), keep=put(keep), **kw)   # the complex128 expansion
    assert np.array_equal(host(other.sums), host(got.sums))


# --------------------------------------------------------------------------------------------------------------------- strips
STRIP_CENTRE = dict(first_guess=(179.88013, 9.80007), step_km=12.0, n=5, annulus=(2.0, 10.0))


@functools.lru_cache(maxsize=None)
def strip_want():
    """tests/test_gpu_grid.py's raster beyond one strip and two workgroup columns: the lattice's square lies across several
    strips and all three workgroup columns, most workgroups stage nothing, and the strips meet in global memory."""
    w, keep, ties, _ = strip_case()
    want = cref.sums(w, *ties, **STRIP_CENTRE, keep=keep)
    lon_g, lat_g = STRIP_CENTRE["first_guess"]
    p = cref.pixel_chart(*pref.gref.geolocate(*pref.tie_tables(*ties, np.arange(float(w.shape[0])), np.arange(float(w.shape[1])))), w, keep, lon_g, lat_g,
                         *pref.tables(lat_g, 4)[:2])
    with np.errstate(invalid="ignore"):
        staged = p["ok"] & (np.abs(p["x"]) < 34.0) & (np.abs(p["y"]) < 34.0)
    rows, cols = np.nonzero(staged.any(axis=1))[0], np.nonzero(staged.any(axis=0))[0]
    assert (want[0] > 5000).all() and 0.05 * w.size < staged.sum() < 0.3 * w.size
    assert rows[-1] - rows[0] > 5 * 32 and cols[0] < 256 and cols[-1] >= 512 and rows[0] > 64 and rows[-1] < w.shape[0] - 64
    return want


def test_beyond_one_strip_and_one_workgroup_column(torch, path):
    w, keep, ties, _ = strip_case()
    want = strip_want()
    lines, samples = w.shape
    gx, gy, lpb = launch_of(lines, samples)
    assert gx == 3 and samples % 256 and gy >= 2 and lines % lpb and lpb <= 64 and 1400 < lines < 1600 and 600 < samples < 800, (gx, gy, lpb)
    got = wind_centre_scores(up(torch, w), TiePoints(*ties), keep=up(torch, keep), **STRIP_CENTRE)
    assert_same(got, want, cref.finish(want), f"strips {path}")


# --------------------------------------------------------------------------------------------------------------- accumulating
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", ["small", "ring"])
def test_accumulating_in_any_order(torch, path, name, route):
    from test_grid_cpu import second_scene
    a, keep = pc.scene()
    b, ties_b = second_scene()
    kw = cc.spec(name)
    put = on(torch, route)
    tp_a, tp_b = tie_points(name), TiePoints(*ties_b)
    whole, fields = cc.case(name)
    want = cref.sums(b, *ties_b, **kw, into=whole.copy())
    ab = wind_centre_scores(put(b), tp_b, into=wind_centre_scores(put(a), tp_a, keep=put(keep), **kw), **kw)
    first = wind_centre_scores(put(b), tp_b, **kw)
    ba = wind_centre_scores(put(a), tp_a, keep=put(keep), into=first, **kw)
    assert ba is first
    assert_same(ab, want, cref.finish(want), f"A then B, {name} {path} {route}")
    assert_same(ba, want, cref.finish(want), f"B then A, {name} {path} {route}")
    # the two row halves of one scene, each with its own lines; then merged from two results, in either order
    top = wind_centre_scores(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), **kw)
    assert 0 < host(top.count).sum() < whole[0].sum()
    both = wind_centre_scores(put(a[48:]), tp_a, line=np.arange(48, pc.L), keep=put(keep[48:]), into=top, **kw)
    assert_same(both, whole, fields, f"row halves, {name} {path} {route}")
    bottom_first = wind_centre_scores(put(a[48:]), tp_a, line=np.arange(48, pc.L), keep=put(keep[48:]), **kw)
    wind_centre_scores(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), into=bottom_first, **kw)
    assert_same(bottom_first, whole, fields, f"row halves the other way, {name} {path} {route}")
    lower = wind_centre_scores(put(a[48:]), tp_a, line=np.arange(48, pc.L), keep=put(keep[48:]), **kw)
    upper = wind_centre_scores(put(a[:48]), tp_a, line=np.arange(48), keep=put(keep[:48]), **kw)
    upper += lower
    assert_same(upper, whole, fields, f"merged halves, {name} {path} {route}")


# --------------------------------------------------------------------------------------------------------- further properties
def test_keep_alone_empties_a_candidate(torch, path):
    name = "ring"
    w, keep = pc.scene()
    kw = cc.spec(name)
    whole, _ = cc.case(name)
    p = cc.pixels(name)
    i, j = 0, kw["n"] - 1                       # the south-east corner of the lattice
    off = cref.lattice(kw["n"], kw["step_km"])
    hit, _, _ = cref.candidate(p, off[j], off[i], *kw["annulus"])
    k2 = np.array(keep)
    k2[hit] = False
    want = cref.sums(w, *cc.ties(name), **kw, keep=k2)
    assert whole[0][i, j] > 100 and want[0][i, j] == 0 and (want[:, i, j] == 0).all() and (want[0] > 0).sum() == kw["n"] ** 2 - 1
    for put in (on(torch, "device"), on(torch, "numpy")):
        got = wind_centre_scores(put(w), tie_points(name), keep=put(k2), **kw)
        assert_same(got, want, cref.finish(want), "keep")
        assert host(got.count)[i, j] == 0 and np.isnan(host(got.vt)[i, j]) and np.isnan(host(got.wspd)[i, j])
        fix = got.best("vt", min_coverage=0.0)
        assert (fix.i, fix.j) != (i, j) and (fix.i, fix.j, fix.score) == cref.best(want, kw["first_guess"][1], "vt", 0.0)


def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):
    """`wind` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns while the
    producer is still in flight and its sums are those of the filled values."""
    dev = torch.device("cuda", 0)
    name = "wide"
    w, keep = pc.scene()
    want, fields = cc.case(name)
    kw = cc.spec(name)
    decoy = np.where(np.isnan(w.real), w, w * 0.5)
    assert not np.array_equal(cref.sums(decoy, *cc.ties(name), **kw, keep=keep), want)
    tp = tie_points(name)
    buf, src, tk = up(torch, decoy), up(torch, w), up(torch, keep)
    wind_centre_scores(src, tp, keep=tk, **kw)   # once on landed values: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = wind_centre_scores(buf, tp, keep=tk, **kw)
        vt, wspd = out.vt, out.wspd
        _in_flight(done)
        got = _read_back(torch, P, out.sums, vt, wspd)
    assert np.array_equal(got[0], want) and pref.same_bits(got[1], fields["vt"]) and pref.same_bits(got[2], fields["wspd"])


def test_bad_path_and_mixed_containers_are_refused(torch, monkeypatch):
    w, keep = pc.scene()
    tp = tie_points("small")
    kw = cc.spec("small")
    host_result = lambda: CentreScores(np.zeros((5, 9, 9), np.int64), CentreSpec(**kw))
    with pytest.raises(ValueError, match="container kind"):
        wind_centre_scores(up(torch, w), tp, keep=keep, **kw)
    with pytest.raises(ValueError, match="container kind"):
        wind_centre_scores(up(torch, w), tp, into=host_result(), **kw)
    with pytest.raises(ValueError, match="container kind"):
        host_result().merge(wind_centre_scores(up(torch, w), tp, **kw))
    monkeypatch.setenv("XSW_CENTRE_PATH", "staged")
    with pytest.raises(ValueError, match="XSW_CENTRE_PATH"):
        wind_centre_scores(up(torch, w), tp, **kw)


def test_raw_entry_refusals_and_host_sums_are_added_to(monkeypatch):
    """The raw entry on host buffers: `sums` is copied up, added to and copied down; bad arguments give XSW_EINVAL and leave
    `sums` alone, a bad XSW_CENTRE_PATH among them (read by the library at every call)."""
    monkeypatch.delenv("XSW_CENTRE_PATH", raising=False)
    ctx = _lib.default_context(0)
    name = "ring"
    w, keep = pc.scene()
    kw = cc.spec(name)
    want, _ = cc.case(name)
    (lon_g, lat_g), step, n, (r_in, r_out) = kw["first_guess"], kw["step_km"], kw["n"], kw["annulus"]
    cos_g, sin_g = pref.tables(lat_g, 4)[:2]
    tl, ts, lon, lat, heading = cc.ties(name)
    tie = pref.tie_tables(tl, ts, lon, lat, heading, np.arange(float(pc.L)), np.arange(float(pc.S)))
    tables = [np.ascontiguousarray(a, np.float64) for a in tie[:4]]
    br = [np.ascontiguousarray(a, t) for a, t in zip(tie[4:], (np.int32, np.float64, np.int32, np.float64))]
    k8 = np.ascontiguousarray(keep).view(np.uint8)
    sums = np.full((5, n, n), 7, np.int64)
    sums[3] = -(2 ** 40)                       # a negative start: the adds are two's complement
    start = sums.copy()

    def args(**o):
        t = [None] * 4 if o.get("no_ties") else [a.ctypes.data for a in tables]
        return (pc.L, pc.S, _lib.MEM_HOST, o.get("kind", _lib.CELLS_C128), None if o.get("no_src") else w.ctypes.data, k8.ctypes.data, len(tl), len(ts), *t,
                *[a.ctypes.data for a in br], o.get("lon_g", lon_g), o.get("lat_g", lat_g), cos_g, sin_g, o.get("step", step), o.get("n", n),
                o.get("r_in", r_in), o.get("r_out", r_out), None if o.get("no_sums") else sums.ctypes.data)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(n=0), dict(n=8), dict(n=33), dict(n=-1), dict(step=0.0), dict(step=-1.0), dict(step=nan), dict(step=inf), dict(r_in=-1.0), dict(r_in=nan),
                dict(r_out=inf), dict(r_out=nan), dict(r_in=8.0), dict(r_in=9.0), dict(lat_g=89.5), dict(lat_g=nan), dict(lon_g=inf), dict(kind=3),
                dict(no_ties=True), dict(no_src=True), dict(no_sums=True)):
        with pytest.raises(_lib.XswError):
            ctx.wind_centre_raw(*args(**bad))
    monkeypatch.setenv("XSW_CENTRE_PATH", "lds")
    with pytest.raises(_lib.XswError, match="XSW_CENTRE_PATH"):
        ctx.wind_centre_raw(*args())
    assert np.array_equal(sums, start)
    monkeypatch.delenv("XSW_CENTRE_PATH")
    ctx.wind_centre_raw(*args())
    assert np.array_equal(sums, want + start)
    # one candidate: step_km is not read, whatever it holds
    one = np.zeros((5, 1, 1), np.int64)
    kw1 = cc.spec("one_axes")
    a = list(args(step=nan, n=1, r_in=kw1["annulus"][0], r_out=kw1["annulus"][1]))
    a[-1] = one.ctypes.data
    ctx.wind_centre_raw(*a)
    assert np.array_equal(one, cc.case("one_axes")[0])


# ------------------------------------------------------------------------------------------------------------ the vortex, from codes
@functools.lru_cache(maxsize=None)
def vortex_codes():
    """The vortex of tests/centre_cases.py as co-pol codes: sigma0 simulated from it on the LUT, inverted with the vortex as the
    a-priori wind.  (inc, raw codes, LUT, the codes' complex128 expansion on the host, tie arguments, the vortex's guess)."""
    w, ties, guess = cc.vortex(cc.TRUE_OFFSETS[0])
    inc = np.ascontiguousarray(np.broadcast_to(np.linspace(30.0, 40.0, pc.S), w.shape))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sigma0 = windspeed.simulate_sigma0(inc, wind=np.array(w), model="gmf_cmod5n", units="linear", resolution="low")
        codes = windspeed.invert_copol_codes(inc, sigma0, ancillary_wind=np.array(w), model="gmf_cmod5n", resolution="low")
    raw = host(codes.codes).view(np.uint32).copy()
    wh = host(CopolCodes(inc, raw, codes.lut_co).wind())
    assert (~np.isnan(wh.real)).mean() > 0.99 and np.nanmax(np.abs(wh - w)) < 6.0
    return inc, raw, codes.lut_co, wh, ties, guess


@pytest.mark.parametrize("route", ["device", "numpy"])
def test_find_centre_from_codes_lands_on_the_vortex(torch, path, route):
    inc, raw, lut, wh, ties, guess = vortex_codes()
    offset = cc.TRUE_OFFSETS[0]
    lon, lat = cref.inverse_chart(guess, 1.0, 31)
    start = (float(lon[15 + 4, 15 - 5]), float(lat[15 + 4, 15 - 5]))        # 10 km from the truth, as tests/test_centre_cpu.py starts
    put = on(torch, route)
    codes = CopolCodes(put(inc), up(torch, raw.view(np.int32)) if route == "device" else np.array(raw), lut)
    fix = codes.find_centre(TiePoints(*ties), first_guess=start, steps_km=(4.0, 1.0), n=9, annulus=(4.0, 9.0))
    # the same search on the restatement of the codes' expansion
    g = start
    for level, step in zip(fix.levels, (4.0, 1.0)):
        s = cref.sums(wh, *ties, first_guess=g, step_km=step, n=9, annulus=(4.0, 9.0))
        i, j, score = cref.best(s, g[1], "vt")
        glon, glat = cref.inverse_chart(g, step, 9)
        assert (level.i, level.j, level.score, level.lon, level.lat) == (i, j, score, float(glon[i, j]), float(glat[i, j]))
        g = (level.lon, level.lat)
    assert len(fix.levels) == 2 and (fix.lon, fix.lat) == g and not fix.on_border
    x, y = pref.chart(np.array(fix.lon), np.array(fix.lat), guess[0], guess[1], *pref.tables(guess[1], 4)[:2])
    assert max(abs(float(x) - offset[0]), abs(float(y) - offset[1])) < 1e-3                # the node tests/test_centre_cpu.py lands on
    # and straight from the complex expansion
    direct = find_centre(put(wh), TiePoints(*ties), first_guess=start, steps_km=(4.0, 1.0), n=9, annulus=(4.0, 9.0))
    assert (direct.lon, direct.lat, direct.i, direct.j, direct.score) == (fix.lon, fix.lat, fix.i, fix.j, fix.score)
