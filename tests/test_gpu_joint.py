"""GPU: the joint dual-pol inversion from stored co-pol codes (xsw_joint_from_codes, kernel k_joint_from_codes; `CopolCodes.joint`,
`invert_joint`).

The yardstick everywhere is the dense numpy restatement tests/joint_ref.py (held to the kernel's exactness claim by
tests/test_joint_cpu.py): the joint codes and all four cost rasters must equal it bit for bit, NaN positions and gate codes
included (float32 outputs: the restatement rounded once).  sigma0 is handed in dB (sigma0_is_db), so that the restatement sees
the very values the kernel computes with; where a test hands linear rasters, their dB value is test_gpu_cost_codes._db's.

The input codes come from one xsw_invert launch (mono co-pol) unless a test says otherwise."""
import warnings

import numpy as np
import pytest

import joint_ref as jref
from test_gpu_codes import _device_run
from test_gpu_cost_codes import _db, _differ, _fill
from test_gpu_crosspol_codes import _scene
from test_gpu_streams import ASYNC, _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from test_gpu_uncertainty import _synthetic_luts
from test_joint_cpu import constant_tables, tie_scene
from util import lut_dicts, small_luts

from conftest import golden
from oracle import invert as oinv
from oracle import lut as olut

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output raster
SENTINEL = {np.float32: np.float32(-7.5e37), np.float64: np.float64(-7.5e300)}  # no cost (>= 0 or NaN)
CODE_SENTINEL = 0x12345678
SCALAR = 0.125  # dsig_cr_scalar: exact in float32 and float64, so one restatement serves both raster dtypes


def _joint(ctx, torch, _lib, arrs, out_t, want=(1, 1, 1, 1, 1), mem=None, dsig_co=0.1, is_db=True):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays): arrs = (inc, code_co, sigma0_co, anc, sigma0_cr, dsig_cr or
    None).  Every requested output lies between two guard regions and starts as a sentinel: returns [code uint32, J, Jwind,
    Jsig_co, Jsig_cr] host arrays (None where not requested) after checking that the guards are untouched and every pixel written."""
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    hosts = [None if a is None else np.ascontiguousarray(a if n else np.zeros(1, a.dtype)) for a in arrs]  # (an empty raster: no pointer is NULL)
    host_route = mem == _lib.MEM_HOST
    sents = [CODE_SENTINEL] + [SENTINEL[out_t]] * 4
    types = [np.int32] + [out_t] * 4
    if host_route:
        bufs = [np.full(n + 2 * GUARD, s, t) if w else None for w, s, t in zip(want, sents, types)]
        ins = [None if a is None else a.ctypes.data for a in hosts]
        outs = [None if b is None else b.ctypes.data + GUARD * b.itemsize for b in bufs]
    else:
        dev = torch.device("cuda", 0)
        keep = [None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in hosts]
        tt = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
        bufs = [torch.full((n + 2 * GUARD,), s if t == np.int32 else float(s), dtype=tt[t], device=dev) if w else None for w, s, t in zip(want, sents, types)]
        torch.cuda.synchronize()
        ins = [None if t is None else t.data_ptr() for t in keep]
        outs = [None if b is None else b.data_ptr() + GUARD * b.element_size() for b in bufs]
    ctx.joint_from_codes_raw(shape[0], shape[1], dt, od, _lib.MEM_HOST if host_route else _lib.MEM_DEVICE, *ins, *outs, dsig_co=dsig_co,
                             dsig_cr_scalar=SCALAR, sigma0_is_db=is_db)
    ctx.synchronize()
    res = []
    for b, s in zip(bufs, sents):
        if b is None:
            res.append(None)
            continue
        h = b if host_route else b.cpu().numpy()
        assert np.all(h[:GUARD] == s) and np.all(h[-GUARD:] == s), "a guard region was written"
        assert not np.any(h[GUARD:-GUARD] == s), "a pixel was not written"
        h = h[GUARD:-GUARD].reshape(shape).copy()
        res.append(h.view(np.uint32) if h.dtype == np.int32 else h)
    return res


def _assert_equal(got, want, out_t, what):
    """The codes and every requested cost raster == the restatement's (rounded once to a float32 output), NaN positions included."""
    counts = {}
    if got[0] is not None:
        counts["code"] = int(np.sum(got[0] != want["code"]))
    for k, g in zip(jref.FIELDS, got[1:]):
        if g is not None:
            with np.errstate(all="ignore"):
                counts[k] = _differ(g, want[k].astype(out_t))
    print(f"{what}: pixels that differ from the restatement {counts}")
    assert not any(counts.values()), f"{what}: {counts}"


def _mono_codes(ctx, torch, _lib, inc, s_co_db, anc):
    """The co-pol codes of one xsw_invert launch on device rasters (sigma0 in dB)."""
    return _device_run(ctx, torch, _lib, (inc, s_co_db, None, None, anc), np.complex128, {"codes"}, is_db=True)["cc"].cpu().numpy().view(np.uint32)


def _flat(code):
    return code.astype(np.int64) & 0x3FFFFFFF


def _install(ctx, lco, lcr):
    co, cr = lut_dicts(lco, lcr)
    ctx.upload_luts(co=co, cr=cr)
    return oinv.Prepared(lco, lcr)


@pytest.fixture
def default_ctx(gpu_ctx, default_luts):
    _install(gpu_ctx, *default_luts)
    return gpu_ctx


@pytest.fixture
def lowres_ctx(gpu_ctx, lowres_luts):
    _install(gpu_ctx, *lowres_luts)
    return gpu_ctx


@pytest.fixture(scope="module")
def lowres_tab(lowres_luts):
    return oinv.Prepared(*lowres_luts)


# ------------------------------------------------------------------------------------------------ the recipe on the default tables
@pytest.fixture(scope="module")
def recipe_scene(gpu_ctx, torch, default_luts):
    """12 x 333 pixels of the section's recipe as float32 rasters (their float64 upcast holds the same values, so ONE restatement
    per dsig_cr kind serves all four dtype pairs), the co-pol codes of one xsw_invert launch, and the two restatements: 3.6e8
    dense scores each."""
    from xsarsea_amd import _lib
    p = _install(gpu_ctx, *default_luts)
    shape = (12, 333)
    sc = tuple(a.reshape(shape) for a in jref.recipe(np.random.default_rng(23), shape[0] * shape[1], p, np.float32))
    inc, s_co, s_cr, dsig, anc = sc
    cc = _mono_codes(gpu_ctx, torch, _lib, inc, s_co, anc)
    assert np.all(cc < 0x80000000), "a recipe pixel has no co-pol solution"
    want = {"raster": jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p), "scalar": jref.joint(cc, inc, s_co, anc, 0.1, s_cr, SCALAR, p)}
    return p, sc, cc, want


@pytest.mark.parametrize("kind", ["raster", "scalar"])
@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_recipe_scene_bit_equal_to_the_restatement(default_ctx, torch, recipe_scene, dtype, out_t, kind):
    from xsarsea_amd import _lib
    p, sc, cc, want = recipe_scene
    # the classes that make the comparison meaningful, first (tests/test_joint_cpu.py measures 0.90 and 0.037 on its 1500 pixels)
    w = want["raster"]
    differ = np.mean(_flat(w["code"]) != _flat(cc))
    below = np.mean(p.wspd_dim[_flat(w["code"]) // p.phi_dim.size] < p.wspd_cr[0])
    print(f"joint point != co-pol point: {differ:.3f}; on a speed row below wcr[0]: {below:.3f}")
    assert differ >= 0.5 and below >= 0.01
    inc, s_co, s_cr, dsig, anc = (a.astype(np.complex128 if np.iscomplexobj(a) else np.float64) if dtype == np.float64 else a for a in sc)
    cc_here = _mono_codes(default_ctx, torch, _lib, inc, s_co, anc)
    assert np.array_equal(cc_here, cc), "the co-pol codes depend on the raster dtype although the values are the same"
    got = _joint(default_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig if kind == "raster" else None), out_t)
    _assert_equal(got, want[kind], out_t, f"recipe, {np.dtype(dtype).name} -> {np.dtype(out_t).name}, dsig_cr {kind}")


def test_linear_sigma0_goes_through_the_kernels_own_db(default_ctx, torch, recipe_scene):
    """sigma0_is_db = 0 on a crop: the restatement is handed test_gpu_cost_codes._db of the linear rasters."""
    from xsarsea_amd import _lib
    p, sc, cc, _ = recipe_scene
    k = (slice(0, 2), slice(0, 130))
    inc, s_co, s_cr, dsig, anc = (a[k] for a in sc)
    lin_co, lin_cr = (10.0 ** (s_co.astype(np.float64) / 10.0)).astype(np.float32), (10.0 ** (s_cr.astype(np.float64) / 10.0)).astype(np.float32)
    codes = np.ascontiguousarray(cc[k])
    got = _joint(default_ctx, torch, _lib, (inc, codes, lin_co, anc, lin_cr, dsig), np.float64, is_db=False)
    _assert_equal(got, jref.joint(codes, inc, _db(lin_co, False), anc, 0.1, _db(lin_cr, False), dsig, p), np.float64, "linear float32 sigma0")


# ------------------------------------------------------------------------------------------------ other tables
@pytest.mark.parametrize("scale", [1.0, 0.3, 2.5])
@pytest.mark.parametrize("tag", ["phi180_f64", "phi360_f64", "phi90_f64"])
def test_small_goldens(gpu_ctx, torch, tag, scale):
    """Every pixel of the 24 x 40 scenes on 0..180, 0..360 and 0..90 direction axes: the windows reach the axis ends and the 0..360
    seam; a-priori x 0.3 and x 2.5: large windows.  Every input class of the scenes goes through the gates."""
    from xsarsea_amd import _lib
    d = golden(f"kernel_small_{tag}.npz")
    p = _install(gpu_ctx, *small_luts(d))
    inc, dsig, anc = np.ascontiguousarray(d["inc"]), np.ascontiguousarray(d["dsig_cr"]), np.ascontiguousarray(d["anc"]) * scale
    s_co, s_cr = oinv.to_db(d["sigma0_vv"]), oinv.to_db(d["sigma0_vh"])
    cc = _mono_codes(gpu_ctx, torch, _lib, inc, s_co, anc)
    want = jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p)
    searched = np.isfinite(want["Jsig_cr"])
    assert searched.sum() > 400 and np.mean(_flat(want["code"])[searched] != _flat(cc)[searched]) > 0.2
    if tag != "phi90_f64":
        assert np.any((want["code"][searched] >> 30) & 1) and np.any(~((want["code"][searched] >> 30) & 1).astype(bool)), "one value of the -phi bit only"
    _assert_equal(_joint(gpu_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), np.float64), want, np.float64, f"{tag}, a-priori x {scale}")


def test_nonuniform_table_takes_the_whole_grid(gpu_ctx, torch):
    """Non-uniform axes (no box: !prunable): the whole 11 x 9 grid per pixel, the cross-pol cell by the axis search; the input codes
    are arbitrary grid codes, since the co-pol search itself is not under test here."""
    from xsarsea_amd import _lib
    lco, lcr = _synthetic_luts(11, 9, 13)
    p = _install(gpu_ctx, lco, lcr)
    rng = np.random.default_rng(5)
    shape = (3, 150)
    inc = rng.uniform(15.0, 50.0, shape)
    wspd, phi = rng.uniform(0.2, 5.5, shape), rng.uniform(0.0, 180.0, shape)
    s_co = -22.0 + 9.0 * np.log10(1.0 + wspd) + 2.0 * np.cos(np.deg2rad(2.0 * phi)) + 0.3 * rng.standard_normal(shape)
    dsig = rng.uniform(0.1, 1.0, shape)
    s_cr = -36.0 + 12.0 * np.log10(1.0 + wspd) + dsig * rng.standard_normal(shape)
    anc = wspd * rng.uniform(0.6, 1.5, shape) * np.exp(1j * np.deg2rad(phi + 25.0 * rng.standard_normal(shape)))
    cc = rng.integers(0, 11 * 9, shape).astype(np.uint32)
    want = jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p)
    assert np.mean(_flat(want["code"]) != _flat(cc)) > 0.5 and len(np.unique(_flat(want["code"]))) > 20
    _assert_equal(_joint(gpu_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), np.float64), want, np.float64, "non-uniform table")


def test_ties_go_to_the_smallest_flat_index(gpu_ctx, torch):
    """Constant tables and a zero a-priori wind: every direction of the best speed row ties; the answer is its direction 0."""
    from xsarsea_amd import _lib
    for slope, s_cr_db, d_cr, row in ((0.0, -29.0, 0.5, 0), (2.0, -20.0, 0.25, 14)):
        p = _install(gpu_ctx, *constant_tables(slope_cr=slope))
        cc, inc, s_co, s_cr, dsig, anc = (a.reshape(1, 4) for a in tie_scene(p.phi_dim.size, s_cr_db, d_cr))
        want = jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p)
        assert np.all(want["code"] == row * p.phi_dim.size)
        _assert_equal(_joint(gpu_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), np.float64), want, np.float64, f"tie, best row {row}")


# ------------------------------------------------------------------------------------------------ gates, shapes, outputs, routes
def _lowres_scene(ctx, torch, _lib, p, shape, seed, dtype=np.float64):
    """Recipe pixels on the low-resolution tables with their xsw_invert codes: (inc, code_co, s_co_db, anc, s_cr_db, dsig_cr)."""
    inc, s_co, s_cr, dsig, anc = (a.reshape(shape) for a in jref.recipe(np.random.default_rng(seed), shape[0] * shape[1], p, dtype))
    if inc.size == 0:
        return inc, np.zeros(shape, np.uint32), s_co, anc, s_cr, dsig
    return inc, _mono_codes(ctx, torch, _lib, inc, s_co, anc), s_co, anc, s_cr, dsig


def test_infinite_dsig_cr_returns_the_input_codes(lowres_ctx, torch, lowres_tab):
    from xsarsea_amd import _lib
    inc, cc, s_co, anc, s_cr, _ = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (3, 333), 31)
    dsig = np.full(inc.shape, np.inf)
    got = _joint(lowres_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), np.float64)
    assert np.array_equal(got[0], cc) and np.all(got[4] == 0.0)
    _assert_equal(got, jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, lowres_tab), np.float64, "dsig_cr = inf")


def test_gates(lowres_ctx, torch, lowres_tab):
    """Every gate of rule 6 next to searched pixels, in one wave and across waves."""
    from xsarsea_amd import _lib
    p = lowres_tab
    inc, cc, s_co, anc, s_cr, dsig = _lowres_scene(lowres_ctx, torch, _lib, p, (2, 150), 37)
    plane = p.wspd_dim.size * p.phi_dim.size
    cc[0, 3], cc[0, 4], cc[0, 5], cc[0, 6], cc[0, 7] = _lib.CODE_NAN, _lib.CODE_NAN_RE, 0x80000005, plane, 0x40000000 | plane
    inc[0, 10] = np.nan    # NaN incidence next to a grid code
    inc[0, 4] = np.nan     # ... and next to XSW_CODE_NAN_RE
    s_cr[0, 20] = np.nan   # no cross-pol information
    dsig[1, 21] = np.nan
    s_co[0, 30] = np.nan   # J_ub not finite
    anc[1, 31] = np.nan
    anc[1, 32] = complex(3.0, np.nan)
    dsig[0, 33] = 0.0
    s_cr[1, 34] = np.inf
    s_co[1, 149] = np.nan  # in the last lane of the raster
    want = jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, p)
    assert list(want["code"][0, 3:8]) == [_lib.CODE_NAN, _lib.CODE_NAN_RE, _lib.CODE_NAN_RE, _lib.CODE_NAN_RE, _lib.CODE_NAN_RE] and want["code"][0, 10] == _lib.CODE_NAN_RE
    assert want["code"][0, 20] == cc[0, 20] and want["code"][1, 21] == cc[1, 21] and np.isnan(want["Jsig_cr"][0, 20]) and np.isfinite(want["J"][0, 20])
    assert all(want["code"][k] == _lib.CODE_NAN for k in ((0, 30), (1, 31), (1, 32), (0, 33), (1, 34), (1, 149)))
    assert np.isfinite(want["J"]).sum() > 250
    for out_t in (np.float64, np.float32):
        _assert_equal(_joint(lowres_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), out_t), want, out_t, f"gates -> {np.dtype(out_t).name}")


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 65), (3, 64), (5, 257), (0, 64)])
def test_small_shapes(lowres_ctx, torch, lowres_tab, shape):
    """One lane, one lane short of a wave, one past it, whole waves, one lane past a 256-pixel block, and no pixel at all (the
    call returns and writes nothing)."""
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, shape, 41)
    if shape[0] == 0:
        for mem in (None, _lib.MEM_HOST):
            assert all(g.shape == shape for g in _joint(lowres_ctx, torch, _lib, arrs, np.float64, mem=mem))
        return
    inc, cc, s_co, anc, s_cr, dsig = arrs
    _assert_equal(_joint(lowres_ctx, torch, _lib, arrs, np.float64), jref.joint(cc, inc, s_co, anc, 0.1, s_cr, dsig, lowres_tab), np.float64, f"{shape}")


def test_nullable_outputs(lowres_ctx, torch, lowres_tab):
    """Each output alone and each one left out: what is written equals the all-five run bit for bit, and (inside _joint) nothing is
    written outside the requested rasters."""
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (2, 200), 43, np.float32)
    full = _joint(lowres_ctx, torch, _lib, arrs, np.float32)
    same = lambda a, b: np.array_equal(a, b) if a.dtype == np.uint32 else _differ(a, b) == 0
    for k in range(5):
        alone = tuple(int(j == k) for j in range(5))
        got = _joint(lowres_ctx, torch, _lib, arrs, np.float32, want=alone)
        assert [g is not None for g in got] == [bool(w) for w in alone] and same(got[k], full[k]), f"output {k} alone"
        got = _joint(lowres_ctx, torch, _lib, arrs, np.float32, want=tuple(1 - w for w in alone))
        assert got[k] is None and all(same(g, f) for j, (g, f) in enumerate(zip(got, full)) if j != k), f"without output {k}"


def test_host_route_equals_device_route(lowres_ctx, torch, lowres_tab):
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (3, 333), 47, np.float32)
    for out_t, sub in ((np.float32, arrs), (np.float64, arrs[:5] + (None,))):
        a = _joint(lowres_ctx, torch, _lib, sub, out_t)
        b = _joint(lowres_ctx, torch, _lib, sub, out_t, mem=_lib.MEM_HOST)
        assert np.array_equal(a[0], b[0]) and all(_differ(x, y) == 0 for x, y in zip(a[1:], b[1:])) and np.isfinite(a[1]).all()


def test_statistics_count_the_scored_candidates(lowres_ctx, torch, lowres_tab):
    """xsw_stats_enable: pixels searched and candidates scored; between one candidate per pixel and the whole grid."""
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (3, 333), 49)
    lowres_ctx.stats_enable(True)
    try:
        _joint(lowres_ctx, torch, _lib, arrs, np.float64)
        s = lowres_ctx.stats()
    finally:
        lowres_ctx.stats_enable(False)
    plane = lowres_tab.wspd_dim.size * lowres_tab.phi_dim.size
    assert s["pixels_co"] == 999 and 999 <= s["cand_co"] <= 999 * plane


def test_error_codes(torch, lowres_luts):
    """XSW_ENOLUT (-3) without both tables, XSW_EINVAL (-1) otherwise, each with a message and before any launch: the output keeps
    its fill."""
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a, z = np.full((2, 8), 33.0, np.float32), np.full((2, 8), 5 + 1j, np.complex64)
        c, o = np.zeros((2, 8), np.uint32), np.full((2, 8), 77, np.uint32)
        p = lambda x: None if x is None else x.ctypes.data
        msg = lambda: ctx._lib.xsw_last_error(ctx._h).decode()

        def call(ins=(a, c, a, z), cr=a, outs=(o, None, None, None, None), dsig_co=0.1, shape=(2, 8), dtype=0, mem=0):
            return ctx._lib.xsw_joint_from_codes(ctx._h, *shape, dtype, 0, mem, 1, *(p(x) for x in ins), dsig_co, p(cr), None, 0.1, *(p(x) for x in outs))
        lut_co, lut_cr = lut_dicts(*lowres_luts)
        assert call() == -3 and "LUT" in msg()
        ctx.upload_luts(cr=lut_cr)
        assert call() == -3
        ctx.upload_luts(co=lut_co)
        assert call() == 0
        o[...] = 77
        assert call(outs=(None,) * 5) == -1 and "no output" in msg()
        for k in range(4):
            assert call(ins=tuple(None if j == k else x for j, x in enumerate((a, c, a, z)))) == -1 and "NULL" in msg()
        assert call(cr=None) == -1 and "NULL" in msg()
        assert call(dsig_co=0.0) == -1 and "dsig_co" in msg()
        assert call(dsig_co=float("nan")) == -1 and "dsig_co" in msg()
        assert call(dtype=7) == -1 and call(mem=9) == -1 and call(shape=(-1, 8)) == -1
        assert call(shape=(1 << 31, 1 << 31)) == -1 and "too large" in msg()
        assert call(shape=(0, 8)) == 0
        # a table with a non-finite entry is refused, co-pol or cross-pol
        lco, lcr = constant_tables()
        bad = np.array(lco.values, copy=True)
        bad[1, 2, 3] = np.nan
        co_bad, cr_ok = lut_dicts(olut.Lut(bad, lco.incidence, lco.wspd, lco.phi, "dB", "x", "co", "VV"), lcr)
        ctx.upload_luts(co=co_bad, cr=cr_ok)
        assert call() == -1 and "NaN or infinite" in msg()
        badr = np.array(lcr.values, copy=True)
        badr[0, 1] = np.inf
        co_ok, cr_bad = lut_dicts(lco, olut.Lut(badr, lcr.incidence, lcr.wspd, None, "dB", "x", "cr", "VH"))
        ctx.upload_luts(co=co_ok, cr=cr_bad)
        assert call() == -1 and "NaN or infinite" in msg()
        ctx.synchronize()
        assert np.all(o == 77), "a refused call wrote its output"
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public calls
@pytest.mark.parametrize("container", ["numpy", "torch"])
def test_public_api(gpu_ctx, torch, container):
    """cc.joint == the restatement on the rasters the engine forms (raster and scalar dsig_cr, details, out_dtype); `.wind()` of the
    result == xsw_expand_codes of the restatement's codes; invert_joint == the two calls; `.cost` works on the result."""
    from xsarsea_amd import windspeed
    from xsarsea_amd.windspeed import _engine, get_model
    sc = _scene((12, 333), np.float32, 41)
    h_inc, h_vv, h_vh, h_dsig, h_anc = sc
    if container == "torch":
        dev = torch.device("cuda", 0)
        sc = tuple(torch.from_numpy(a).to(dev) for a in sc)
    inc, s_vv, s_vh, dsig, anc = sc
    host = lambda x: x.cpu().numpy() if container == "torch" else x
    # numpy rasters: float32 sigma0 goes to dB by numpy's own log10 on the host; device rasters: by the kernel
    to_db = (lambda x: _db(x, False)) if container == "torch" else (lambda x: oinv.to_db(x).astype(np.float64))
    co_kw, cr_kw = dict(model="gmf_cmod5n", resolution="low"), dict(model="gmf_s1_v2", resolution="low")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, dsig_co=0.2, **co_kw)
        lut_co, lut_cr = cc.lut_co, _engine.lut_source(get_model("gmf_s1_v2"), dict(resolution="low"))
        p = oinv.Prepared(lut_co, lut_cr)
        codes = host(cc.codes).view(np.uint32)
        for d, h_d in ((dsig, h_dsig), (0.1, _fill(h_vh, 0.1))):
            want = jref.joint(codes, h_inc, to_db(h_vv), h_anc, 0.2, to_db(h_vh), h_d, p)
            assert np.isfinite(want["J"]).sum() > 2000 and np.any(want["code"] == 0xFFFFFFFE) and np.any(want["code"] == 0xFFFFFFFF)
            out = cc.joint(s_vv, anc, s_vh, dsig_cr=d, **cr_kw)
            assert isinstance(out, windspeed.CopolCodes) and out.on_device == (container == "torch") and out.dsig_co == 0.2
            assert np.array_equal(host(out.codes).view(np.uint32), want["code"]), f"{container} joint codes, dsig_cr {'raster' if d is dsig else d}"
        det = cc.joint(s_vv, anc, s_vh, dsig_cr=dsig, details=True, out_dtype=np.float32, **cr_kw)
        want = jref.joint(codes, h_inc, to_db(h_vv), h_anc, 0.2, to_db(h_vh), h_dsig, p)
        _assert_equal([host(det.codes.codes).view(np.uint32)] + [host(det[k]) for k in jref.FIELDS], want, np.float32, f"{container} details")
        assert all(host(det[k]).dtype == np.float32 for k in jref.FIELDS)
        # the winds: what xsw_expand_codes makes of the restatement's codes
        wind = host(det.codes.wind())
        ref_wind = _engine.expand_codes(lut_co, None, want["code"], None)[0]
        assert _differ(wind.real.astype(np.float64), ref_wind.real.astype(wind.real.dtype).astype(np.float64)) == 0
        assert _differ(wind.imag.astype(np.float64), ref_wind.imag.astype(wind.imag.dtype).astype(np.float64)) == 0
        both = windspeed.invert_joint(inc, s_vv, s_vh, ancillary_wind=anc, dsig_co=0.2, dsig_cr=dsig, model=("gmf_cmod5n", "gmf_s1_v2"), resolution="low")
        assert _differ(host(both).real.astype(np.float64), wind.real.astype(np.float64)) == 0 and _differ(host(both).imag.astype(np.float64), wind.imag.astype(np.float64)) == 0
        # the result is a CopolCodes like any other: its co-pol cost at the joint point is the joint cost's co-pol part
        cost = det.codes.cost(s_vv, anc, out_dtype=np.float32)
        assert _differ(host(cost.Jwind), host(det.Jwind)) == 0
        searched = np.isfinite(want["J"])
        assert _differ(host(cost.Jsig)[searched], host(det.Jsig_co)[searched]) == 0


def test_user_stream_without_an_intermediate_sync(gpu_ctx, torch, delay_cycles):  # noqa: F811
    """invert_copol_codes and .joint(details=True) back to back on a user stream whose producer is held back: both return while it
    is in flight, the result is consumed on that stream and equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _scene((48, 260), np.float32, 51), _scene((48, 260), np.float32, 52)
    kw = dict(model="gmf_cmod5n", resolution="low", **ASYNC)
    cr = dict(model="gmf_s1_v2", resolution="low")

    def call(b):
        cc = windspeed.invert_copol_codes(b[0], b[1], ancillary_wind=b[4], **kw)
        j = cc.joint(b[1], b[4], b[2], dsig_cr=b[3], details=True, **cr)
        return j.codes.codes, j.J, j.Jsig_cr

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = _staged(torch, list(sc), list(dec))
        ref = call([src for _, src in pairs])  # landed rasters, synchronised: LUTs installed, work lists sized
        torch.cuda.synchronize()
        ref = [r.cpu().numpy() for r in ref]
        wrong = [r.cpu().numpy() for r in call([buf for buf, _ in pairs])]  # the decoy scene: what a read that overtakes the producer gives
        assert _differ(wrong[1], ref[1]) > 1000
        P = torch.cuda.Stream(device=torch.device("cuda", 0))
        with torch.cuda.stream(P):
            done = _held_back(torch, P, delay_cycles, pairs)
            res = call([buf for buf, _ in pairs])
            _in_flight(done)
            got = _read_back(torch, P, *res)
    assert not np.isnan(ref[1]).all() and np.array_equal(got[0], ref[0]) and _differ(got[1], ref[1]) == 0 and _differ(got[2], ref[2]) == 0
