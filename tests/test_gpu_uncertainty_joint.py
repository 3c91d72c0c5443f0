"""GPU: the error bars of the joint dual-pol solution from stored grid codes (xsw_uncertainty_joint_from_codes, kernel k_unc_joint;
`CopolCodes.uncertainty_joint`).

The yardstick everywhere is the numpy restatement tests/uncertainty_joint_ref.py (its stencil pinned to the dense joint cost by
tests/test_uncertainty_joint_cpu.py).  The six real outputs and the flags must equal it bit for bit, NaN positions included;
float32 outputs are the restatement rounded once.  Only IEEE + - * / sqrt in float64 follow the table reads, so there is no
tolerance.  sigma0 is handed in dB (sigma0_is_db), so that the restatement sees the very values the kernel computes with; where a
test hands linear rasters, their dB value is test_gpu_cost_codes._db's."""
import warnings

import numpy as np
import pytest

import joint_ref as jref
import uncertainty_joint_ref as ujref
import uncertainty_ref as uref
from test_gpu_cost_codes import _db, _differ, _fill
from test_gpu_crosspol_codes import _scene
from test_gpu_joint import _install, _joint, _lowres_scene, _mono_codes, default_ctx, lowres_ctx, lowres_tab  # noqa: F401 (fixtures)
from test_gpu_streams import ASYNC, _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from test_gpu_uncertainty import TABLES, _table_luts, _unc
from util import lut_dicts

from oracle import invert as oinv

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output raster
SENTINEL = {np.float32: np.float32(-7.5e37), np.float64: np.float64(-7.5e300), np.uint8: np.uint8(0xA5)}  # no std, correlation or flag
FIELDS = ujref.FIELDS + ("flag",)
SCALAR = 0.125  # dsig_cr_scalar: exact in float32 and float64, so one restatement serves both raster dtypes


def _uj(ctx, torch, _lib, arrs, out_t, want=(1,) * 7, mem=None, dsig_co=0.1, is_db=True):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays): arrs = (inc, code, sigma0_co, anc, sigma0_cr, dsig_cr or
    None).  Every requested output lies between two guard regions and starts as its sentinel: returns [wspd_std, dir_std, corr,
    u_std, v_std, corr_uv, flag] host arrays (None where not requested) after checking that the guards are untouched and every
    pixel was written."""
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    types = [out_t] * 6 + [np.uint8]
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    hosts = [None if a is None else np.ascontiguousarray(a if n else np.zeros(1, a.dtype)) for a in arrs]  # (an empty raster: no pointer is NULL)
    host_route = mem == _lib.MEM_HOST
    if host_route:
        bufs = [np.full(n + 2 * GUARD, SENTINEL[t], t) if w else None for t, w in zip(types, want)]
        ins = [None if a is None else a.ctypes.data for a in hosts]
        outs = [None if b is None else b.ctypes.data + GUARD * b.itemsize for b in bufs]
    else:
        dev = torch.device("cuda", 0)
        tt = {np.float32: torch.float32, np.float64: torch.float64, np.uint8: torch.uint8}
        keep = [None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in hosts]
        bufs = [torch.full((n + 2 * GUARD,), SENTINEL[t].item(), dtype=tt[t], device=dev) if w else None for t, w in zip(types, want)]
        torch.cuda.synchronize()
        ins = [None if t is None else t.data_ptr() for t in keep]
        outs = [None if b is None else b.data_ptr() + GUARD * b.element_size() for b in bufs]
    ctx.uncertainty_joint_from_codes_raw(shape[0], shape[1], dt, od, _lib.MEM_HOST if host_route else _lib.MEM_DEVICE, *ins, *outs,
                                         dsig_co=dsig_co, dsig_cr_scalar=SCALAR, sigma0_is_db=is_db)
    ctx.synchronize()
    res = []
    for b, t in zip(bufs, types):
        if b is None:
            res.append(None)
            continue
        h = b if host_route else b.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL[t]) and np.all(h[-GUARD:] == SENTINEL[t]), "a guard region was written"
        assert not np.any(h[GUARD:n + GUARD] == SENTINEL[t]), "a pixel was not written"
        res.append(h[GUARD:n + GUARD].reshape(shape).copy())
    return res


def _assert_fields(got, want, out_t, what):
    """Every requested field == the restatement's (reals rounded once to a float32 output), NaN positions included."""
    counts = {}
    for k, g in zip(FIELDS, got):
        if g is not None:
            with np.errstate(all="ignore"):
                counts[k] = _differ(g, want[k] if k == "flag" else want[k].astype(out_t))
            assert g.dtype == (np.uint8 if k == "flag" else out_t)
    print(f"{what}: pixels that differ from the restatement {counts}")
    assert not any(counts.values()), f"{what}: {counts}"


def _same(a, b):
    return all((x is None and y is None) or _differ(x, y) == 0 for x, y in zip(a, b))


def _ref(p, arrs, dsig_co=0.1):
    """The restatement of arrs = (inc, code, s_co_db, anc, s_cr_db, dsig_cr or None: SCALAR in the raster dtype)."""
    inc, code, s_co, anc, s_cr, dsig = arrs
    return ujref.unc_joint(code, inc, s_co, anc, dsig_co, s_cr, _fill(s_cr, SCALAR) if dsig is None else dsig, p)


# ------------------------------------------------------------------------------------------------ the recipe on the default tables
@pytest.fixture(scope="module")
def recipe_scene(gpu_ctx, torch, default_luts):
    """12 x 333 pixels of section 19's recipe as float32 rasters (their float64 upcast holds the same values, so ONE restatement per
    dsig_cr kind serves all four dtype pairs), the joint codes xsw_joint_from_codes itself returns for them (from the co-pol codes
    of one xsw_invert launch, which are kept too), and the restatements at the joint codes."""
    from xsarsea_amd import _lib
    p = _install(gpu_ctx, *default_luts)
    shape = (12, 333)
    sc = tuple(a.reshape(shape) for a in jref.recipe(np.random.default_rng(23), shape[0] * shape[1], p, np.float32))
    inc, s_co, s_cr, dsig, anc = sc
    cc = _mono_codes(gpu_ctx, torch, _lib, inc, s_co, anc)
    jc = _joint(gpu_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), np.float64, want=(1, 0, 0, 0, 0))[0]
    assert np.all(cc < 0x80000000) and np.all(jc < 0x80000000), "a recipe pixel has no solution"
    want = {"raster": _ref(p, (inc, jc, s_co, anc, s_cr, dsig)), "scalar": _ref(p, (inc, jc, s_co, anc, s_cr, None))}
    return p, sc, cc, jc, want


def _assert_recipe_conditions(p, sc, jc, want):
    """What makes the comparison meaningful, from the restatement alone (tests/test_uncertainty_joint_cpu.py measures 0.982 and
    0.977 on its 600 pixels): most pixels have an estimate, and it is not the co-pol one."""
    inc, s_co, s_cr, dsig, anc = sc
    co = uref.unc_co(jc, inc, s_co, anc, 0.1, p)
    est, both = want["flag"] == 0, (want["flag"] == 0) & (co["flag"] == 0)
    smaller = np.mean(want["wspd_std"][both] < co["wspd_std"][both])
    print(f"estimate on {est.mean():.3f} of the pixels; joint wspd_std below the co-pol stencil's on {smaller:.3f} of the {both.sum()} with both; "
          f"median {np.median(want['wspd_std'][both]):.2f} against {np.median(co['wspd_std'][both]):.2f} m/s")
    assert est.mean() >= 0.75 and smaller >= 0.5


@pytest.mark.parametrize("kind", ["raster", "scalar"])
@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_recipe_scene_bit_equal_to_the_restatement(default_ctx, torch, recipe_scene, dtype, out_t, kind):  # noqa: F811
    from xsarsea_amd import _lib
    p, sc, _, jc, want = recipe_scene
    _assert_recipe_conditions(p, sc, jc, want["raster"])
    inc, s_co, s_cr, dsig, anc = (a.astype(np.complex128 if np.iscomplexobj(a) else np.float64) if dtype == np.float64 else a for a in sc)
    got = _uj(default_ctx, torch, _lib, (inc, jc, s_co, anc, s_cr, dsig if kind == "raster" else None), out_t)
    _assert_fields(got, want[kind], out_t, f"recipe, joint codes, {np.dtype(dtype).name} -> {np.dtype(out_t).name}, dsig_cr {kind}")


def test_recipe_scene_from_plain_copol_codes(default_ctx, torch, recipe_scene):  # noqa: F811
    """Any grid code of the tables comes in: the co-pol search's own, where the centre of the stencil need not be its smallest."""
    from xsarsea_amd import _lib
    p, (inc, s_co, s_cr, dsig, anc), cc, jc, _ = recipe_scene
    assert np.mean((cc & 0x3FFFFFFF) != (jc & 0x3FFFFFFF)) >= 0.5
    arrs = (inc, cc, s_co, anc, s_cr, dsig)
    want = _ref(p, arrs)
    assert np.mean(want["flag"] == 0) > 0.5
    _assert_fields(_uj(default_ctx, torch, _lib, arrs, np.float64), want, np.float64, "recipe, co-pol codes")


def test_linear_sigma0_goes_through_the_kernels_own_db(default_ctx, torch, recipe_scene):  # noqa: F811
    """sigma0_is_db = 0 on a crop: the restatement is handed test_gpu_cost_codes._db of the linear rasters."""
    from xsarsea_amd import _lib
    p, sc, _, jc, _ = recipe_scene
    k = (slice(0, 2), slice(0, 130))
    inc, s_co, s_cr, dsig, anc = (a[k] for a in sc)
    lin_co, lin_cr = (10.0 ** (s_co.astype(np.float64) / 10.0)).astype(np.float32), (10.0 ** (s_cr.astype(np.float64) / 10.0)).astype(np.float32)
    codes = np.ascontiguousarray(jc[k])
    got = _uj(default_ctx, torch, _lib, (inc, codes, lin_co, anc, lin_cr, dsig), np.float64, is_db=False)
    want = _ref(p, (inc, codes, _db(lin_co, False), anc, _db(lin_cr, False), dsig))
    assert np.mean(want["flag"] == 0) > 0.5
    _assert_fields(got, want, np.float64, "linear float32 sigma0")


# ------------------------------------------------------------------------------------------------ every grid point of a table
@pytest.mark.parametrize("name", TABLES)
def test_every_grid_point(gpu_ctx, torch, name):
    """Code rasters that enumerate every (iw, ip) x both values of bit 30 x three incidences (below the axis, between two nodes, at
    the last node), as tests/test_gpu_uncertainty.py does: every border and corner combination, on the three small goldens'
    tables, a non-uniform table and shapes where every point is a border.  sigma0 and the a-priori follow the code's own grid
    point smoothly, so that interior points are mostly convex."""
    from xsarsea_amd import _lib
    lco, lcr = _table_luts(name)
    p = _install(gpu_ctx, lco, lcr)
    n_w, n_phi = len(lco.wspd), len(lco.phi)
    plane = n_w * n_phi
    ax = np.asarray(lco.incidence, dtype=np.float64)
    incs = [ax[0] - 1.0, 0.5 * (ax[0] + ax[1]) + 0.3 * (ax[1] - ax[0]), ax[-1]]
    shape = (6, plane)
    flat = np.arange(plane, dtype=np.uint32)
    code = np.stack([flat | np.uint32(bit << 30) for _ in incs for bit in (0, 1)])
    inc = np.repeat(np.array(incs), 2)[:, None] * np.ones((1, plane))
    iw, ip = np.divmod(np.arange(plane), n_phi)
    j = (np.arange(6) // 2)[:, None] * plane + np.arange(plane)[None, :]  # the two rows of a bit-30 pair see the same rasters
    i_inc = np.argmin(np.abs(ax[None, :] - np.array(incs)[:, None]), axis=1).repeat(2)
    s_co = lco.values[i_inc[:, None], iw[None, :], ip[None, :]] + 0.05 * np.sin(0.37 * j)
    w, phi = np.asarray(lco.wspd)[iw], np.asarray(lco.phi)[ip]
    anc = (w * np.exp(1j * np.deg2rad(phi)))[None, :] * (1.0 + 0.02 * np.cos(0.11 * j)) + 0.1j * np.sin(0.23 * j)
    i_inc_cr = np.argmin(np.abs(np.asarray(lcr.incidence)[None, :] - np.array(incs)[:, None]), axis=1).repeat(2)
    wcr = np.asarray(lcr.wspd, dtype=np.float64)
    at_w = np.stack([np.interp(w, wcr, lcr.values[k]) if wcr.size > 1 else np.full(w.shape, lcr.values[k, 0]) for k in i_inc_cr])
    s_cr = at_w + 0.05 * np.sin(0.29 * j)
    dsig = 0.1 + 0.05 * (1.0 + np.sin(0.13 * j))
    degenerate = name.startswith("degenerate")

    arrs = (inc, code, s_co, anc, s_cr, dsig)
    got = _uj(gpu_ctx, torch, _lib, arrs, np.float64)
    _assert_fields(got, _ref(p, arrs), np.float64, name)
    on_w, on_p = (iw == 0) | (iw == n_w - 1), (ip == 0) | (ip == n_phi - 1)
    assert np.array_equal(got[6] & 6, np.broadcast_to(2 * on_w + 4 * on_p, shape)) and not np.any(got[6] & 17)
    if degenerate:
        assert np.all(got[6] != 0) and all(np.isnan(g).all() for g in got[:6])
    else:
        seen = set(got[6].ravel().tolist())
        assert {0, 2, 4, 6} <= seen and np.mean(got[6][:, ~(on_w | on_p)] == 0) > 0.5, seen
        for k in (0, 1, 2, 3, 4):
            assert _differ(got[k][0], got[k][1]) == 0  # bit 30 enters corr_uv alone,
        assert _differ(got[5][0], -got[5][1]) == 0 and np.any(got[5][0] != 0)  # as its sign
        # ... and the cross-pol term is in it: the co-pol error bars differ
        co = _unc(gpu_ctx, torch, _lib, "co", (inc, code, s_co, anc), np.float64, True)
        both = (got[6] == 0) & (co[3] == 0)
        assert both.sum() > 10 and np.mean(got[0][both] != co[0][both]) > 0.5


# ------------------------------------------------------------------------------------------------ the rules, one by one
def test_infinite_dsig_cr_is_the_copol_pass(lowres_ctx, torch, lowres_tab):  # noqa: F811
    """Jsig_cr = 0 exactly: xsw_uncertainty_from_codes' outputs of the same rasters bit for bit, bit 16 clear."""
    from xsarsea_amd import _lib
    inc, cc, s_co, anc, s_cr, _ = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (3, 333), 31)
    arrs = (inc, cc, s_co, anc, s_cr, np.full(inc.shape, np.inf))
    got = _uj(lowres_ctx, torch, _lib, arrs, np.float64)
    co = _unc(lowres_ctx, torch, _lib, "co", (inc, cc, s_co, anc), np.float64, True)
    assert _same(got[:3] + [got[6]], co) and np.mean(co[3] == 0) > 0.5
    _assert_fields(got, _ref(lowres_tab, arrs), np.float64, "dsig_cr = inf")


def test_rule_cases(lowres_ctx, torch, lowres_tab):  # noqa: F811
    """No cross-pol information (bit 16 and the co-pol pass' real outputs), a stencil that is not finite (NOT_CONVEX), foreign codes
    and a NaN incidence (NO_SOLUTION), next to ordinary pixels in one wave and across waves."""
    from xsarsea_amd import _lib
    p = lowres_tab
    inc, cc, s_co, anc, s_cr, dsig = _lowres_scene(lowres_ctx, torch, _lib, p, (2, 150), 37)
    code = _joint(lowres_ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), np.float64, want=(1, 0, 0, 0, 0))[0]
    base = _ref(p, (inc, code, s_co, anc, s_cr, dsig))
    ok = np.argwhere(base["flag"] == 0)
    assert len(ok) > 200
    at = [tuple(ok[k]) for k in np.linspace(0, len(ok) - 1, 16).astype(int)]
    plane = p.wspd_dim.size * p.phi_dim.size
    s_cr[at[0]], dsig[at[1]] = np.nan, np.nan                                        # no cross-pol information
    dsig[at[2]], s_cr[at[3]], s_cr[at[4]] = 0.0, np.inf, -np.inf                     # J not finite
    s_co[at[5]], anc[at[6]], anc[at[7]] = np.nan, np.nan, complex(3.0, np.nan)
    for k, bad in zip(range(8, 13), (_lib.CODE_NAN, _lib.CODE_NAN_RE, 0x80000005, plane, 0x40000000 | plane)):
        code[at[k]] = bad                                                            # no grid code of this LUT
    inc[at[13]] = np.nan
    inc[at[14]], s_cr[at[14]] = np.nan, np.nan                                       # NO_SOLUTION and no cross-pol information
    arrs = (inc, code, s_co, anc, s_cr, dsig)
    want = _ref(p, arrs)
    flag = [int(want["flag"][a]) for a in at]
    assert flag == [16, 16] + [8] * 6 + [1] * 6 + [17, 0], flag
    assert np.isfinite(want["u_std"][at[0]]) and np.isfinite(want["corr_uv"][at[1]])
    for out_t in (np.float32, np.float64):
        got = _uj(lowres_ctx, torch, _lib, arrs, out_t)
        _assert_fields(got, want, out_t, f"rule cases -> {np.dtype(out_t).name}")
        assert all(np.array_equal(np.isnan(g), (got[6] & 15) != 0) for g in got[:6])
    co = _unc(lowres_ctx, torch, _lib, "co", (inc, code, s_co, anc), np.float64, True)
    for a in at[:2]:  # the co-pol pass' bits
        assert all(np.isfinite(c[a]) and g[a] == c[a] for g, c in zip(got[:3], co[:3]))
    assert np.array_equal(got[6] & 7, co[3] & 7)  # the gates and the borders are that pass' too


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 65), (3, 64), (5, 257), (0, 64)])
def test_small_shapes(lowres_ctx, torch, lowres_tab, shape):  # noqa: F811
    """One lane, one lane short of a wave, one past it, whole waves, one lane past a 256-pixel block, and no pixel at all (the
    call returns and writes nothing)."""
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, shape, 41)
    if shape[0] == 0:
        for mem in (None, _lib.MEM_HOST):
            assert all(g.shape == shape for g in _uj(lowres_ctx, torch, _lib, arrs, np.float64, mem=mem))
        return
    want = _ref(lowres_tab, arrs)
    _assert_fields(_uj(lowres_ctx, torch, _lib, arrs, np.float64), want, np.float64, f"{shape}")
    assert shape == (1, 1) or np.any(want["flag"] == 0)


def test_nullable_outputs(lowres_ctx, torch, lowres_tab):  # noqa: F811
    """Each output alone, each one left out, and a few subsets: what is written equals the all-seven run bit for bit, and (inside
    _uj) nothing is written outside the requested rasters; no output at all is XSW_EINVAL."""
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (2, 200), 43, np.float32)
    full = _uj(lowres_ctx, torch, _lib, arrs, np.float32)
    assert np.any(full[6] == 0) and np.any(full[6] != 0)
    subsets = [tuple(int(j == k) for j in range(7)) for k in range(7)] + [tuple(int(j != k) for j in range(7)) for k in range(7)]
    subsets += [(1, 1, 1, 0, 0, 0, 1), (0, 0, 0, 1, 1, 1, 0), (1, 0, 0, 0, 0, 1, 0), (0, 1, 0, 1, 0, 0, 1), (1,) * 7]
    for want in subsets:
        got = _uj(lowres_ctx, torch, _lib, arrs, np.float32, want=want)
        assert [g is not None for g in got] == [bool(w) for w in want]
        assert _same(got, [g if w else None for g, w in zip(full, want)]), f"outputs {want}"
    with pytest.raises(_lib.XswError, match=r"\(-1\).*no output"):
        _uj(lowres_ctx, torch, _lib, arrs, np.float32, want=(0,) * 7)


def test_host_route_equals_device_route(lowres_ctx, torch, lowres_tab):  # noqa: F811
    from xsarsea_amd import _lib
    arrs = _lowres_scene(lowres_ctx, torch, _lib, lowres_tab, (3, 333), 47, np.float32)
    for out_t, sub, want in ((np.float32, arrs, (1,) * 7), (np.float64, arrs[:5] + (None,), (1, 0, 0, 1, 0, 1, 1))):
        a = _uj(lowres_ctx, torch, _lib, sub, out_t, want=want)
        b = _uj(lowres_ctx, torch, _lib, sub, out_t, want=want, mem=_lib.MEM_HOST)
        assert _same(a, b) and np.mean(a[6] == 0) > 0.5, np.dtype(out_t).name


def test_error_codes(torch, lowres_luts):
    """XSW_ENOLUT (-3) without both tables, XSW_EINVAL (-1) otherwise, each with a message and before any launch: the outputs keep
    their fill.  A table with a non-finite entry is NOT refused: the stencils that touch it are not convex."""
    from test_joint_cpu import constant_tables
    from oracle import lut as olut
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a, z = np.full((2, 8), 33.0, np.float32), np.full((2, 8), 5 + 1j, np.complex64)
        c = np.zeros((2, 8), np.uint32)
        o, fl = np.full((2, 8), 77.0, np.float32), np.full((2, 8), 0xA5, np.uint8)
        p = lambda x: None if x is None else x.ctypes.data
        msg = lambda: ctx._lib.xsw_last_error(ctx._h).decode()

        def call(ins=(a, c, a, z), cr=a, outs=(o, None, None, None, None, None, fl), dsig_co=0.1, shape=(2, 8), dtype=0, mem=0):
            return ctx._lib.xsw_uncertainty_joint_from_codes(ctx._h, *shape, dtype, 0, mem, 1, *(p(x) for x in ins), dsig_co, p(cr), None, 0.1,
                                                             *(p(x) for x in outs))
        lut_co, lut_cr = lut_dicts(*lowres_luts)
        assert call() == -3 and "LUT" in msg()
        ctx.upload_luts(cr=lut_cr)
        assert call() == -3
        ctx.upload_luts(co=lut_co)
        assert call(outs=(None,) * 7) == -1 and "no output" in msg()
        for k in range(4):
            assert call(ins=tuple(None if j == k else x for j, x in enumerate((a, c, a, z)))) == -1 and "NULL" in msg()
        assert call(cr=None) == -1 and "NULL" in msg()
        assert call(dsig_co=0.0) == -1 and "dsig_co" in msg()
        assert call(dsig_co=float("nan")) == -1 and "dsig_co" in msg()
        assert call(dtype=7) == -1 and call(mem=9) == -1 and call(shape=(-1, 8)) == -1
        assert call(shape=(1 << 31, 1 << 31)) == -1 and "too large" in msg()
        assert call(shape=(0, 8)) == 0
        ctx.synchronize()
        assert np.all(o == 77.0) and np.all(fl == 0xA5), "a refused call wrote its output"
        assert call() == 0 and np.all(fl == 6) and np.isnan(o).all()  # code 0: the corner of the grid
        # a NaN in the co-pol table: no refusal; the stencils around it are not convex, the others keep their estimate
        lco, lcr = constant_tables(slope_cr=2.0)
        n_phi = len(lco.phi)
        bad = np.array(lco.values, copy=True)
        bad[:, 6, 5] = np.nan
        co_bad, cr_ok = lut_dicts(olut.Lut(bad, lco.incidence, lco.wspd, lco.phi, "dB", "x", "co", "VV"), lcr)
        ctx.upload_luts(co=co_bad, cr=cr_ok)
        c[...] = 12 * n_phi + 5
        c[0, :3] = [6 * n_phi + 5, 7 * n_phi + 4, 5 * n_phi + 6]
        a[...], z[...] = 30.0, 7.0 * np.exp(1j * np.deg2rad(75.0))
        s_co, s_cr = np.full((2, 8), -12.5, np.float32), np.full((2, 8), -20.0, np.float32)
        assert call(ins=(a, c, s_co, z), cr=s_cr) == 0
        assert list(fl[0, :3]) == [8, 8, 8] and np.all(fl.ravel()[3:] == 0) and np.isfinite(o.ravel()[3:]).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public call
@pytest.mark.parametrize("container", ["numpy", "torch"])
def test_public_api(gpu_ctx, torch, container):
    """cc.joint(...).uncertainty_joint(...) == the raw entry on the rasters the engine forms == the restatement (raster and scalar
    dsig_cr, out_dtype, dsig_co from invert_copol_codes); `.uncertainty` on the same codes is the co-pol pass and differs."""
    from xsarsea_amd import _lib, windspeed
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
    raw_s = (lambda x: (x, False)) if container == "torch" else (lambda x: (oinv.to_db(x), True))
    co_kw, cr_kw = dict(model="gmf_cmod5n", resolution="low"), dict(model="gmf_s1_v2", resolution="low")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cc = windspeed.invert_copol_codes(inc, s_vv, ancillary_wind=anc, dsig_co=0.2, **co_kw)
        best = cc.joint(s_vv, anc, s_vh, dsig_cr=dsig, **cr_kw)
        lut_co, lut_cr = cc.lut_co, _engine.lut_source(get_model("gmf_s1_v2"), dict(resolution="low"))
        p = oinv.Prepared(lut_co, lut_cr)
        codes = host(best.codes).view(np.uint32)
        for d, h_d in ((dsig, h_dsig), (0.1, _fill(h_vh, 0.1))):
            u = best.uncertainty_joint(s_vv, anc, s_vh, dsig_cr=d, **cr_kw)
            assert isinstance(u, windspeed.JointUncertainty) and u["flag"] is u.flag
            got = [host(u[k]) for k in FIELDS]
            assert all(g.shape == (12, 333) for g in got) and [g.dtype for g in got] == [np.float64] * 6 + [np.uint8]
            want = ujref.unc_joint(codes, h_inc, to_db(h_vv), h_anc, 0.2, to_db(h_vh), h_d, p)
            _assert_fields(got, want, np.float64, f"{container} uncertainty_joint, dsig_cr {'raster' if d is dsig else d}")
            assert np.mean(got[6] == 0) > 0.5 and np.any(got[6] & 16) and np.any(got[6] & 1)
        co, cr = lut_dicts(lut_co, lut_cr)
        gpu_ctx.upload_luts(co=co, cr=cr)
        (r_vv, is_db), (r_vh, _) = raw_s(h_vv), raw_s(h_vh)
        u = best.uncertainty_joint(s_vv, anc, s_vh, dsig_cr=dsig, **cr_kw)
        raw = _uj(gpu_ctx, torch, _lib, (h_inc, codes, r_vv, h_anc, r_vh, h_dsig), np.float64, dsig_co=0.2, is_db=is_db)
        assert _same([host(u[k]) for k in FIELDS], raw), "not the raw entry's bits"
        u32 = best.uncertainty_joint(s_vv, anc, s_vh, dsig_cr=dsig, dsig_co=0.1, out_dtype=np.float32, **cr_kw)
        got32 = [host(u32[k]) for k in FIELDS]
        assert got32[3].dtype == np.float32
        _assert_fields(got32, ujref.unc_joint(codes, h_inc, to_db(h_vv), h_anc, 0.1, to_db(h_vh), h_dsig, p), np.float32, f"{container} float32, dsig_co 0.1")
        # `.uncertainty` of the joint codes is the co-pol curvature: the same flags but bit 16 where no cross-pol term entered, other bars
        plain = best.uncertainty(s_vv, anc)
        g, pl = host(u.wspd_std), host(plain.wspd_std)
        both = (host(u.flag) == 0) & (host(plain.flag) == 0)
        assert both.sum() > 1000 and np.mean(g[both] != pl[both]) > 0.9
        nocr = host(u.flag) == 16
        assert nocr.sum() > 10 and _differ(g[nocr], pl[nocr]) == 0


def test_user_stream_without_an_intermediate_sync(gpu_ctx, torch, delay_cycles):  # noqa: F811
    """invert_copol_codes, .joint and .uncertainty_joint back to back on a user stream whose producer is held back: all return while
    it is in flight, the result is consumed on that stream and equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _scene((48, 260), np.float32, 51), _scene((48, 260), np.float32, 52)
    kw = dict(model="gmf_cmod5n", resolution="low", **ASYNC)
    cr = dict(model="gmf_s1_v2", resolution="low")

    def call(b):
        cc = windspeed.invert_copol_codes(b[0], b[1], ancillary_wind=b[4], **kw)
        u = cc.joint(b[1], b[4], b[2], dsig_cr=b[3], **cr).uncertainty_joint(b[1], b[4], b[2], dsig_cr=b[3], **cr)
        return tuple(u[k] for k in FIELDS)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = _staged(torch, list(sc), list(dec))
        ref = call([src for _, src in pairs])  # landed rasters, synchronised: LUTs installed, work lists sized
        torch.cuda.synchronize()
        ref = [r.cpu().numpy() for r in ref]
        wrong = [r.cpu().numpy() for r in call([buf for buf, _ in pairs])]  # the decoy scene: what a read that overtakes the producer gives
        assert _differ(wrong[0], ref[0]) > 1000
        P = torch.cuda.Stream(device=torch.device("cuda", 0))
        with torch.cuda.stream(P):
            done = _held_back(torch, P, delay_cycles, pairs)
            res = call([buf for buf, _ in pairs])
            _in_flight(done)
            got = _read_back(torch, P, *res)
    assert not np.isnan(ref[0]).all() and _same(got, ref)
