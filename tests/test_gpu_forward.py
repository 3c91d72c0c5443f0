"""GPU: the forward operator on rasters (xsw_lut_eval / xsw_lut_eval_cr, kernels k_lut_eval_co / k_lut_eval_cr;
`windspeed.simulate_sigma0`, `LutModel.__call__` on rasters).

The yardstick everywhere is the numpy restatement tests/forward_ref.py (pinned to `LutModel.__call__` by tests/test_forward_cpu.py),
evaluated on the table READ BACK from the context (xsw_lut_read), never on a host-built copy.  Every output must equal it bit for
bit, NaN positions included; float32 outputs are the restatement rounded once.  Only IEEE + - * / in float64 follow the cell
search, so there is no tolerance."""
import itertools
import warnings

import numpy as np
import pytest

import forward_ref as fref
from test_gpu_streams import _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from util import lut_dicts, small_luts

from conftest import golden
from oracle import lut as olut

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output raster
SENTINEL = {np.float32: np.float32(-7.5e37), np.float64: np.float64(-7.5e300)}  # no sigma0 in dB and no slope of a table
MARGINS = (2.5, 1.5, 5.0)  # of `_scene`, beyond the default tables' axes
FIELDS = {"co": ("sigma0_db", "dwspd", "dphi"), "cr": ("sigma0_db", "dwspd")}


def _differ(a, b):
    """Elements whose BITS differ (so +0.0 is not -0.0), but for NaN, which equals NaN whatever its payload."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.dtype in (np.float32, np.float64)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return int(np.sum(~((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b)))))


def _eval(ctx, torch, _lib, kind, arrs, out_t, want=None, mem=None, fold=True):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays).  kind "co": arrs = (inc, wspd, phi) -> [sigma0_db, dwspd,
    dphi]; "cr": (inc, wspd) -> [sigma0_db, dwspd].  Every requested output lies between two guard regions and starts as the
    sentinel; returns host arrays (None where not requested) after checking that the guards are untouched and every pixel was
    written."""
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    want = (1,) * len(FIELDS[kind]) if want is None else want
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    item, sent = np.dtype(out_t).itemsize, SENTINEL[out_t]
    hosts = [np.ascontiguousarray(a if n else np.zeros(1, a.dtype)) for a in arrs]  # an empty raster: no pointer is NULL
    host_route = mem == _lib.MEM_HOST
    if host_route:
        bufs = [np.full(n + 2 * GUARD, sent, out_t) if w else None for w in want]
        ins = [a.ctypes.data for a in hosts]
        outs = [None if b is None else b.ctypes.data + GUARD * item for b in bufs]
    else:
        dev = torch.device("cuda", 0)
        keep = [torch.from_numpy(a).to(dev) for a in hosts]
        bufs = [torch.full((n + 2 * GUARD,), float(sent), dtype=torch.float32 if out_t == np.float32 else torch.float64, device=dev) if w else None
                for w in want]
        torch.cuda.synchronize()
        ins = [t.data_ptr() for t in keep]
        outs = [None if b is None else b.data_ptr() + GUARD * item for b in bufs]
    lines, samples = (shape[0], shape[1]) if len(shape) == 2 else _lib.lines_samples(shape)
    m = _lib.MEM_HOST if host_route else _lib.MEM_DEVICE
    if kind == "co":
        ctx.lut_eval_raw(lines, samples, dt, od, m, *ins, *outs, fold_phi=fold)
    else:
        ctx.lut_eval_cr_raw(lines, samples, dt, od, m, *ins, *outs)
    ctx.synchronize()
    res = []
    for b in bufs:
        if b is None:
            res.append(None)
            continue
        h = b if host_route else b.cpu().numpy()
        assert np.all(h[:GUARD] == sent) and np.all(h[-GUARD:] == sent), "a guard region was written"
        assert not np.any(h[GUARD:n + GUARD] == sent), "a pixel was not written"
        res.append(h[GUARD:n + GUARD].reshape(shape).copy())
    return res


def _assert_fields(kind, got, want, out_t, what):
    """Every requested field == the restatement's (rounded once to a float32 output), NaN positions included."""
    counts = {}
    for k, g in zip(FIELDS[kind], got):
        if g is not None:
            with np.errstate(all="ignore"):
                counts[k] = _differ(g, want[k].astype(out_t))
            assert g.dtype == out_t
    print(f"{what}: pixels that differ from the restatement {counts}")
    assert not any(counts.values()), f"{what}: {counts}"


def _same(a, b):
    return all((x is None and y is None) or _differ(x, y) == 0 for x, y in zip(a, b))


class Installed:
    """A co-pol / cross-pol LUT pair installed on `ctx`, with the tables as the context holds them (xsw_lut_read)."""

    def __init__(self, ctx, lco, lcr):
        co, cr = lut_dicts(lco, lcr)
        ctx.upload_luts(co=co, cr=cr)
        self.ctx = ctx
        self.co_axes = tuple(np.asarray(a, dtype=np.float64) for a in (lco.incidence, lco.wspd, lco.phi))
        self.cr_axes = tuple(np.asarray(a, dtype=np.float64) for a in (lcr.incidence, lcr.wspd))
        self.co = ctx.read_lut(tuple(len(a) for a in self.co_axes))
        self.cr = ctx.read_lut(tuple(len(a) for a in self.cr_axes), cross=True)

    def ref_co(self, inc, wspd, phi, fold=True):
        return fref.eval_co(self.co, *self.co_axes, inc, wspd, phi, fold_phi=fold)

    def ref_cr(self, inc, wspd):
        return fref.eval_cr(self.cr, *self.cr_axes, inc, wspd)


@pytest.fixture
def default_tables(gpu_ctx, default_luts):
    return Installed(gpu_ctx, *default_luts)


def _scene(tab, shape, dtype, seed=0):
    """(inc, wspd, phi, wspd_cr) rasters of `dtype`: drawn beyond the axes, on nodes, one NaN per coordinate (forward_ref.points);
    half of the directions from -200 to 400 degrees.  The default tables' axes are long (50 degrees, 50 and 77 m/s), so the
    margins are 2.5 degrees / 1.5 m/s here: on the CPU that gives 0.87 (co-pol, folded) and 0.89 (cross-pol) finite pixels, where
    the small tables' margins would leave less than 0.05 outside."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    inc, w, p = fref.points(rng, tab.co_axes, n, MARGINS)
    p2 = rng.uniform(-200.0, 400.0, n)
    at = rng.random(n) < 0.5
    p = np.where(at & ~np.isnan(p), p2, p)
    wcr = fref.points(rng, tab.cr_axes, n, MARGINS)[1]
    return tuple(a.reshape(shape).astype(dtype) for a in (inc, w, p, wcr))


@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_equal_to_the_restatement(default_tables, torch, dtype, out_t):
    """70 x 333 (ragged last block) on the default LUTs: co-pol with and without the fold, cross-pol."""
    from xsarsea_amd import _lib
    tab = default_tables
    inc, w, p, wcr = _scene(tab, (70, 333), dtype)
    for fold in (True, False):
        got = _eval(tab.ctx, torch, _lib, "co", (inc, w, p), out_t, fold=fold)
        want = tab.ref_co(inc, w, p, fold)
        _assert_fields("co", got, want, out_t, f"co-pol, fold {fold}")
        finite = np.isfinite(want["sigma0_db"]).mean()
        print(f"fold {fold}: finite share {finite:.3f}, reflected {want['reflected'].mean():.3f}")
        assert 1 - finite >= 0.05 and (finite >= 0.75 or not fold)
        assert all(np.array_equal(np.isnan(g), np.isnan(got[0])) for g in got[1:])
    assert want["reflected"].sum() == 0 and tab.ref_co(inc, w, p)["reflected"].mean() > 0.1
    got = _eval(tab.ctx, torch, _lib, "cr", (inc, wcr), out_t)
    want = tab.ref_cr(inc, wcr)
    _assert_fields("cr", got, want, out_t, "cross-pol")
    finite = np.isfinite(want["sigma0_db"]).mean()
    assert finite >= 0.75 and 1 - finite >= 0.05


# ------------------------------------------------------------------------------------------------ every cell and node of a table
def _small_table(n_w, n_phi):
    """dB tables with 2 incidences, n_w speeds, n_phi directions (0..180) and a 2 x n_w cross-pol table."""
    ai, aw, ap = np.array([25.0, 40.0]), np.linspace(2.0, 20.0, n_w), np.linspace(0.0, 180.0, n_phi)
    co = -20.0 + 0.5 * aw[None, :, None] + 1.5 * np.cos(np.deg2rad(ap))[None, None, :] * np.sqrt(aw)[None, :, None] - 0.2 * (ai - 25.0)[:, None, None]
    cr = -35.0 + 0.6 * aw[None, :] - 0.05 * (ai - 25.0)[:, None]
    return olut.Lut(co, ai, aw, ap, "dB", "x", "co", "VV"), olut.Lut(cr, ai, aw, None, "dB", "x", "cr", "VH")


def _table_luts(name):
    if name.startswith("golden_"):
        return small_luts(golden(f"kernel_small_{name[7:]}_f64.npz"))
    if name == "nonuniform_11x9":  # phi_pad = 12: phi_pad % 8 == 4
        (co, ai, aw, ap), (cr, _, awcr) = fref.nonuniform_tables()
        return olut.Lut(co, ai, aw, ap, "dB", "x", "co", "VV"), olut.Lut(cr, ai, awcr, None, "dB", "x", "cr", "VH")
    return _small_table(*{"small_2x2x2": (2, 2), "small_2x9x2": (9, 2)}[name])


def _nodes_and_centres(ax):
    out = np.empty(2 * len(ax) - 1)
    out[0::2], out[1::2] = ax, 0.5 * (ax[:-1] + ax[1:])
    return out


TABLES = ["golden_phi180", "golden_phi360", "golden_phi90", "nonuniform_11x9", "small_2x2x2", "small_2x9x2"]


@pytest.mark.parametrize("name", TABLES)
def test_every_cell_and_node(gpu_ctx, torch, name):
    """Every node and every cell centre of the three axes, as one raster: nodes take the cell below them, the first node the
    first cell.  With the fold also the mirror image -phi, phi + 360 and 180 - phi of every direction (beyond a 0..90 table: NaN)."""
    from xsarsea_amd import _lib
    tab = Installed(gpu_ctx, *_table_luts(name))
    if name == "nonuniform_11x9":
        assert (tab.co.shape[2] + 3) // 4 * 4 % 8 == 4  # phi_pad: a pair's rows alternate between 16- and 8-byte alignment
    gi, gw, gp = (_nodes_and_centres(a) for a in tab.co_axes)
    for fold in (False, True):
        pp = np.concatenate([gp, -gp, gp + 360.0, 180.0 - gp]) if fold else gp
        inc, w, p = (a.reshape(len(gi) * len(gw), len(pp)) for a in np.meshgrid(gi, gw, pp, indexing="ij"))
        got = _eval(gpu_ctx, torch, _lib, "co", (inc, w, p), np.float64, fold=fold)
        want = tab.ref_co(inc, w, p, fold)
        _assert_fields("co", got, want, np.float64, f"{name}, fold {fold}")
        if not fold:
            assert np.isfinite(got[0]).all()
            # at a node the value is the table's own entry (slope * (x_hi - x_lo) + y_lo may differ from y_hi in the last bit:
            # judged on the first node of every axis, where it is y_lo + 0)
            assert got[0].reshape(len(gi), len(gw), len(gp))[0, 0, 0] == tab.co[0, 0, 0]
        elif name == "golden_phi90":
            assert np.isnan(got[0]).any() and np.isfinite(got[0]).any()
        else:
            assert np.isfinite(got[0]).all()
    gi, gw = (_nodes_and_centres(a) for a in tab.cr_axes)
    inc, w = np.meshgrid(gi, gw, indexing="ij")
    got = _eval(gpu_ctx, torch, _lib, "cr", (inc, w), np.float64)
    _assert_fields("cr", got, tab.ref_cr(inc, w), np.float64, f"{name} cross-pol")
    assert np.isfinite(got[0]).all() and got[0][0, 0] == tab.cr[0, 0]


# ------------------------------------------------------------------------------------------------ shapes, routes, outputs
@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 64), (0, 5)])
def test_small_shapes_and_host_route(default_tables, torch, shape):
    """One lane, one short of / exactly / one past a block, whole waves, no pixel at all (the calls return and write nothing); the
    host route equals the device route."""
    from xsarsea_amd import _lib
    tab = default_tables
    if 0 in shape:
        z = np.zeros(shape)
        for mem in (None, _lib.MEM_HOST):
            assert all(g.shape == shape for g in _eval(tab.ctx, torch, _lib, "co", (z, z, z), np.float64, mem=mem))
            assert all(g.shape == shape for g in _eval(tab.ctx, torch, _lib, "cr", (z, z), np.float32, mem=mem))
        return
    rng = np.random.default_rng(7)
    inc, w, p = rng.uniform(17, 65, shape), rng.uniform(0.3, 49, shape), rng.uniform(-180, 180, shape)
    dev = _eval(tab.ctx, torch, _lib, "co", (inc, w, p), np.float64)
    _assert_fields("co", dev, tab.ref_co(inc, w, p), np.float64, f"{shape} co-pol")
    assert np.isfinite(dev[0]).all()
    assert _same(_eval(tab.ctx, torch, _lib, "co", (inc, w, p), np.float64, mem=_lib.MEM_HOST), dev)
    wcr = rng.uniform(3.5, 79, shape)  # (the cross-pol speed axis: 3 .. 80 m/s)
    dev = _eval(tab.ctx, torch, _lib, "cr", (inc, wcr), np.float64)
    _assert_fields("cr", dev, tab.ref_cr(inc, wcr), np.float64, f"{shape} cross-pol")
    assert np.isfinite(dev[0]).all()
    assert _same(_eval(tab.ctx, torch, _lib, "cr", (inc, wcr), np.float64, mem=_lib.MEM_HOST), dev)


def test_host_route_equals_device_route(default_tables, torch):
    from xsarsea_amd import _lib
    tab = default_tables
    for dtype, out_t in ((np.float32, np.float64), (np.float64, np.float32)):
        inc, w, p, wcr = _scene(tab, (9, 333), dtype, 3)
        assert _same(_eval(tab.ctx, torch, _lib, "co", (inc, w, p), out_t, mem=_lib.MEM_HOST), _eval(tab.ctx, torch, _lib, "co", (inc, w, p), out_t))
        assert _same(_eval(tab.ctx, torch, _lib, "cr", (inc, wcr), out_t, mem=_lib.MEM_HOST), _eval(tab.ctx, torch, _lib, "cr", (inc, wcr), out_t))


def test_every_subset_of_outputs(default_tables, torch):
    """All 7 + 3 non-empty subsets: a requested output equals the full call's, an unrequested one is never written (`_eval` checks
    the guard regions of every buffer it hands over)."""
    from xsarsea_amd import _lib
    tab = default_tables
    inc, w, p, wcr = _scene(tab, (5, 333), np.float32, 4)
    for kind, arrs in (("co", (inc, w, p)), ("cr", (inc, wcr))):
        full = _eval(tab.ctx, torch, _lib, kind, arrs, np.float64)
        subsets = [s for s in itertools.product((0, 1), repeat=len(full)) if any(s)]
        assert len(subsets) == (7 if kind == "co" else 3)
        for s in subsets:
            for mem in (None, _lib.MEM_HOST):
                got = _eval(tab.ctx, torch, _lib, kind, arrs, np.float64, want=s, mem=mem)
                assert all((g is None) == (not k) for g, k in zip(got, s))
                assert _same(got, [f if k else None for f, k in zip(full, s)]), (kind, s, mem)


def test_error_codes(torch):
    """An error code and a message before any launch: the outputs keep their fill."""
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a = np.full((2, 8), 33.0, np.float32)
        o = np.full((2, 8), 77.0, np.float32)
        p = lambda x: None if x is None else x.ctypes.data
        msg = lambda: ctx._lib.xsw_last_error(ctx._h).decode()
        co = lambda ins=(a, a, a), outs=(o, None, None), shape=(2, 8), dt=0, od=0, mem=0: ctx._lib.xsw_lut_eval(
            ctx._h, *shape, dt, od, mem, 1, *(p(x) for x in ins), *(p(x) for x in outs))
        cr = lambda ins=(a, a), outs=(o, None), shape=(2, 8), dt=0, od=0, mem=0: ctx._lib.xsw_lut_eval_cr(
            ctx._h, *shape, dt, od, mem, *(p(x) for x in ins), *(p(x) for x in outs))
        assert co() == -3 and "no co-pol LUT" in msg()
        assert cr() == -3 and "no cross-pol LUT" in msg()
        # a 9 x 1 table: there is no cell on the direction axis, nor on the one-point cross-pol speed axis
        ai, aw = np.array([20.0, 30.0, 45.0]), np.linspace(1.0, 9.0, 9)
        lco = olut.Lut(np.zeros((3, 9, 1)), ai, aw, np.array([0.0]), "dB", "x", "co", "VV")
        lcr = olut.Lut(np.zeros((3, 1)), ai, aw[:1], None, "dB", "x", "cr", "VH")
        dco, dcr = lut_dicts(lco, lcr)
        ctx.upload_luts(co=dco, cr=dcr)
        assert co() == -1 and "fewer than two points" in msg()
        assert cr() == -1 and "fewer than two points" in msg()
        ctx.upload_luts(*lut_dicts(*_small_table(2, 2)))
        assert co() == 0 and cr() == 0
        o[:] = 77.0
        for k in range(3):
            ins = [a, a, a]
            ins[k] = None
            assert co(ins=ins) == -1 and "NULL" in msg()
        assert cr(ins=(None, a)) == -1 and cr(ins=(a, None)) == -1 and "NULL" in msg()
        assert co(outs=(None, None, None)) == -1 and "no output" in msg()
        assert cr(outs=(None, None)) == -1 and "no output" in msg()
        assert co(shape=(-1, 8)) == -1 and co(dt=2) == -1 and co(od=5) == -1 and co(mem=9) == -1
        assert cr(shape=(2, -8)) == -1 and cr(dt=2) == -1 and cr(mem=9) == -1
        assert co(shape=(1 << 31, 1 << 20)) == -1 and "too large" in msg()
        assert cr(shape=(1 << 31, 1 << 20)) == -1 and "too large" in msg()
        assert np.all(o == 77.0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public interface
KW = dict(model="gmf_cmod5n", resolution="low")
KW_CR = dict(model="gmf_s1_v2", resolution="low")


def _public_scene(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    inc, w, p = rng.uniform(15.5, 66.5, shape), rng.uniform(0.0, 51.0, shape), rng.uniform(-200.0, 400.0, shape)
    inc[0, 0], w[0, 1], p[0, 2] = np.nan, np.nan, np.nan
    return inc.astype(dtype), w.astype(dtype), p.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_simulate_sigma0_numpy_and_torch(torch, dtype):
    """`simulate_sigma0` on numpy rasters and on torch tensors == the raw entries on the context it installed its table in."""
    from xsarsea_amd import _lib, windspeed
    from xsarsea_amd.windspeed import _engine
    inc, w, p = _public_scene((33, 130), dtype, 21)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (inc, w, p)]
    ctx = _lib.default_context(0)
    for fold in (True, False):
        jac = windspeed.simulate_sigma0(inc, w, p, jacobian=True, fold_phi=fold, **KW)
        raw = _eval(ctx, torch, _lib, "co", (inc, w, p), np.float64, fold=fold)
        assert _same([jac.sigma0, jac.dwspd, jac.dphi], raw) and jac.sigma0.dtype == np.float64
        lut = _engine.lut_source(windspeed.get_model(KW["model"]), dict(resolution="low"))
        table = ctx.read_lut(lut.shape)
        _assert_fields("co", raw, fref.eval_co(table, lut.incidence, lut.wspd, lut.phi, inc, w, p, fold_phi=fold), np.float64, f"public, fold {fold}")
        tj = windspeed.simulate_sigma0(*t, jacobian=True, fold_phi=fold, **KW)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (tj.sigma0, tj.dwspd, tj.dphi))
        assert _same([x.cpu().numpy() for x in (tj.sigma0, tj.dwspd, tj.dphi)], raw)
        finite = np.isfinite(raw[0]).mean()  # (the scene lies 0.5 degrees / 0.2 and 1 m/s beyond the axes; unfolded: -200 .. 400 degrees)
        assert (0.75 < finite < 0.99) if fold else (0.2 < finite < 0.5)
    # alone, float32 out, linear units
    s32 = windspeed.simulate_sigma0(inc, w, p, out_dtype=np.float32, **KW)
    assert s32.dtype == np.float32 and _differ(s32, _eval(ctx, torch, _lib, "co", (inc, w, p), np.float32)[0]) == 0
    db = windspeed.simulate_sigma0(inc, w, p, **KW)
    assert _differ(windspeed.simulate_sigma0(inc, w, p, units="linear", **KW), 10 ** (db / 10)) == 0
    tdb = windspeed.simulate_sigma0(*t, **KW)
    assert _differ(windspeed.simulate_sigma0(*t, units="linear", **KW).cpu().numpy(), (10 ** (tdb / 10)).cpu().numpy()) == 0
    # wind=: the array module's own modulus and degrees(angle), then the same kernel
    wind = (np.nan_to_num(w, nan=3.0) * np.exp(1j * np.deg2rad(np.nan_to_num(p, nan=10.0)))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    assert _differ(windspeed.simulate_sigma0(inc, wind=wind, **KW), windspeed.simulate_sigma0(inc, np.abs(wind), np.degrees(np.angle(wind)), **KW)) == 0
    tw = torch.from_numpy(wind).to(dev)
    assert _differ(windspeed.simulate_sigma0(t[0], wind=tw, **KW).cpu().numpy(),
                   windspeed.simulate_sigma0(t[0], torch.abs(tw), torch.rad2deg(torch.angle(tw)), **KW).cpu().numpy()) == 0
    # Python scalars are expanded; an empty raster
    assert _differ(windspeed.simulate_sigma0(inc, 7.5, 30, **KW), windspeed.simulate_sigma0(inc, np.full_like(inc, 7.5), np.full_like(inc, 30), **KW)) == 0
    assert windspeed.simulate_sigma0(inc[:0], w[:0], p[:0], **KW).shape == (0, 130)
    assert tuple(windspeed.simulate_sigma0(t[0][:0], t[1][:0], t[2][:0], **KW).shape) == (0, 130)
    # cross-pol: no direction
    jc = windspeed.simulate_sigma0(inc, w, jacobian=True, **KW_CR)
    raw = _eval(ctx, torch, _lib, "cr", (inc, w), np.float64)
    assert _same([jc.sigma0, jc.dwspd], raw) and jc.dphi is None and np.isfinite(raw[0]).any()
    lut = _engine.lut_source(windspeed.get_model(KW_CR["model"]), dict(resolution="low"))
    _assert_fields("cr", raw, fref.eval_cr(ctx.read_lut(lut.shape, cross=True), lut.incidence, lut.wspd, inc, w), np.float64, "public cross-pol")
    tc = windspeed.simulate_sigma0(t[0], t[1], jacobian=True, **KW_CR)
    assert _same([tc.sigma0.cpu().numpy(), tc.dwspd.cpu().numpy()], raw)
    assert _differ(windspeed.simulate_sigma0(inc, wind=wind, **KW_CR), windspeed.simulate_sigma0(inc, np.abs(wind), **KW_CR)) == 0


def test_array_lut_model_on_rasters(torch):
    """`model(inc2d, wspd2d, phi2d, units="dB")` for an ArrayLutModel: numpy and torch rasters, pointwise, no fold: bit for bit the
    diagonal of its own 1-D call (three host lerp_axis passes)."""
    from xsarsea_amd.windspeed import models
    from xsarsea_amd.windspeed.lut import Lut
    (co, ai, aw, ap), (cr, _, awcr) = fref.nonuniform_tables()
    try:
        m = models.ArrayLutModel("gmf_fwdgpu_co", Lut(co, ai, aw, ap, units="dB", resolution="high"), pol="VV")
        mcr = models.ArrayLutModel("gmf_fwdgpu_cr", Lut(cr, ai, awcr, None, units="dB", resolution="high"), pol="VH")
        rng = np.random.default_rng(5)
        cols = fref.points(rng, (ai, aw, ap), 60)
        inc, w, p = (c.reshape(6, 10) for c in cols)
        want = np.einsum("iii->i", np.asarray(m(*cols, units="dB"))).reshape(6, 10)
        got = m(inc, w, p, units="dB")
        assert isinstance(got, np.ndarray) and _differ(got, want) == 0 and np.isnan(want).any() and np.isfinite(want).mean() > 0.5
        dev = torch.device("cuda", 0)
        tg = m(*(torch.from_numpy(a).to(dev) for a in (inc, w, p)), units="dB")
        assert tg.is_cuda and _differ(tg.cpu().numpy(), want) == 0
        wc = fref.points(rng, (ai, awcr), 60)[1].reshape(6, 10)
        want = np.einsum("ii->i", np.asarray(mcr(inc.ravel(), wc.ravel(), units="dB"))).reshape(6, 10)
        assert _differ(mcr(inc, wc, units="dB"), want) == 0 and np.isfinite(want).any()
    finally:
        for n in ("gmf_fwdgpu_co", "gmf_fwdgpu_cr"):
            models.Model._available_models.pop(n, None)


def test_user_stream_without_an_intermediate_sync(torch, delay_cycles):
    """simulate_sigma0 (co-pol with its Jacobian, cross-pol) on a user stream whose producer is held back, followed by dependent
    torch work on that stream: all return while the producer is in flight, and the result equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _public_scene((48, 260), np.float32, 51), _public_scene((48, 260), np.float32, 52)

    def call(b):
        j = windspeed.simulate_sigma0(b[0], b[1], b[2], jacobian=True, **KW)
        vh = windspeed.simulate_sigma0(b[0], b[1], **KW_CR)
        return j.sigma0 - vh, j.dwspd * 2.0, j.dphi  # dependent torch work, no synchronisation in between

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = _staged(torch, list(sc), list(dec))
        ref = call([src for _, src in pairs])  # landed rasters, synchronised: LUTs installed
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
    assert np.isfinite(ref[0]).mean() > 0.5 and _same(got, ref)
