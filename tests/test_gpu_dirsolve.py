"""GPU: wind direction at a known speed (xsw_dir_solve, kernel k_dir_solve_co; `windspeed.retrieve_dir`, `retrieve_wind`).

The yardstick everywhere is the numpy restatement tests/dirsolve_ref.py (held to the forward restatement and to the plain meaning
of its count by tests/test_dirsolve_cpu.py), evaluated on the table READ BACK from the context (xsw_lut_read), never on a
host-built copy.  Every real output, the count and the flag must equal it bit for bit, NaN positions included; float32 outputs are
the restatement rounded once.  Only IEEE + - * / and fmod in float64 follow the cell search, so there is no tolerance."""
import warnings

import numpy as np
import pytest

import dirsolve_ref as dref
import forward_ref as fref
import solve_ref as sref
from test_gpu_forward import GUARD, SENTINEL, Installed, _differ, _nodes_and_centres, default_tables  # noqa: F401 (fixture)
from test_gpu_streams import _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from util import lut_dicts, small_luts
from conftest import golden

from oracle import lut as olut

pytestmark = pytest.mark.gpu

BYTE_SENTINEL = np.uint8(0xA5)  # no count of these tests and no combination of the XSW_DIR_* bits
FIELDS = dref.FIELDS            # phi1, phi2, sens1, sens2, phi_near, sens_near, phi_closest, count, flag: xsw_dir_solve's order
ALL, NO_NEAR = (1,) * 9, (1, 1, 1, 1, 0, 0, 1, 1, 1)


def _dir(ctx, torch, _lib, arrs, out_t, near=None, want=None, mem=None, fold=True):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays): arrs = (inc, sigma0_db, wspd), near a fourth raster or
    None -> the nine outputs in FIELDS' order.  Every requested output lies between two guard regions and starts as its sentinel;
    returns host arrays (None where not requested) after checking that the guards are untouched and every pixel was written."""
    want = (ALL if near is not None else NO_NEAR) if want is None else want
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    types = (out_t,) * 7 + (np.uint8,) * 2
    sents = (SENTINEL[out_t],) * 7 + (BYTE_SENTINEL,) * 2
    given = list(arrs) + ([near] if near is not None else [])
    hosts = [np.ascontiguousarray(a if n else np.zeros(1, a.dtype)) for a in given]  # an empty raster: no pointer is NULL
    host_route = mem == _lib.MEM_HOST
    if host_route:
        bufs = [np.full(n + 2 * GUARD, s, t) if w else None for w, t, s in zip(want, types, sents)]
        ins = [a.ctypes.data for a in hosts]
        outs = [None if b is None else b.ctypes.data + GUARD * b.itemsize for b in bufs]
    else:
        dev = torch.device("cuda", 0)
        keep = [torch.from_numpy(a).to(dev) for a in hosts]
        bufs = [torch.from_numpy(np.full(n + 2 * GUARD, s, t)).to(dev) if w else None for w, t, s in zip(want, types, sents)]
        torch.cuda.synchronize()
        ins = [t.data_ptr() for t in keep]
        outs = [None if b is None else b.data_ptr() + GUARD * b.element_size() for b in bufs]
    if near is None:
        ins.append(None)
    lines, samples = (shape[0], shape[1]) if len(shape) == 2 else _lib.lines_samples(shape)
    ctx.dir_solve_raw(lines, samples, dt, od, _lib.MEM_HOST if host_route else _lib.MEM_DEVICE, *ins, *outs, fold_phi=fold)
    ctx.synchronize()
    res = []
    for b, sent in zip(bufs, sents):
        if b is None:
            res.append(None)
            continue
        h = b if host_route else b.cpu().numpy()
        assert np.all(h[:GUARD] == sent) and np.all(h[-GUARD:] == sent), "a guard region was written"
        assert not np.any(h[GUARD:n + GUARD] == sent), "a pixel was not written"
        res.append(h[GUARD:n + GUARD].reshape(shape).copy())
    return res


def _assert_fields(got, want, out_t, what):
    """Every requested field == the restatement's (reals rounded once to a float32 output), NaN positions included."""
    counts = {}
    for k, g in zip(FIELDS, got):
        if g is None:
            continue
        if k in ("count", "flag"):
            assert g.dtype == np.uint8
            counts[k] = int(np.sum(g != want[k]))
        else:
            assert g.dtype == out_t
            with np.errstate(all="ignore"):
                counts[k] = _differ(g, want[k].astype(out_t))
    print(f"{what}: pixels that differ from the restatement {counts}")
    assert not any(counts.values()), f"{what}: {counts}"


def _same(a, b):
    return all((x is None and y is None) or (np.array_equal(x, y) if x.dtype == np.uint8 else _differ(x, y) == 0) for x, y in zip(a, b))


def _ref(tab, inc, s, w, near=None, fold=True):
    return dref.solve(tab.co, *tab.co_axes, inc, s, w, near=near, fold_phi=fold)


def _scene(tab, shape, dtype, seed=0):
    """(inc, s, w, near) rasters of `dtype` on the default tables: incidence 18..46 degrees and, for one pixel in sixteen, up to 2
    degrees beyond either end of the axis or exactly on it; speeds 0..55 m/s (the axis: 0.2..50); s the table's own value at a random
    true direction plus N(0, 0.3 dB) (a plain -15 dB where the speed or the incidence has no table value); near that direction or its
    mirror image, a turn of 360 degrees added to a third; NaN holes in each input, in different pixels."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    ai, aw, ap = tab.co_axes
    inc = rng.uniform(18.0, 46.0, n)
    edge = np.flatnonzero(rng.random(n) < 1 / 16)
    inc[edge] = np.choose(np.arange(len(edge)) % 4, [rng.uniform(ai[0] - 2.0, ai[0], len(edge)), rng.uniform(ai[-1], ai[-1] + 2.0, len(edge)),
                                                      np.full(len(edge), ai[0]), np.full(len(edge), ai[-1])])
    w = rng.uniform(0.0, 55.0, n)
    p = rng.uniform(ap[0], ap[-1], n)
    s = fref.eval_co(tab.co, ai, aw, ap, inc, w, p, fold_phi=False)["sigma0_db"]
    s = np.where(np.isnan(s), -15.0, s) + rng.normal(0.0, 0.3, n)
    near = np.where(rng.random(n) < 0.5, p, -p) + 360.0 * rng.integers(-1, 2, n)
    for k, x in enumerate((inc, s, w, near)):
        x[rng.choice(n, n // 100, replace=False)] = np.nan
    return tuple(a.reshape(shape).astype(dtype) for a in (inc, s, w, near))


def _shares(r):
    f, c = r["flag"], r["count"]
    return dict(below=float((f == dref.BELOW).mean()), above=float((f == dref.ABOVE).mean()), one=float((c == 1).mean()), two=float((c == 2).mean()),
                more=float((c > 2).mean()), nan=float((f == dref.NAN).mean()))


@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_equal_to_the_restatement(default_tables, torch, dtype, out_t):
    """70 x 333 (ragged last block) on the default LUT, with the reference direction, with and without the mirror images, and
    without a reference.  The classes of the restatement's answer are asserted first, so that none is thin: no solution BELOW, no
    solution ABOVE, one, two, gated NaN."""
    from xsarsea_amd import _lib
    tab = default_tables
    inc, s, w, near = _scene(tab, (70, 333), dtype)
    for fold in (True, False):
        want = _ref(tab, inc, s, w, near, fold)
        sh = _shares(want)
        print(f"fold {fold}: {sh}")
        assert min(sh["below"], sh["above"], sh["one"], sh["two"], sh["nan"]) >= 0.03 and sh["more"] == 0
        got = _dir(tab.ctx, torch, _lib, (inc, s, w), out_t, near=near, fold=fold)
        _assert_fields(got, want, out_t, f"fold {fold}")
        real = dict(zip(FIELDS, got))
        assert np.array_equal(np.isnan(real["phi1"]), real["count"] == 0) and np.array_equal(np.isnan(real["phi2"]), real["count"] < 2)
        assert np.array_equal(real["count"] == 0, (real["flag"] & 7) != 0) and np.array_equal(np.isnan(real["phi_closest"]), real["flag"] == dref.NAN)
        assert np.array_equal(np.isnan(real["phi_near"]), (real["count"] == 0) | np.isnan(near)) and (fold or not np.any(real["phi_near"] < 0))
    assert np.any(got[4] != _dir(tab.ctx, torch, _lib, (inc, s, w), out_t, near=near)[4])  # (the mirror images are chosen somewhere)
    _assert_fields(_dir(tab.ctx, torch, _lib, (inc, s, w), out_t), _ref(tab, inc, s, w), out_t, "no reference")


# ------------------------------------------------------------------------------------------------ every cell and node of a table
HAND_MADE = {"wavy": dref.wavy_table, "zigzag_301": dref.zigzag_table, "flat": dref.flat_table, "nan_nodes": dref.nan_table, "monotone": dref.monotone_table}
SMALL = ["golden_phi180", "golden_phi360", "golden_phi90", "nonuniform_11x9"] + list(HAND_MADE)


def _small_luts(name):
    cr, ai_cr, aw_cr = sref.nonmonotone_cr()
    lcr = olut.Lut(cr, ai_cr, aw_cr, None, "dB", "x", "cr", "VH")
    if name.startswith("golden_"):
        return small_luts(golden(f"kernel_small_{name[7:]}_f64.npz"))
    co, ai, aw, ap = fref.nonuniform_tables()[0] if name == "nonuniform_11x9" else HAND_MADE[name]()
    return olut.Lut(co, ai, aw, ap, "dB", "x", "co", "VV"), lcr


@pytest.mark.parametrize("name", SMALL)
def test_every_cell_and_node(gpu_ctx, torch, name):
    """Every node and cell centre of the incidence and the speed axis, and at each of them s on every node value d(j) and midway
    through every cell of the column, half a dB below its lowest and above its highest value: as one raster, with reference
    directions that walk round the circle twice."""
    from xsarsea_amd import _lib
    tab = Installed(gpu_ctx, *_small_luts(name))
    ai, aw, ap = tab.co_axes
    inc, w = (a.ravel() for a in np.meshgrid(_nodes_and_centres(ai), _nodes_and_centres(aw), indexing="ij"))
    D = dref.node_values(tab.co, ai, aw, inc, w)
    with np.errstate(all="ignore"):
        s = np.concatenate([D, 0.5 * (D[:, :-1] + D[:, 1:]), np.nanmin(D, axis=1, keepdims=True) - 0.5, np.nanmax(D, axis=1, keepdims=True) + 0.5], axis=1)
    inc, w = (np.repeat(a[:, None], s.shape[1], axis=1) for a in (inc, w))
    near = (np.arange(s.size, dtype=np.float64).reshape(s.shape) * 7.25) % 720.0 - 360.0
    for fold in (True, False):
        want = _ref(tab, inc, s, w, near, fold)
        got = _dir(gpu_ctx, torch, _lib, (inc, s, w), np.float64, near=near, fold=fold)
        _assert_fields(got, want, np.float64, f"{name}, fold {fold}")
    sh = _shares(want)
    print(name, sh, "largest count", int(want["n"].max()))
    assert sh["below"] > 0 and sh["above"] > 0 and (sh["one"] > 0) == (name != "zigzag_301") and (sh["nan"] > 0) == (name == "nan_nodes")
    assert (sh["more"] > 0) == (name not in ("nonuniform_11x9", "flat", "nan_nodes", "monotone"))  # (the goldens' columns are rough)
    if name == "zigzag_301":
        assert want["n"].max() == 300 and want["count"].max() == 255 and got[7].max() == 255
    if name == "flat":
        assert np.isinf(got[3]).any() and not np.isnan(got[1][np.isinf(got[3])]).any()  # the flat last cell: a direction, an infinite sensitivity


# ------------------------------------------------------------------------------------------------ shapes, routes, outputs
@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (1, 256), (1, 257), (2, 3, 43), (0, 5)])
def test_small_shapes_and_host_route(default_tables, torch, shape):
    """One lane, one short of / exactly / one past a block, three axes (through lines_samples), no pixel at all (the calls return
    and write nothing); the host route equals the device route."""
    from xsarsea_amd import _lib
    tab = default_tables
    if 0 in shape:
        z = np.zeros(shape)
        for mem in (None, _lib.MEM_HOST):
            assert all(g.shape == shape for g in _dir(tab.ctx, torch, _lib, (z, z, z), np.float64, near=z, mem=mem))
            assert all(g is None or g.shape == shape for g in _dir(tab.ctx, torch, _lib, (z, z, z), np.float32, mem=mem))
        return
    rng = np.random.default_rng(7)
    inc, w, p = rng.uniform(17, 65, shape), rng.uniform(0.3, 20, shape), rng.uniform(0, 180, shape)
    s = fref.eval_co(tab.co, *tab.co_axes, inc, w, p)["sigma0_db"]
    dev = _dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, near=p)
    _assert_fields(dev, _ref(tab, inc, s, w, p), np.float64, f"{shape}")
    assert np.isfinite(dev[4]).all() and np.abs(dev[4] - p).max() < 1e-6  # (without noise the true direction itself comes back)
    assert _same(_dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, near=p, mem=_lib.MEM_HOST), dev)


def test_host_route_equals_device_route(default_tables, torch):
    from xsarsea_amd import _lib
    tab = default_tables
    for dtype, out_t in ((np.float32, np.float64), (np.float64, np.float32)):
        inc, s, w, near = _scene(tab, (9, 333), dtype, 3)
        assert _same(_dir(tab.ctx, torch, _lib, (inc, s, w), out_t, near=near, mem=_lib.MEM_HOST), _dir(tab.ctx, torch, _lib, (inc, s, w), out_t, near=near))
        assert _same(_dir(tab.ctx, torch, _lib, (inc, s, w), out_t, mem=_lib.MEM_HOST), _dir(tab.ctx, torch, _lib, (inc, s, w), out_t))


def test_each_output_alone_and_all_together(default_tables, torch):
    """Each of the nine outputs alone, all together, and the seven that need no reference direction with `near` absent: a requested
    output equals the full call's, an unrequested one is never written (`_dir` checks the guard regions of every buffer it hands
    over)."""
    from xsarsea_amd import _lib
    tab = default_tables
    inc, s, w, near = _scene(tab, (5, 333), np.float32, 4)
    full = _dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, near=near)
    _assert_fields(full, _ref(tab, inc, s, w, near), np.float64, "all nine")
    for mem in (None, _lib.MEM_HOST):
        for k in range(9):
            sub = tuple(int(j == k) for j in range(9))
            got = _dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, near=near, want=sub, mem=mem)
            assert all((g is None) == (j != k) for j, g in enumerate(got)) and _same(got, [f if j == k else None for j, f in enumerate(full)]), (FIELDS[k], mem)
            if k not in (4, 5):  # the same output without a reference direction
                assert _same(_dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, want=sub, mem=mem), got), (FIELDS[k], mem)
        got = _dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, mem=mem)
        assert _same(got, [f if k else None for f, k in zip(full, NO_NEAR)]), mem
        got = _dir(tab.ctx, torch, _lib, (inc, s, w), np.float64, near=near, want=NO_NEAR, mem=mem)  # a reference nobody selects by
        assert _same(got, [f if k else None for f, k in zip(full, NO_NEAR)]), mem


def test_error_codes(torch):
    """An error code and a message before any launch: the outputs keep their fill."""
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    try:
        a = np.full((2, 8), 33.0, np.float32)
        o = np.full((2, 8), 77.0, np.float32)
        f = np.full((2, 8), 0xA5, np.uint8)
        at = lambda x: None if x is None else x.ctypes.data
        msg = lambda: ctx._lib.xsw_last_error(ctx._h).decode()
        none = (None,) * 9
        some = (o, None, None, None, None, None, None, None, f)
        call = lambda ins=(a, a, a, None), outs=some, shape=(2, 8), dt=0, od=0, mem=0: ctx._lib.xsw_dir_solve(
            ctx._h, *shape, dt, od, mem, 1, *(at(x) for x in ins), *(at(x) for x in outs))
        assert call() == -3 and "no co-pol LUT" in msg()
        ai, aw = np.array([20.0, 30.0, 45.0]), np.linspace(1.0, 9.0, 9)
        lcr = olut.Lut(np.zeros((3, 9)), ai, aw, None, "dB", "x", "cr", "VH")
        ctx.upload_luts(*lut_dicts(olut.Lut(np.zeros((3, 9, 1)), ai, aw, np.array([0.0]), "dB", "x", "co", "VV"), lcr))
        assert call() == -1 and "fewer than two points" in msg()
        ctx.upload_luts(*lut_dicts(*_small_luts("wavy")))
        assert call() == 0 and not np.any(o == 77.0) and not np.any(f == 0xA5)
        o[:], f[:] = 77.0, 0xA5
        for k in range(3):
            ins = [a, a, a, None]
            ins[k] = None
            assert call(ins=ins) == -1 and "NULL" in msg()
        assert call(outs=none) == -1 and "no output" in msg()
        for k in (4, 5):  # out_phi_near, out_sens_near without near
            outs = list(none)
            outs[k] = o
            assert call(outs=outs) == -1 and "near" in msg()
            assert call(ins=(a, a, a, a), outs=outs) == 0
            o[:] = 77.0
        assert call(shape=(-1, 8)) == -1 and call(shape=(2, -8)) == -1 and call(dt=2) == -1 and call(od=5) == -1 and call(mem=9) == -1
        assert call(shape=(1 << 31, 1 << 20)) == -1 and "too large" in msg()
        assert call(shape=(0, 8)) == 0 and call(shape=(0, 0)) == 0  # an empty raster: XSW_OK, nothing written
        assert np.all(o == 77.0) and np.all(f == 0xA5)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public interface
KW = dict(model="gmf_cmod5n", resolution="low")
KW_CR = dict(model="gmf_s1_v2", resolution="low")


def _public_scene(shape, dtype, seed):
    """(inc, sigma0_db, wspd, near, sigma0_cr_db): the models' own tables at a wind of 0.5 .. 60 m/s (the co-pol table ends at 50,
    the cross-pol one at 80), 0.3 / 0.1 dB of noise, a NaN in each raster."""
    from xsarsea_amd import windspeed
    rng = np.random.default_rng(seed)
    inc, w, p = rng.uniform(17.5, 64.5, shape), rng.uniform(0.5, 60.0, shape), rng.uniform(-180.0, 180.0, shape)
    s = np.nan_to_num(windspeed.simulate_sigma0(inc, w, p, **KW), nan=-12.0) + rng.normal(0.0, 0.3, shape)
    scr = np.nan_to_num(windspeed.simulate_sigma0(inc, w, **KW_CR), nan=-30.0) + rng.normal(0.0, 0.1, shape)
    near = p + rng.normal(0.0, 20.0, shape)
    inc[0, 0], s[0, 1], w[0, 2], near[0, 3], scr[0, 4] = (np.nan,) * 5
    return tuple(a.astype(dtype) for a in (inc, s, w, near, scr))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_retrieve_dir_numpy_and_torch(torch, dtype):
    """`retrieve_dir` on numpy rasters and on torch tensors == the raw entry on the context it installed its table in == the
    restatement on that table; simulate_sigma0 of the answer gives sigma0 back; wind= is near= with the raster's angle."""
    from xsarsea_amd import _lib, windspeed
    from xsarsea_amd.windspeed import _engine
    inc, s, w, near, _ = _public_scene((33, 130), dtype, 21)
    dev = torch.device("cuda", 0)
    ti, ts, tw, tn = (torch.from_numpy(a).to(dev) for a in (inc, s, w, near))
    ctx = _lib.default_context(0)
    names = windspeed.RetrievedDir.FIELDS
    for fold in (True, False):
        r = windspeed.retrieve_dir(inc, s, w, near=near, units="dB", details=True, fold_phi=fold, **KW)
        raw = _dir(ctx, torch, _lib, (inc, s, w), np.float64, near=near, fold=fold)
        assert _same([r[k] for k in names], raw) and r.phi1.dtype == np.float64 and r.count.dtype == np.uint8 and r.flag.dtype == np.uint8
        lut = _engine.lut_source(windspeed.get_model(KW["model"]), dict(resolution="low"))
        want = dref.solve(ctx.read_lut(lut.shape), lut.incidence, lut.wspd, lut.phi, inc, s, w, near=near, fold_phi=fold)
        _assert_fields(raw, want, np.float64, f"public, fold {fold}")
        tr = windspeed.retrieve_dir(ti, ts, tw, near=tn, units="dB", details=True, fold_phi=fold, **KW)
        assert all(isinstance(tr[k], torch.Tensor) and tr[k].is_cuda for k in names) and tr.flag.dtype == torch.uint8 and tr.count.dtype == torch.uint8
        assert _same([tr[k].cpu().numpy() for k in names], raw)
        solved = raw[7] > 0
        print(f"fold {fold}: solved share {solved.mean():.3f}")
        assert 0.5 < solved.mean() < 0.95
        # the round trip through the forward operator, on the float64 rasters the kernel read
        chosen = np.isfinite(raw[4])
        back = windspeed.simulate_sigma0(inc.astype(np.float64), w.astype(np.float64), raw[4], **KW)
        err = np.abs(back - s.astype(np.float64))[chosen].max()
        print(f"round trip: {err:.3g} dB")
        assert err <= 1e-10 and chosen.sum() == solved.sum() - int(solved[0, 3])
    # the plain returns: the pair without a reference, phi_near with one; float32 out; an absent reference in the details
    pair = windspeed.retrieve_dir(inc, s, w, units="dB", **KW)
    assert isinstance(pair, tuple) and _same(pair, raw[:2])
    tpair = windspeed.retrieve_dir(ti, ts, tw, units="dB", **KW)
    assert _same([x.cpu().numpy() for x in tpair], raw[:2])
    n32 = windspeed.retrieve_dir(inc, s, w, near=near, units="dB", out_dtype=np.float32, **KW)
    assert n32.dtype == np.float32 and _differ(n32, _dir(ctx, torch, _lib, (inc, s, w), np.float32, near=near)[4]) == 0
    r = windspeed.retrieve_dir(ti, ts, tw, units="dB", details=True, **KW)
    assert r.phi_near is None and r.dphi_near_dsigma0 is None and _differ(r.phi_closest.cpu().numpy(), raw[6]) == 0
    # linear units (the array module's own dB)
    lin = (10 ** (s / 10)).astype(dtype)
    assert _differ(windspeed.retrieve_dir(inc, lin, w, near=near, **KW), windspeed.retrieve_dir(inc, _engine._to_db(lin), w, near=near, units="dB", **KW)) == 0
    tl = torch.from_numpy(lin).to(dev)
    assert _differ(windspeed.retrieve_dir(ti, tl, tw, near=tn, **KW).cpu().numpy(),
                   windspeed.retrieve_dir(ti, 10 * torch.log10(tl + 1e-15), tw, near=tn, units="dB", **KW).cpu().numpy()) == 0
    # wind=: an ancillary_from_streaks-style complex raster; only its angle is used
    wind = (7.0 * np.exp(1j * np.deg2rad(np.nan_to_num(near, nan=10.0)))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    assert _differ(windspeed.retrieve_dir(inc, s, w, wind=wind, units="dB", **KW), windspeed.retrieve_dir(inc, s, w, near=np.degrees(np.angle(wind)), units="dB", **KW)) == 0
    twind = torch.from_numpy(wind).to(dev)
    assert _differ(windspeed.retrieve_dir(ti, ts, tw, wind=twind, units="dB", **KW).cpu().numpy(),
                   windspeed.retrieve_dir(ti, ts, tw, near=torch.rad2deg(torch.angle(twind)), units="dB", **KW).cpu().numpy()) == 0
    # scalars are expanded; an empty raster
    assert _differ(windspeed.retrieve_dir(inc, s, 7, near=30, units="dB", **KW),
                   windspeed.retrieve_dir(inc, s, np.full_like(inc, 7), near=np.full_like(inc, 30), units="dB", **KW)) == 0
    assert windspeed.retrieve_dir(inc[:0], s[:0], w[:0], near=near[:0], **KW).shape == (0, 130)
    assert tuple(windspeed.retrieve_dir(ti[:0], ts[:0], tw[:0], details=True, **KW).flag.shape) == (0, 130)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_retrieve_wind_numpy_and_torch(torch, dtype):
    """`retrieve_wind` == the composition of the two restatements on the tables read back from the context: bit for bit on numpy
    rasters, `torch.equal` on the device against the same torch statement on the restatements' speed and direction."""
    from xsarsea_amd import _lib, windspeed
    from xsarsea_amd.windspeed import _engine
    inc, s, _, near, scr = _public_scene((33, 130), dtype, 31)
    models = (KW["model"], KW_CR["model"])
    got = windspeed.retrieve_wind(inc, s, scr, near=near, model=models, units="dB", resolution="low")
    ctx = _lib.default_context(0)
    lco = _engine.lut_source(windspeed.get_model(models[0]), dict(resolution="low"))
    lcr = _engine.lut_source(windspeed.get_model(models[1]), dict(resolution="low"))
    speed = sref.solve_cr(ctx.read_lut(lcr.shape, cross=True), lcr.incidence, lcr.wspd, inc, scr)["wspd"]
    phi = dref.solve(ctx.read_lut(lco.shape), lco.incidence, lco.wspd, lco.phi, inc, s, speed, near=near)["phi_near"]
    want = speed * np.exp(1j * np.radians(phi))
    assert got.dtype == np.complex128 and got.shape == inc.shape
    assert _differ(np.ascontiguousarray(got.real), np.ascontiguousarray(want.real)) == 0 and _differ(np.ascontiguousarray(got.imag), np.ascontiguousarray(want.imag)) == 0
    beyond = speed > lco.wspd[-1]  # a speed the cross-pol table holds and the co-pol table does not
    print(f"finite share {np.isfinite(got).mean():.3f}, speeds beyond the co-pol axis {beyond.mean():.3f}")
    assert beyond.mean() > 0.03 and np.isnan(got[beyond]).all() and 0.4 < np.isfinite(got).mean() < 0.95
    assert np.array_equal(np.isnan(got), np.isnan(speed) | np.isnan(phi)) and np.isnan(got[0, [0, 1, 3, 4]]).all()
    dev = torch.device("cuda", 0)
    ti, ts, tn, tscr = (torch.from_numpy(a).to(dev) for a in (inc, s, near, scr))
    tg = windspeed.retrieve_wind(ti, ts, tscr, near=tn, model=models, units="dB", resolution="low")
    tspeed, tphi = torch.from_numpy(speed).to(dev), torch.from_numpy(phi).to(dev)
    twant = tspeed * torch.exp(1j * torch.deg2rad(tphi))
    assert tg.is_cuda and tg.dtype == torch.complex128
    assert torch.equal(torch.isnan(tg.real), torch.isnan(twant.real)) and torch.equal(torch.nan_to_num(torch.view_as_real(tg)), torch.nan_to_num(torch.view_as_real(twant)))
    # wind= and complex64
    wind = (2.0 * np.exp(1j * np.radians(np.nan_to_num(near, nan=10.0)))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    g64 = windspeed.retrieve_wind(inc, s, scr, wind=wind, model=models, units="dB", resolution="low")
    g32 = windspeed.retrieve_wind(inc, s, scr, near=np.degrees(np.angle(wind)), model=models, units="dB", resolution="low", out_dtype=np.float32)
    assert g32.dtype == np.complex64 and np.array_equal(g32, g64.astype(np.complex64), equal_nan=True)


def test_user_stream_without_an_intermediate_sync(torch, delay_cycles):
    """retrieve_dir with its details and retrieve_wind on a user stream whose producer is held back, followed by dependent torch
    work on that stream: all return while the producer is in flight, and the result equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _public_scene((48, 260), np.float32, 51), _public_scene((48, 260), np.float32, 52)
    models = (KW["model"], KW_CR["model"])

    def call(b):
        r = windspeed.retrieve_dir(b[0], b[1], b[2], near=b[3], units="dB", details=True, **KW)
        v = windspeed.retrieve_wind(b[0], b[1], b[4], near=b[3], model=models, units="dB", resolution="low")
        return r.phi_near - r.phi1, r.dphi_near_dsigma0 * 2.0, r.count + r.flag, torch.view_as_real(v)[..., 0]  # dependent torch work, no synchronisation in between

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pairs = _staged(torch, list(sc), list(dec))
        ref = call([src for _, src in pairs])  # landed rasters, synchronised: LUTs installed
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
    assert np.isfinite(ref[1]).mean() > 0.3 and _same(got, ref)
