"""GPU: wind speed at a known direction (xsw_wspd_solve / xsw_wspd_solve_cr, kernels k_wspd_solve_co / k_wspd_solve_cr;
`windspeed.retrieve_wspd`).

The yardstick everywhere is the numpy restatement tests/solve_ref.py (held to its plain meaning and to the forward restatement by
tests/test_solve_cpu.py), evaluated on the table READ BACK from the context (xsw_lut_read), never on a host-built copy.  Every
real output and the flag must equal it bit for bit, NaN positions included; float32 outputs are the restatement rounded once.
Only IEEE + - * / in float64 follow the cell search, so there is no tolerance."""
import itertools
import warnings

import numpy as np
import pytest

import forward_ref as fref
import solve_ref as sref
from test_gpu_forward import GUARD, MARGINS, SENTINEL, Installed, _differ, default_tables  # noqa: F401 (fixture)
from test_gpu_streams import _held_back, _in_flight, _read_back, _staged, delay_cycles, torch  # noqa: F401 (fixtures)
from util import lut_dicts

from oracle import lut as olut

pytestmark = pytest.mark.gpu

FLAG_SENTINEL = np.uint8(0xA5)  # no combination of the XSW_SOLVE_* bits
FIELDS = ("wspd", "sens", "flag")


def _solve(ctx, torch, _lib, kind, arrs, out_t, want=(1, 1, 1), mem=None, fold=True):
    """The raw entry on device rasters (or, mem = MEM_HOST, host arrays).  kind "co": arrs = (inc, sigma0_db, phi); "cr": (inc,
    sigma0_db) -> [wspd, sens, flag].  Every requested output lies between two guard regions and starts as its sentinel; returns
    host arrays (None where not requested) after checking that the guards are untouched and every pixel was written."""
    inc = arrs[0]
    shape, n = inc.shape, inc.size
    dt, od = (_lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64), (_lib.XSW_F32 if out_t == np.float32 else _lib.XSW_F64)
    types = (out_t, out_t, np.uint8)
    sents = (SENTINEL[out_t], SENTINEL[out_t], FLAG_SENTINEL)
    hosts = [np.ascontiguousarray(a if n else np.zeros(1, a.dtype)) for a in arrs]  # an empty raster: no pointer is NULL
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
    lines, samples = (shape[0], shape[1]) if len(shape) == 2 else _lib.lines_samples(shape)
    m = _lib.MEM_HOST if host_route else _lib.MEM_DEVICE
    if kind == "co":
        ctx.wspd_solve_raw(lines, samples, dt, od, m, *ins, *outs, fold_phi=fold)
    else:
        ctx.wspd_solve_cr_raw(lines, samples, dt, od, m, *ins, *outs)
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
        if k == "flag":
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


class Tables:
    """What the restatement needs of an `Installed` pair: the read-back tables, their axes, and mono_rows / cr_monotone derived
    from them as the install derives them."""

    def __init__(self, tab):
        self.tab, self.ctx = tab, tab.ctx
        self.co, self.cr = (tab.co, *tab.co_axes), (tab.cr, *tab.cr_axes)
        self.mono, self.cr_mono = sref.mono_rows(tab.co), sref.cr_monotone(tab.cr, tab.cr_axes[1])

    def ref_co(self, inc, s, phi, fold=True):
        return sref.solve_co(*self.co, inc, s, phi, fold_phi=fold, mono=self.mono)

    def ref_cr(self, inc, s):
        return sref.solve_cr(*self.cr, inc, s, monotone=self.cr_mono)


def _luts(co, cr):
    return olut.Lut(co[0], co[1], co[2], co[3], "dB", "x", "co", "VV"), olut.Lut(cr[0], cr[1], cr[2], None, "dB", "x", "cr", "VH")


def _scene(t, shape, dtype, seed=0):
    """(inc, s_co, phi, s_cr) rasters of `dtype`: inc and phi from forward_ref.points with the margins of tests/test_gpu_forward.py
    (beyond the axes, on nodes, one NaN each), half of the directions from -200 to 400 degrees; s the restated forward value at a
    uniform speed plus N(0, 0.5 dB) (NaN where the incidence is outside or NaN)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    inc, _, p = fref.points(rng, t.co[1:], n, MARGINS)
    p2 = rng.uniform(-200.0, 400.0, n)
    p = np.where((rng.random(n) < 0.5) & ~np.isnan(p), p2, p)
    w = rng.uniform(t.co[2][0], t.co[2][-1], n)
    wcr = rng.uniform(t.cr[2][0], t.cr[2][-1], n)
    s = fref.eval_co(*t.co, inc, w, p)["sigma0_db"] + rng.normal(0.0, 0.5, n)
    scr = fref.eval_cr(*t.cr, inc, wcr)["sigma0_db"] + rng.normal(0.0, 0.5, n)
    return tuple(a.reshape(shape).astype(dtype) for a in (inc, s, p, scr))


def _shares(flag):
    return dict(lead=float((flag == 0).mean()), tail=float((flag == sref.TAIL).mean()),
                out=float(((flag == sref.BELOW) | (flag == sref.ABOVE)).mean()), nan=float((flag == sref.NAN).mean()))


@pytest.mark.parametrize("out_t", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bit_equal_to_the_restatement(default_tables, torch, dtype, out_t):
    """70 x 333 (ragged last block) on the default LUTs: co-pol with and without the fold, cross-pol.  The classes of the
    restatement's answer are asserted first, so that none is empty: a solution in the leading rows, one past them (TAIL), none
    (BELOW / ABOVE), NaN."""
    from xsarsea_amd import _lib
    t = Tables(default_tables)
    assert t.cr_mono and 2 <= t.mono.min() < t.mono.max() == len(t.co[2])
    inc, s, p, scr = _scene(t, (70, 333), dtype)
    for fold in (True, False):
        want = t.ref_co(inc, s, p, fold)
        sh = _shares(want["flag"])
        print(f"co-pol, fold {fold}: {sh}")
        if fold:
            assert sh["lead"] >= 0.5 and sh["tail"] >= 0.02 and sh["out"] >= 0.02 and sh["nan"] >= 0.05
        got = _solve(t.ctx, torch, _lib, "co", (inc, s, p), out_t, fold=fold)
        _assert_fields(got, want, out_t, f"co-pol, fold {fold}")
        assert np.array_equal(np.isnan(got[0]), (got[2] & 7) != 0) and np.array_equal(np.isnan(got[1]), np.isnan(got[0]))
    want = t.ref_cr(inc, scr)
    sh = _shares(want["flag"])
    print(f"cross-pol: {sh}")
    assert sh["lead"] >= 0.5 and sh["out"] >= 0.02 and sh["nan"] >= 0.05 and sh["tail"] == 0  # (every row of the default table rises)
    got = _solve(t.ctx, torch, _lib, "cr", (inc, scr), out_t)
    _assert_fields(got, want, out_t, "cross-pol")


# ------------------------------------------------------------------------------------------------ every cell and node of a table
def _nodes_and_centres(ax):
    out = np.empty(2 * len(ax) - 1)
    out[0::2], out[1::2] = ax, 0.5 * (ax[:-1] + ax[1:])
    return out


def _small_tables(name):
    if name == "nonuniform_11x9":  # phi_pad = 12; the cross-pol speed axis is not uniform: scanned
        return fref.nonuniform_tables()
    if name in ("turnover", "turnover_flat"):
        co, ai, aw, ap = sref.turnover_table()[:4]
        if name == "turnover_flat":  # its first cell flat: the one place where a flat cell is the lowest bracket
            co = co.copy()
            co[:, 1] = co[:, 0]
        return (co, ai, aw, ap), sref.nonmonotone_cr()
    cr, ai, aw = sref.nonmonotone_cr()
    return sref.falling_table()[:4], (np.sort(cr, axis=1), ai, aw)  # (a small cross-pol table that IS monotone: bisected)


@pytest.mark.parametrize("name", ["nonuniform_11x9", "turnover", "turnover_flat", "falling"])
def test_every_cell_and_node(gpu_ctx, torch, name):
    """Every node and cell centre of the incidence and direction axes, and at each of them s on every node value c(k) and midway
    through every cell of the column, half a dB below the lowest and above the highest: as one raster."""
    from xsarsea_amd import _lib
    co, cr = _small_tables(name)
    t = Tables(Installed(gpu_ctx, *_luts(co, cr)))
    assert t.cr_mono == (name == "falling")
    assert np.array_equal(t.mono, {"nonuniform_11x9": [11, 11, 11], "turnover": [4, 3, 8], "turnover_flat": [4, 3, 8], "falling": [1, 1]}[name])
    n_w = len(t.co[2])
    gi, gp = _nodes_and_centres(t.co[1]), _nodes_and_centres(t.co[3])
    for fold in (False, True):
        pp = np.concatenate([gp, -gp, gp + 360.0]) if fold else gp
        inc, p = (a.ravel() for a in np.meshgrid(gi, pp, indexing="ij"))
        C = np.stack([sref.node_values(t.co[0], t.co[1], t.co[3], inc, p, np.full(len(inc), k), fold_phi=fold) for k in range(n_w)], axis=1)
        assert np.isfinite(C).all()  # (the mirror images fold back into the table, whatever its last direction)
        s = np.concatenate([C, 0.5 * (C[:, :-1] + C[:, 1:]), C.min(axis=1, keepdims=True) - 0.5, C.max(axis=1, keepdims=True) + 0.5], axis=1)
        inc, p = (np.repeat(a[:, None], s.shape[1], axis=1) for a in (inc, p))
        got = _solve(gpu_ctx, torch, _lib, "co", (inc, s, p), np.float64, fold=fold)
        want = t.ref_co(inc, s, p, fold)
        _assert_fields(got, want, np.float64, f"{name}, fold {fold}")
        if not fold:
            sh = _shares(want["flag"])
            print(name, sh)
            assert sh["nan"] == 0 and sh["out"] > 0 and (sh["tail"] > 0) == (name != "nonuniform_11x9") and (sh["lead"] > 0) == (name != "falling")
            assert np.isinf(got[1]).any() == (name == "turnover_flat") and not np.isnan(got[0][np.isinf(got[1])]).any()
    gi = _nodes_and_centres(t.cr[1])
    C = np.stack([sref.node_values(t.cr[0], t.cr[1], None, gi, None, np.full(len(gi), k)) for k in range(len(t.cr[2]))], axis=1)
    s = np.concatenate([C, 0.5 * (C[:, :-1] + C[:, 1:]), C.min(axis=1, keepdims=True) - 0.5, C.max(axis=1, keepdims=True) + 0.5], axis=1)
    inc = np.repeat(gi[:, None], s.shape[1], axis=1)
    got = _solve(gpu_ctx, torch, _lib, "cr", (inc, s), np.float64)
    want = t.ref_cr(inc, s)
    _assert_fields(got, want, np.float64, f"{name} cross-pol")
    sh = _shares(want["flag"])
    assert sh["out"] > 0 and (sh["tail"] > 0) == (not t.cr_mono) and (sh["lead"] > 0) == t.cr_mono


# ------------------------------------------------------------------------------------------------ shapes, routes, outputs
@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (1, 256), (1, 257), (2, 3, 43), (0, 5)])
def test_small_shapes_and_host_route(default_tables, torch, shape):
    """One lane, one short of / exactly / one past a block, three axes (through lines_samples), no pixel at all (the calls return
    and write nothing); the host route equals the device route."""
    from xsarsea_amd import _lib
    t = Tables(default_tables)
    if 0 in shape:
        z = np.zeros(shape)
        for mem in (None, _lib.MEM_HOST):
            assert all(g.shape == shape for g in _solve(t.ctx, torch, _lib, "co", (z, z, z), np.float64, mem=mem))
            assert all(g.shape == shape for g in _solve(t.ctx, torch, _lib, "cr", (z, z), np.float32, mem=mem))
        return
    rng = np.random.default_rng(7)
    inc, w, p = rng.uniform(17, 65, shape), rng.uniform(0.3, 20, shape), rng.uniform(-180, 180, shape)
    s = fref.eval_co(*t.co, inc, w, p)["sigma0_db"]
    dev = _solve(t.ctx, torch, _lib, "co", (inc, s, p), np.float64)
    _assert_fields(dev, t.ref_co(inc, s, p), np.float64, f"{shape} co-pol")
    assert np.isfinite(dev[0]).all() and np.abs(dev[0] - w).max() < 1e-6  # (below the turn-over: the speed itself comes back)
    assert _same(_solve(t.ctx, torch, _lib, "co", (inc, s, p), np.float64, mem=_lib.MEM_HOST), dev)
    wcr = rng.uniform(3.5, 79, shape)
    s = fref.eval_cr(*t.cr, inc, wcr)["sigma0_db"]
    dev = _solve(t.ctx, torch, _lib, "cr", (inc, s), np.float64)
    _assert_fields(dev, t.ref_cr(inc, s), np.float64, f"{shape} cross-pol")
    assert np.isfinite(dev[0]).all()
    assert _same(_solve(t.ctx, torch, _lib, "cr", (inc, s), np.float64, mem=_lib.MEM_HOST), dev)


def test_host_route_equals_device_route(default_tables, torch):
    from xsarsea_amd import _lib
    t = Tables(default_tables)
    for dtype, out_t in ((np.float32, np.float64), (np.float64, np.float32)):
        inc, s, p, scr = _scene(t, (9, 333), dtype, 3)
        assert _same(_solve(t.ctx, torch, _lib, "co", (inc, s, p), out_t, mem=_lib.MEM_HOST), _solve(t.ctx, torch, _lib, "co", (inc, s, p), out_t))
        assert _same(_solve(t.ctx, torch, _lib, "cr", (inc, scr), out_t, mem=_lib.MEM_HOST), _solve(t.ctx, torch, _lib, "cr", (inc, scr), out_t))


def test_every_subset_of_outputs(default_tables, torch):
    """All 7 non-empty subsets of (wspd, sens, flag), each output left out in turn among them: a requested output equals the full
    call's, an unrequested one is never written (`_solve` checks the guard regions of every buffer it hands over)."""
    from xsarsea_amd import _lib
    t = Tables(default_tables)
    inc, s, p, scr = _scene(t, (5, 333), np.float32, 4)
    for kind, arrs in (("co", (inc, s, p)), ("cr", (inc, scr))):
        full = _solve(t.ctx, torch, _lib, kind, arrs, np.float64)
        for sub in [x for x in itertools.product((0, 1), repeat=3) if any(x)]:
            for mem in (None, _lib.MEM_HOST):
                got = _solve(t.ctx, torch, _lib, kind, arrs, np.float64, want=sub, mem=mem)
                assert all((g is None) == (not k) for g, k in zip(got, sub))
                assert _same(got, [f if k else None for f, k in zip(full, sub)]), (kind, sub, mem)


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
        co = lambda ins=(a, a, a), outs=(o, None, f), shape=(2, 8), dt=0, od=0, mem=0: ctx._lib.xsw_wspd_solve(
            ctx._h, *shape, dt, od, mem, 1, *(at(x) for x in ins), *(at(x) for x in outs))
        cr = lambda ins=(a, a), outs=(o, None, f), shape=(2, 8), dt=0, od=0, mem=0: ctx._lib.xsw_wspd_solve_cr(
            ctx._h, *shape, dt, od, mem, *(at(x) for x in ins), *(at(x) for x in outs))
        assert co() == -3 and "no co-pol LUT" in msg()
        assert cr() == -3 and "no cross-pol LUT" in msg()
        ai, aw = np.array([20.0, 30.0, 45.0]), np.linspace(1.0, 9.0, 9)
        lco = olut.Lut(np.zeros((3, 9, 1)), ai, aw, np.array([0.0]), "dB", "x", "co", "VV")
        lcr = olut.Lut(np.zeros((3, 1)), ai, aw[:1], None, "dB", "x", "cr", "VH")
        ctx.upload_luts(*lut_dicts(lco, lcr))
        assert co() == -1 and "fewer than two points" in msg()
        assert cr() == -1 and "fewer than two points" in msg()
        ctx.upload_luts(*lut_dicts(*_luts(*_small_tables("turnover"))))
        assert co() == 0 and cr() == 0 and not np.any(o == 77.0) and not np.any(f == 0xA5)
        o[:], f[:] = 77.0, 0xA5
        for k in range(3):
            ins = [a, a, a]
            ins[k] = None
            assert co(ins=ins) == -1 and "NULL" in msg()
        assert cr(ins=(None, a)) == -1 and cr(ins=(a, None)) == -1 and "NULL" in msg()
        assert co(outs=(None, None, None)) == -1 and "no output" in msg()
        assert cr(outs=(None, None, None)) == -1 and "no output" in msg()
        assert co(shape=(-1, 8)) == -1 and co(dt=2) == -1 and co(od=5) == -1 and co(mem=9) == -1
        assert cr(shape=(2, -8)) == -1 and cr(dt=2) == -1 and cr(mem=9) == -1
        assert co(shape=(1 << 31, 1 << 20)) == -1 and "too large" in msg()
        assert cr(shape=(1 << 31, 1 << 20)) == -1 and "too large" in msg()
        assert co(shape=(0, 8)) == 0 and cr(shape=(0, 0)) == 0  # an empty raster: XSW_OK, nothing written
        assert np.all(o == 77.0) and np.all(f == 0xA5)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public interface
KW = dict(model="gmf_cmod5n", resolution="low")
KW_CR = dict(model="gmf_s1_v2", resolution="low")


def _public_scene(shape, dtype, seed):
    """(inc, sigma0_db, phi, sigma0_cr_db): the models' own tables at a uniform wind, 0.3 dB of noise, a NaN in each raster."""
    from xsarsea_amd import windspeed
    rng = np.random.default_rng(seed)
    inc, w, p = rng.uniform(15.5, 66.5, shape), rng.uniform(0.5, 45.0, shape), rng.uniform(-200.0, 400.0, shape)
    s = windspeed.simulate_sigma0(inc, w, p, **KW) + rng.normal(0.0, 0.3, shape)
    scr = windspeed.simulate_sigma0(inc, rng.uniform(3.5, 70.0, shape), **KW_CR) + rng.normal(0.0, 0.3, shape)
    inc[0, 0], s[0, 1], p[0, 2], scr[0, 3] = np.nan, np.nan, np.nan, np.nan
    return inc.astype(dtype), s.astype(dtype), p.astype(dtype), scr.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_retrieve_wspd_numpy_and_torch(torch, dtype):
    """`retrieve_wspd` on numpy rasters and on torch tensors == the raw entries on the context it installed its table in == the
    restatement on that table; simulate_sigma0 of the answer gives sigma0 back; wind= is phi= with the raster's angle."""
    from xsarsea_amd import _lib, windspeed
    from xsarsea_amd.windspeed import _engine
    inc, s, p, scr = _public_scene((33, 130), dtype, 21)
    dev = torch.device("cuda", 0)
    ti, ts, tp, tscr = (torch.from_numpy(a).to(dev) for a in (inc, s, p, scr))
    ctx = _lib.default_context(0)
    for fold in (True, False):
        r = windspeed.retrieve_wspd(inc, s, p, units="dB", details=True, fold_phi=fold, **KW)
        raw = _solve(ctx, torch, _lib, "co", (inc, s, p), np.float64, fold=fold)
        assert _same([r.wspd, r.dwspd_dsigma0, r.flag], raw) and r.wspd.dtype == np.float64 and r.flag.dtype == np.uint8
        lut = _engine.lut_source(windspeed.get_model(KW["model"]), dict(resolution="low"))
        table = ctx.read_lut(lut.shape)
        want = sref.solve_co(table, lut.incidence, lut.wspd, lut.phi, inc, s, p, fold_phi=fold)
        _assert_fields(raw, want, np.float64, f"public, fold {fold}")
        tr = windspeed.retrieve_wspd(ti, ts, tp, units="dB", details=True, fold_phi=fold, **KW)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (tr.wspd, tr.dwspd_dsigma0, tr.flag)) and tr.flag.dtype == torch.uint8
        assert _same([x.cpu().numpy() for x in (tr.wspd, tr.dwspd_dsigma0, tr.flag)], raw)
        solved = (raw[2] & 7) == 0
        print(f"fold {fold}: solved share {solved.mean():.3f}")
        assert (solved.mean() > 0.5) if fold else (0.1 < solved.mean() < 0.5)
        # the round trip through the forward operator: to rounding (its axis order differs), on the float64 rasters the kernels read
        back = windspeed.simulate_sigma0(inc.astype(np.float64), raw[0], p.astype(np.float64), fold_phi=fold, **KW)
        err = np.abs(back - s.astype(np.float64))[solved].max()
        print(f"round trip: {err:.3g} dB")
        assert err <= 1e-10 and np.isfinite(back[solved]).all()
    # the speed alone, float32 out, linear units (the array module's own dB)
    w32 = windspeed.retrieve_wspd(inc, s, p, units="dB", out_dtype=np.float32, **KW)
    assert w32.dtype == np.float32 and _differ(w32, _solve(ctx, torch, _lib, "co", (inc, s, p), np.float32)[0]) == 0
    lin = (10 ** (s / 10)).astype(dtype)
    assert _differ(windspeed.retrieve_wspd(inc, lin, p, **KW), windspeed.retrieve_wspd(inc, _engine._to_db(lin), p, units="dB", **KW)) == 0
    tl = torch.from_numpy(lin).to(dev)
    assert _differ(windspeed.retrieve_wspd(ti, tl, tp, **KW).cpu().numpy(),
                   windspeed.retrieve_wspd(ti, 10 * torch.log10(tl + 1e-15), tp, units="dB", **KW).cpu().numpy()) == 0
    # wind=: an ancillary_from_streaks-style complex raster; only its angle is used
    wind = (7.0 * np.exp(1j * np.deg2rad(np.nan_to_num(p, nan=10.0)))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    assert _differ(windspeed.retrieve_wspd(inc, s, wind=wind, units="dB", **KW), windspeed.retrieve_wspd(inc, s, np.degrees(np.angle(wind)), units="dB", **KW)) == 0
    tw = torch.from_numpy(wind).to(dev)
    assert _differ(windspeed.retrieve_wspd(ti, ts, wind=tw, units="dB", **KW).cpu().numpy(),
                   windspeed.retrieve_wspd(ti, ts, torch.rad2deg(torch.angle(tw)), units="dB", **KW).cpu().numpy()) == 0
    # a scalar direction is expanded; an empty raster
    assert _differ(windspeed.retrieve_wspd(inc, s, 30, units="dB", **KW), windspeed.retrieve_wspd(inc, s, np.full_like(inc, 30), units="dB", **KW)) == 0
    assert windspeed.retrieve_wspd(inc[:0], s[:0], p[:0], **KW).shape == (0, 130)
    assert tuple(windspeed.retrieve_wspd(ti[:0], ts[:0], tp[:0], details=True, **KW).flag.shape) == (0, 130)
    # cross-pol: no direction
    rc = windspeed.retrieve_wspd(inc, scr, units="dB", details=True, **KW_CR)
    raw = _solve(ctx, torch, _lib, "cr", (inc, scr), np.float64)
    assert _same([rc.wspd, rc.dwspd_dsigma0, rc.flag], raw) and np.isfinite(raw[0]).mean() > 0.5
    lut = _engine.lut_source(windspeed.get_model(KW_CR["model"]), dict(resolution="low"))
    _assert_fields(raw, sref.solve_cr(ctx.read_lut(lut.shape, cross=True), lut.incidence, lut.wspd, inc, scr), np.float64, "public cross-pol")
    tc = windspeed.retrieve_wspd(ti, tscr, units="dB", details=True, **KW_CR)
    assert _same([x.cpu().numpy() for x in (tc.wspd, tc.dwspd_dsigma0, tc.flag)], raw)
    solved = (raw[2] & 7) == 0
    back = windspeed.simulate_sigma0(inc.astype(np.float64), raw[0], **KW_CR)
    assert np.abs(back - scr.astype(np.float64))[solved].max() <= 1e-10


def test_user_stream_without_an_intermediate_sync(torch, delay_cycles):
    """retrieve_wspd (co-pol with its details, cross-pol) on a user stream whose producer is held back, followed by dependent
    torch work on that stream: all return while the producer is in flight, and the result equals the synchronised run."""
    from xsarsea_amd import windspeed
    sc, dec = _public_scene((48, 260), np.float32, 51), _public_scene((48, 260), np.float32, 52)

    def call(b):
        r = windspeed.retrieve_wspd(b[0], b[1], b[2], units="dB", details=True, **KW)
        vh = windspeed.retrieve_wspd(b[0], b[3], units="dB", **KW_CR)
        return r.wspd - vh, r.dwspd_dsigma0 * 2.0, r.flag + 1  # dependent torch work, no synchronisation in between

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
    assert np.isfinite(ref[1]).mean() > 0.5 and _same(got, ref)
