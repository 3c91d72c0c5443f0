"""CPU: what `windspeed._plan.CallPlan` answers about one `xsw_invert` call, and what `_engine.invert_numpy` then hands to
`Context.invert_raw`, against the expressions of `_engine.py` / `_lib.py` at 1fd76ea restated here (file:line beside each).

The host path runs end to end on a `Context` made without `xsw_ctx_create`: a lock, a `lut_key`, and an `invert_raw` that
records its arguments and drives the `stage` callback over uneven pieces into a numpy buffer of its own."""
import itertools
import threading

import numpy as np
import pytest

from xsarsea_amd import _lib, options
from xsarsea_amd.windspeed import _engine, _plan

F32, F64, C64, C128 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.complex64), np.dtype(np.complex128)
DTYPES = [(F32, F32), (F64, F64), (F32, F64), (F64, F32)]  # (sigma0, incidence)
ANC = [None, C64, C128]
SEARCH = ["co", "cr", "dual"]
DSIG = ["absent", "scalar", "raster"]
SHAPES = [((6, 5), (6, 5)), ((5,), (6, 5)), ((2, 3, 5), (2, 3, 5)), ((7,), (7,)), ((), ()), ((0, 5), (0, 5))]  # (incidence, sigma0)
SCALAR = 0.2  # not a float32 value: rounding it through float32 shows


@pytest.fixture
def opts():
    keep = {k: getattr(options, k) for k in ("db_on_device", "device_out_dtype", "algo", "devices", "devices_min_pixels", "host_threads")}
    yield options
    for k, v in keep.items():
        setattr(options, k, v)


def metas(dts, anc_dt, search, dsig, shapes):
    """(inc, sigma0_co, sigma0_cr, dsig_cr, anc) as the plan takes them: None, a scalar, or (shape, dtype)."""
    (s_dt, i_dt), (i_shape, s_shape) = dts, shapes
    sig = (s_shape, s_dt)
    return ((i_shape, i_dt), sig if search != "cr" else None, sig if search != "co" else None,
            {"absent": None, "scalar": SCALAR, "raster": sig}[dsig], None if anc_dt is None else (s_shape, anc_dt))


def parent(inc, co, cr, dsig, anc, device, coded=False, dual_select=False):
    """The answers of the three inversion functions of `_engine.py` at 1fd76ea, from the same metadata."""
    e = {}
    scalar = dsig is not None and np.isscalar(dsig)
    rasters = [m for m in (inc, co, cr, None if scalar else dsig) if m is not None]  # :226, :356, :421 / :431
    shape = e["shape"] = tuple(np.broadcast_shapes(*(m[0] for m in rasters + ([] if anc is None else [anc]))))  # :229, :357, :415
    n = e["n"] = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1  # :311, :378, :416
    if device:
        e["lines"], e["samples"] = (n // shape[-1], shape[-1]) if len(shape) and n else (1 if n else 0, 1 if n else 0)  # :379
    else:
        e["lines"], e["samples"] = (int(np.prod(shape[:-1])), shape[-1]) if len(shape) >= 1 and n else (0, 0)  # _lib.py:494
        if len(shape) == 0:
            e["lines"], e["samples"] = 1, 1  # _lib.py:495-496
    want_co, want_cr = e["want_co"], e["want_cr"] = co is not None, cr is not None  # :239, :414
    all_f32 = e["all_f32"] = all(m[1] == np.float32 for m in rasters) and (anc is None or anc[1] == np.complex64)  # :230, :358, :422 / :432
    e["dtype"], e["cdtype"] = (np.float32, np.complex64) if all_f32 else (np.float64, np.complex128)  # :236-238, :359, :443-444
    e["code"], e["item"] = (_lib.XSW_F32, 4) if all_f32 else (_lib.XSW_F64, 8)  # :384, :455-456
    f32_sigma0 = any(m is not None and m[1] == np.float32 for m in (co, cr))
    if device:
        is_db = not all_f32 and f32_sigma0  # :361, :423
        e["db_by"] = "torch" if is_db else "kernel"
    else:
        on_dev = options.db_on_device  # :232, :433
        if on_dev == "auto":
            on_dev = not f32_sigma0  # :234, :435 (sigma0 only, not the incidence)
        is_db = not on_dev  # :235, :436
        e["db_by"] = "numpy" if is_db else "kernel"
    e["is_db"] = is_db
    e["dsig_scalar"], e["dsig_fill"] = 0.1, None  # :372, :447, _lib.py:505
    if dsig is None:
        e["dsig"] = "none"
    elif not scalar:
        e["dsig"] = "raster"  # :264, :354, :420 / :430
    elif not want_cr:
        if device or coded:
            e["dsig"] = "none"  # :373, :448
        else:
            e["dsig"], e["dsig_scalar"] = "scalar", float(dsig)  # :264 -> _lib.py:509
    elif is_db:
        e["dsig"], e["dsig_fill"] = "fill", dsig  # :254, :368, :425, :439
    elif all_f32:
        e["dsig"], e["dsig_scalar"] = "scalar_f32", float(np.float32(dsig))  # :256, :374, :449
    else:
        e["dsig"], e["dsig_scalar"] = "scalar", float(dsig)  # _lib.py:509, :374, :449
    e["out_dtype"] = np.complex64 if (device and options.device_out_dtype == "complex64") else np.complex128  # :305, :375, :450-451
    e["out_code"], e["out_item"] = (_lib.XSW_F32, 8) if e["out_dtype"] == np.complex64 else (_lib.XSW_F64, 16)  # :385, :455-456
    e["algo"] = _lib.ALGOS.get(options.algo, options.algo)  # :387, :457, _lib.py:532
    e["fused_select"] = bool(dual_select and device and want_co and want_cr)  # :387, :458, _lib.py:478
    return e


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("db_on_device", ["auto", True, False])
@pytest.mark.parametrize("out", ["complex128", "complex64"])
def test_plan_answers_equal_the_parents(opts, device, db_on_device, out):
    opts.db_on_device, opts.device_out_dtype = db_on_device, out
    seen = set()
    for algo in ("auto", "exact", _lib.ALGO_EXHAUSTIVE_F64):
        opts.algo = algo
        for case in itertools.product(DTYPES, ANC, SEARCH, DSIG, SHAPES):
            m = metas(*case)
            for coded, dual_select in ((False, False), (False, True), (True, True)):
                plan = _plan.CallPlan(*m, device=device, coded=coded, dual_select=dual_select)
                want = parent(*m, device, coded, dual_select)
                got = {k: getattr(plan, k) for k in want}
                assert got == want, (case, coded, dual_select)
                assert type(plan.shape) is tuple and type(plan.dsig_scalar) is float
                seen.add((plan.db_by, plan.dsig))
    by = ("torch", "kernel") if device else {"auto": ("numpy", "kernel"), True: ("kernel",), False: ("numpy",)}[db_on_device]
    assert {b for b, _ in seen} == set(by)
    # every outcome the route can reach was met (host "auto" leaves no all-float32 call to the kernel's dB: no float32 rounding)
    reach = {"none", "raster", "scalar"} | ({"scalar_f32"} if device or db_on_device is True else set()) | ({"fill"} if by != ("kernel",) else set())
    assert {d for _, d in seen} == reach


def test_lines_samples_of_every_rank():
    for shape, want in (((6, 5), (6, 5)), ((2, 3, 5), (6, 5)), ((7,), (1, 7)), ((), (1, 1)), ((0, 5), (0, 0)), ((4, 0), (0, 0))):
        assert _lib.lines_samples(shape) == want


# ---- the host path end to end, on a recording stand-in --------------------------------------------------------------------

PTRS = ("inc", "sigma0_co", "sigma0_cr", "dsig_cr", "anc", "out_co", "out_cr", "out_idx", "out_code_co", "out_code_cr")


class RecordingContext:
    invert_host = _lib.Context.invert_host

    def __init__(self, log, name=0):
        self.lock, self.lut_key, self.log, self.name = threading.RLock(), (None, None), log, name

    def set_host_threads(self, n):
        self.log.append(dict(call="set_host_threads", ctx=self.name, n=n))

    def invert_raw(self, lines, samples, dtype, out_dtype, mem, inc, sigma0_co, sigma0_cr, dsig_cr, anc, out_co, out_cr, out_idx=None,
                   dsig_co=0.1, dsig_cr_scalar=0.1, sigma0_is_db=False, algo=_lib.ALGO_AUTO, dual_select=False, out_code_co=None,
                   out_code_cr=None, stage=None):
        given = dict(zip(PTRS, (inc, sigma0_co, sigma0_cr, dsig_cr, anc, out_co, out_cr, out_idx, out_code_co, out_code_cr)))
        addr = {k: None if p is None else int(getattr(p, "value", p)) for k, p in given.items()}
        rec = dict(call="invert_raw", ctx=self.name, lines=int(lines), samples=int(samples), dtype=dtype, out_dtype=out_dtype, mem=mem,
                   is_db=bool(sigma0_is_db), dsig_co=float(dsig_co), dsig_cr_scalar=float(dsig_cr_scalar), algo=algo,
                   dual_select=bool(dual_select), null={k for k, a in addr.items() if a is None},
                   as_inc={k for k, a in addr.items() if k != "inc" and a is not None and a == addr["inc"]}, addr=addr,
                   staged=None if stage is None else {})
        if stage is not None:
            n = int(lines) * int(samples)
            dt = np.float32 if dtype == _lib.XSW_F32 else np.float64
            edges = sorted({0, min(1, n), n // 3, min(n // 3 + 2, n), (2 * n) // 3 + 1 if n > 2 else n, n})
            for which in (_lib.STAGE_INC, _lib.STAGE_SIGMA0_CO, _lib.STAGE_SIGMA0_CR, _lib.STAGE_DSIG_CR, _lib.STAGE_ANC):
                buf = np.full(n + 3, -7.0, dtype=dt)
                filled = {bool(stage(which, a, b - a, buf[1 + a:1 + b].ctypes.data)) for a, b in zip(edges[:-1], edges[1:]) if b > a}
                assert len(filled) == 1, "a raster is staged for every piece or for none"
                assert buf[0] == -7.0 and (buf[n + 1:] == -7.0).all()
                if filled == {True}:
                    rec["staged"][which] = buf[1:n + 1].copy()
        self.log.append(rec)


@pytest.fixture
def recorder(monkeypatch, opts):
    log, ctxs = [], {}

    def ctx_of(device=0, replica=0):
        return ctxs.setdefault((int(device), int(replica)), RecordingContext(log, (int(device), int(replica))))

    def ensure(ctx, lut_co, lut_cr):
        other = []  # LUT install and inversion are one step under the context's lock: another thread cannot take it now
        t = threading.Thread(target=lambda: other.append(ctx.lock.acquire(blocking=False)))
        t.start()
        t.join()
        assert other == [False]
        log.append(dict(call="ensure_luts", ctx=ctx.name, luts=(lut_co, lut_cr)))

    monkeypatch.setattr(_lib, "default_context", ctx_of)
    monkeypatch.setattr(_lib, "contexts_for", lambda devs: [ctx_of(d, list(devs[:i]).count(d)) for i, d in enumerate(devs)])
    monkeypatch.setattr(_engine, "ensure_luts", ensure)
    return log


def rasters(dts, anc_dt, search, dsig, shapes, seed=5):
    (s_dt, i_dt), (i_shape, s_shape) = dts, shapes
    rng = np.random.default_rng(seed)

    def sigma0():
        x = np.asarray(rng.uniform(-0.01, 2.0, s_shape)).astype(s_dt)
        if x.size > 4:
            x.reshape(-1)[:4] = np.nan, 0.0, np.inf, -1.0
        return x

    inc = np.asarray(rng.uniform(20, 45, i_shape)).astype(i_dt)
    co, cr = (sigma0() if search != "cr" else None), (sigma0() if search != "co" else None)
    d = {"absent": None, "scalar": SCALAR, "raster": np.asarray(rng.uniform(0.1, 0.3, s_shape)).astype(s_dt)}[dsig]
    anc = None if anc_dt is None else np.asarray(rng.normal(0, 5, s_shape) + 1j * rng.normal(0, 5, s_shape)).astype(anc_dt)
    return inc, co, cr, d, anc


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_call(rec, arrays, rows=None, codes=False):
    """One recorded `invert_raw` against the parent's expressions for these rasters (rows: the tile, for tile-local offsets)."""
    inc, co, cr, dsig, anc = arrays
    e = parent(*(_plan.meta(a) for a in (inc, co, cr)), dsig if (dsig is None or np.isscalar(dsig)) else _plan.meta(dsig), _plan.meta(anc), False)
    shape = e["shape"] if rows is None else (rows[1] - rows[0],) + e["shape"][1:]
    lines, samples = (int(np.prod(shape[:-1])), shape[-1]) if len(shape) else (1, 1)  # _lib.py:494-496
    assert (rec["lines"], rec["samples"]) == (lines, samples)
    assert (rec["dtype"], rec["out_dtype"], rec["mem"]) == (e["code"], _lib.XSW_F64, _lib.MEM_HOST)  # :305, _lib.py:529-530
    assert (rec["is_db"], rec["dsig_co"], rec["dsig_cr_scalar"], rec["algo"], rec["dual_select"]) == (e["is_db"], 0.125, e["dsig_scalar"], e["algo"], False)
    null = {"out_idx"} | ({"sigma0_co"} if co is None else set()) | ({"sigma0_cr"} if cr is None else set()) | ({"anc"} if anc is None else set())
    null |= set() if e["dsig"] in ("raster", "fill") else {"dsig_cr"}  # :261-264
    for k, s in (("co", co), ("cr", cr)):  # winds or codes, for the searches that run (_lib.py:517-527)
        null |= {"out_" + k, "out_code_" + k} if s is None else ({"out_" + k} if codes else {"out_code_" + k})
    assert rec["null"] == null
    # rasters the staging callback fills are passed as the incidence pointer (:258-262)
    as_inc = ({k for k, s in (("sigma0_co", co), ("sigma0_cr", cr)) if s is not None} if e["is_db"] else set()) | ({"dsig_cr"} if e["dsig"] == "fill" else set())
    assert rec["as_inc"] == as_inc
    if not e["is_db"]:
        assert rec["staged"] is None  # :268-269
        return e
    cut = lambda a: (lambda b: b if rows is None else b[rows[0]:rows[1]])(np.broadcast_to(a, e["shape"])).reshape(-1)
    with np.errstate(all="ignore"):
        want = {w: (10 * np.log10(cut(s) + 1e-15)).astype(e["dtype"]) for w, s in ((_lib.STAGE_SIGMA0_CO, co), (_lib.STAGE_SIGMA0_CR, cr)) if s is not None}  # :246-250, :285-290
        if e["dsig"] == "fill":
            want[_lib.STAGE_DSIG_CR] = (cut(cr) * 0 + dsig).astype(e["dtype"])  # :284, from the LINEAR sigma0 in its own dtype
    assert set(rec["staged"]) == set(want)
    for w in want:
        assert rec["staged"][w].dtype == want[w].dtype and np.array_equal(bits(rec["staged"][w]), bits(want[w])), w
    return e


@pytest.mark.parametrize("db_on_device", ["auto", True, False])
@pytest.mark.parametrize("shapes", SHAPES)
def test_invert_numpy_hands_the_parents_call_to_invert_raw(recorder, db_on_device, shapes):
    options.db_on_device, options.algo, options.devices = db_on_device, "auto", None
    luts = (object(), object())
    for case in itertools.product(DTYPES, ANC, SEARCH, DSIG):
        arrays = rasters(*case, shapes)
        del recorder[:]
        out_co, out_cr = _engine.invert_numpy(*luts, *arrays, dsig_co=0.125)
        want_co, want_cr = arrays[1] is not None, arrays[2] is not None
        assert recorder[0] == dict(call="ensure_luts", ctx=(0, 0), luts=(luts[0] if want_co else None, luts[1] if want_cr else None))  # :298
        calls = [r for r in recorder if r["call"] == "invert_raw"]
        shape = np.broadcast_shapes(*(np.shape(a) for a in arrays if a is not None and not np.isscalar(a)))
        for o, want in ((out_co, want_co), (out_cr, want_cr)):
            # (a 0-d call comes back with one axis: `np.ascontiguousarray` gives every cast raster at least one, :237)
            assert (o is None) if not want else (o.shape == (shape or (1,)) and o.dtype == np.complex128)
        if 0 in shape:
            assert not calls  # _lib.py:528
            continue
        assert len(recorder) == 2 and len(calls) == 1
        check_call(calls[0], arrays)
        for o, k in ((out_co, "out_co"), (out_cr, "out_cr")):
            assert o is None or o.ctypes.data == calls[0]["addr"][k]


def test_invert_numpy_codes(recorder):
    options.db_on_device, options.devices, options.host_threads = "auto", [0, 0], 3  # codes: never tiled (:312)
    options.devices_min_pixels = 1
    arrays = rasters((F32, F32), C64, "dual", "scalar", ((16, 5), (16, 5)))
    co, cr = _engine.invert_numpy(None, None, *arrays, dsig_co=0.125, codes=True)
    assert [r["call"] for r in recorder] == ["ensure_luts", "set_host_threads", "invert_raw"] and recorder[1]["n"] == 3  # :298-300
    rec = recorder[2]
    check_call(rec, arrays, codes=True)
    assert co.dtype == cr.dtype == np.uint32 and co.shape == cr.shape == (16, 5)
    assert (co.ctypes.data, cr.ctypes.data) == (rec["addr"]["out_code_co"], rec["addr"]["out_code_cr"])


@pytest.mark.parametrize("dts,anc_dt,dsig", [((F32, F32), C64, "scalar"), ((F32, F64), None, "scalar"), ((F64, F64), C128, "raster")])
def test_invert_numpy_row_tiles(recorder, dts, anc_dt, dsig):
    """`options.devices = [0, 0]`: two contexts, row tiles in place, tile-local pixel offsets in the staging callback (:310-329)."""
    options.db_on_device, options.devices = "auto", [0, 0]
    arrays = rasters(dts, anc_dt, "dual", dsig, ((5,), (17, 5)))
    for min_px, lines, tiled in ((85, 17, True), (86, 17, False), (1, 7, False), (1, 8, True)):  # n < min_pixels, shape[0] < 4 * 2
        options.devices_min_pixels = min_px
        arr = tuple(a if (a is None or np.isscalar(a) or a.ndim < 2) else a[:lines] for a in arrays)
        del recorder[:]
        out_co, out_cr = _engine.invert_numpy(None, None, *arr, dsig_co=0.125)
        calls = sorted((r for r in recorder if r["call"] == "invert_raw"), key=lambda r: r["ctx"])
        assert out_co.shape == out_cr.shape == (lines, 5)
        if not tiled:
            assert [r["ctx"] for r in calls] == [(0, 0)]  # the first entry of `devices` (:315)
            check_call(calls[0], arr)
            continue
        assert [r["ctx"] for r in calls] == [(0, 0), (0, 1)]
        assert sorted(r["ctx"] for r in recorder if r["call"] == "ensure_luts") == [(0, 0), (0, 1)]
        tiles = [(0, lines // 2), (lines // 2, lines)]  # tile_rows: the last tile takes the remainder
        for rec, rows in zip(calls, tiles):
            e = check_call(rec, arr, rows=rows)
            for o, k in ((out_co, "out_co"), (out_cr, "out_cr")):
                assert rec["addr"][k] == o.ctypes.data + rows[0] * 5 * 16  # written in place
        # every raster pointer of the second tile stands `rows` further in the same raster
        for k in ("inc", "sigma0_co", "sigma0_cr") + (("dsig_cr",) if e["dsig"] in ("raster", "fill") else ()):
            assert calls[1]["addr"][k] - calls[0]["addr"][k] == tiles[1][0] * 5 * e["item"]
        if anc_dt is not None:
            assert calls[1]["addr"]["anc"] - calls[0]["addr"]["anc"] == tiles[1][0] * 5 * 2 * e["item"]


# ---- the device materialise step and the chunk closures, on CPU tensors ----------------------------------------------------

@pytest.mark.parametrize("s_dt,i_dt,a_dt,dsig", [(np.float32, np.float32, np.complex64, SCALAR), (np.float32, np.float64, None, SCALAR),
                                                 (np.float64, np.float64, np.complex128, None), (np.float32, np.float64, np.complex64, "raster"),
                                                 (np.float64, np.float32, None, SCALAR)])
def test_device_rasters_are_the_parents_tensors(monkeypatch, opts, s_dt, i_dt, a_dt, dsig):
    """`_engine._device_rasters` (behind `invert_device` and the device branch of `invert_coded`) against :351-374 restated."""
    import torch
    from xsarsea_amd import _device
    monkeypatch.setattr(_device, "device_of", lambda *a: torch.device("cpu"))
    rng = np.random.default_rng(2)
    co, cr = (torch.from_numpy(rng.uniform(0, 1, (6, 5)).astype(s_dt)) for _ in range(2))
    inc = torch.from_numpy(rng.uniform(20, 40, (5,)).astype(i_dt))
    anc = None if a_dt is None else torch.from_numpy((rng.normal(size=(6, 5)) + 1j).astype(a_dt))
    d = torch.from_numpy(rng.uniform(.1, .3, (6, 5)).astype(s_dt)) if dsig == "raster" else dsig
    plan, dev, t = _engine._device_rasters(inc, co, cr, d, anc, True, broadcast=torch.broadcast_shapes)
    t_d = d if dsig == "raster" else None  # :354
    rasters = [x for x in (inc, co, cr, t_d) if x is not None]  # :356
    all_f32 = all(x.dtype == torch.float32 for x in rasters) and (anc is None or anc.dtype == torch.complex64)  # :358
    rt, ct = (torch.float32, torch.complex64) if all_f32 else (torch.float64, torch.complex128)  # :359
    t_co, t_cr, is_db = co, cr, False
    if not all_f32 and co.dtype == torch.float32:  # :361
        if t_d is None and d is not None:
            t_d = t_cr * 0 + d  # :368, from the LINEAR sigma0
        t_co, t_cr, is_db = 10 * torch.log10(t_co + 1e-15), 10 * torch.log10(t_cr + 1e-15), True  # :364, :369
    prep = lambda x, dt: None if x is None else x.to(dt).expand((6, 5)).contiguous()  # :370
    for got, want in zip(t, (prep(inc, rt), prep(t_co, rt), prep(t_cr, rt), prep(t_d, rt), prep(anc, ct))):
        assert (got is None) == (want is None)
        assert got is None or (got.dtype == want.dtype and got.is_contiguous() and got.shape == (6, 5) and torch.equal(got, want))
    assert (plan.is_db, plan.fused_select, plan.shape, dev) == (is_db, True, (6, 5), torch.device("cpu"))
    # rasters that do not broadcast: `invert_device` raises torch's error, as `torch.broadcast_shapes` did at :357
    with pytest.raises(RuntimeError):
        _engine._device_rasters(inc, co[:, :4], cr, d, anc, True, broadcast=torch.broadcast_shapes)


@pytest.mark.parametrize("flat", [False, True])
def test_chunk_calls_arguments_and_lifetime(monkeypatch, flat):
    """`multi_gpu.chunk_calls` (behind `invert_coded` and `invert_tiled_device`): the argument order and addresses of
    :496-509 / multi_gpu.py:300-310, and that tensors a `sigma0` hook makes for one chunk are alive while `invert_raw` runs and
    are tied to the launch stream only after it (at :487-493 they were locals of `invert_chunk`)."""
    import gc
    import weakref
    import torch
    from xsarsea_amd import _device, multi_gpu
    S, log = 5, []

    class Pipe:
        samples, device = S, "dev"
        codes, codes_dual = torch.zeros(6, S, dtype=torch.int32), torch.zeros(6, S, dtype=torch.int32)
        full_codes, full_codes_dual = codes, codes_dual
        full, full_dual = torch.zeros(6, S, dtype=torch.complex64), torch.zeros(6, S, dtype=torch.complex64)

    class Ctx:
        def invert_raw(self, *a, **k):
            gc.collect()
            log.append(("invert_raw", a, k, [w() is not None for w in made]))

        def expand_codes_on_stream(self, *a):
            log.append(("expand", a))

    monkeypatch.setattr(_device, "keep_alive", lambda tensors, device: log.append(("keep_alive", [id(x) for x in tensors], device)))
    pipe, made = Pipe(), []
    inc, co, anc = torch.zeros(6, S, dtype=torch.float64), torch.ones(6, S, dtype=torch.float64), torch.zeros(6, S, dtype=torch.complex128)
    scalars = (0.125, 0.25, True, _lib.ALGO_EXACT, False)
    ic, er = multi_gpu.chunk_calls(Ctx(), pipe, (inc, co, None, None, anc), _lib.XSW_F64, _lib.XSW_F32, _lib.MEM_DEVICE, scalars,
                                   flat=flat, second=False)
    ic(0, 2, 4)
    (_, a, k, _), keep = log
    assert a[:5] == ((1, 2 * S) if flat else (2, S)) + (_lib.XSW_F64, _lib.XSW_F32, _lib.MEM_DEVICE)
    assert a[5:10] == (inc.data_ptr() + 2 * S * 8, co.data_ptr() + 2 * S * 8, None, None, anc.data_ptr() + 2 * S * 16)
    assert a[10:] == (None, None, None) + scalars
    assert k == dict(out_code_co=pipe.codes.data_ptr() + 2 * S * 4, out_code_cr=None, stage=None) and keep == ("keep_alive", [], "dev")
    er(2, 4, type("S", (), {"cuda_stream": 7})())
    assert log[2] == ("expand", (7, 2 * S, _lib.XSW_F32, pipe.full_codes.data_ptr() + 2 * S * 4, None, pipe.full.data_ptr() + 2 * S * 8, None))

    def hook(off, npx, lines):
        up = torch.full((npx,), 3.0, dtype=torch.float64)
        made.append(weakref.ref(up))
        return _lib.MEM_DEVICE_SIGMA0_HOST, up.data_ptr(), None, "stage", [up]

    del log[:]
    ic, er = multi_gpu.chunk_calls(Ctx(), pipe, (inc, None, None, None, anc), _lib.XSW_F64, _lib.XSW_F32, _lib.MEM_DEVICE, scalars, sigma0=hook)
    ic(1, 4, 6)
    (_, a, k, alive), keep = log
    assert alive == [True] and a[4] == _lib.MEM_DEVICE_SIGMA0_HOST and a[7] is None and k["stage"] == "stage"
    assert k["out_code_cr"] == pipe.codes_dual.data_ptr() + 4 * S * 4 and keep[0] == "keep_alive" and len(keep[1]) == 1
    gc.collect()
    assert made[0]() is None  # nothing else keeps a chunk's tensors
