"""CPU: what the numpy side of `_engine.cross_from_codes`, `cost_from_codes` and `cost_cr_from_codes` hands to the `*_raw`
methods of a context, against the expressions of `cross_numpy`, `cost_numpy` and `cost_cr_numpy` of `_engine.py` at 0a2d5eb
restated here (file:line beside each; `_plan.py` is that commit's too).

As in test_engine_plan.py the `Context` is made without `xsw_ctx_create`: a lock, a `lut_key`, and `*_raw` methods that record
their arguments and copy the host buffers behind the addresses they are given."""
import ctypes
import threading

import numpy as np
import pytest

from xsarsea_amd import _lib, options
from xsarsea_amd.windspeed import _engine, _plan

SCALAR = 0.2  # not a float32 value: rounding it through float32 would show
SHAPES = [(6, 10), (1, 7)]
DTYPES = [np.float32, np.float64]
DSIG = ["absent", "scalar", "raster"]
DB = ["auto", False]
INPUTS = {"cross": ("inc", "code_co", "sigma0", "dsig_cr"), "cost": ("inc", "code_co", "sigma0", "anc"),
          "cost_cr": ("inc", "code_co", "code_cr", "sigma0", "dsig_cr")}


class RecordingContext:
    def __init__(self, log):
        self.lock, self.lut_key, self.log = threading.RLock(), (None, None), log

    def _record(self, call, lines, samples, dtype, out_dtype, mem, inputs, outputs, **scalars):
        n, es = int(lines) * int(samples), 4 if dtype == _lib.XSW_F32 else 8
        size = {"code_co": 4, "code_cr": 4, "anc": 2 * es}
        self.log.append(dict(call=call, lines=int(lines), samples=int(samples), dtype=dtype, out_dtype=out_dtype, mem=mem, outputs=outputs,
                             bytes={k: None if p is None else ctypes.string_at(int(p), n * size.get(k, es)) for k, p in zip(INPUTS[call], inputs)},
                             **scalars))

    def cross_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_cr, dsig_cr, out_code_cr, out_cr,
                             dsig_cr_scalar=0.1, sigma0_is_db=False, dual_select=False):
        self._record("cross", lines, samples, dtype, out_dtype, mem, (inc, code_co, sigma0_cr, dsig_cr), (out_code_cr, out_cr),
                     dsig_cr_scalar=dsig_cr_scalar, is_db=sigma0_is_db, dual_select=dual_select)

    def cost_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, sigma0_co, anc, out_J, out_Jsig=None, out_Jwind=None,
                            out_residual=None, dsig_co=0.1, sigma0_is_db=False):
        self._record("cost", lines, samples, dtype, out_dtype, mem, (inc, code_co, sigma0_co, anc), (out_J, out_Jsig, out_Jwind, out_residual),
                     dsig_co=dsig_co, is_db=sigma0_is_db)

    def cost_cr_from_codes_raw(self, lines, samples, dtype, out_dtype, mem, inc, code_co, code_cr, sigma0_cr, dsig_cr, out_J, out_Jsig=None,
                               out_Jwind=None, out_residual=None, dsig_cr_scalar=0.1, sigma0_is_db=False):
        self._record("cost_cr", lines, samples, dtype, out_dtype, mem, (inc, code_co, code_cr, sigma0_cr, dsig_cr),
                     (out_J, out_Jsig, out_Jwind, out_residual), dsig_cr_scalar=dsig_cr_scalar, is_db=sigma0_is_db)


@pytest.fixture
def recorder(monkeypatch):
    keep = options.db_on_device
    log = []
    ctx = RecordingContext(log)

    def ensure(c, lut_co, lut_cr):
        other = []  # LUT install and kernel call are one step under the context's lock (:432, :487, :534)
        t = threading.Thread(target=lambda: other.append(c.lock.acquire(blocking=False)))
        t.start()
        t.join()
        assert c is ctx and other == [False]
        log.append(dict(call="ensure_luts", luts=(lut_co, lut_cr)))

    monkeypatch.setattr(_lib, "default_context", lambda device=0, replica=0: ctx)
    monkeypatch.setattr(_engine, "ensure_luts", ensure)
    yield log
    options.db_on_device = keep


def scene(shape, dt, dsig_kind):
    """A 1-D incidence row (broadcast over the lines), the sigma0 the codes belong to with the values dB is delicate for, the
    ancillary wind, dsig_cr of the asked kind, two code arrays (int32 holding uint32 bit patterns, as a torch caller has them)."""
    rng = np.random.default_rng(shape[1])
    inc = rng.uniform(20, 45, shape[1]).astype(dt)
    s = rng.uniform(-0.01, 2.0, shape).astype(dt)
    s.reshape(-1)[:4] = np.nan, 0.0, np.inf, -1.0
    anc = (rng.normal(0, 5, shape) + 1j * rng.normal(0, 5, shape)).astype(np.complex64 if dt == np.float32 else np.complex128)
    dsig = {"absent": None, "scalar": SCALAR, "raster": rng.uniform(0.1, 0.3, shape).astype(dt)}[dsig_kind]
    cc, ccr = (rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32) for _ in range(2))
    return inc, s, anc, dsig, cc, ccr


def parent_inputs(shape, db_on_device, inc, s, dsig, anc):
    """(kernel dtype, is_db, dsig_cr_scalar, {name: bytes or None}) of the rasters the three numpy functions formed at 0a2d5eb."""
    reals = [a for a in (inc, s, dsig) if a is not None and not np.isscalar(a)]
    f32 = all(a.dtype == np.float32 for a in reals) and anc.dtype == np.complex64  # _plan.py:33
    dt = np.float32 if f32 else np.float64  # _plan.py:34
    is_db = (s.dtype == np.float32) if db_on_device == "auto" else not db_on_device  # _plan.py:36-42: "auto" keeps a float32 sigma0 on the host
    cast = lambda a, t=dt: np.ascontiguousarray(np.broadcast_to(np.asarray(a), shape), dtype=t)  # :420, :480, :521
    scalar, d = 0.1, None  # _plan.py:43, :422, :523
    with np.errstate(all="ignore"):
        if dsig is not None and np.isscalar(dsig):
            if is_db:
                d = cast(s * 0 + dsig)  # _plan.py:50-51, :424, :525 -> :235: from the LINEAR sigma0, in its own dtype
            else:
                scalar = float(np.float32(dsig)) if f32 else float(dsig)  # _plan.py:53-55
        elif dsig is not None:
            d = cast(dsig)  # :426, :527
        s_db = cast(10 * np.log10(s + 1e-15) if is_db else s)  # :427, :482, :528 -> :132: dB in sigma0's own dtype, then the cast
    return dt, is_db, scalar, dict(inc=cast(inc).tobytes(), sigma0=s_db.tobytes(), dsig_cr=None if d is None else d.tobytes())


def code_bytes(c):
    return np.ascontiguousarray(c, dtype=np.uint32).tobytes()  # :428, :483, :530


def check_common(rec, shape, dt, is_db):
    assert (rec["lines"], rec["samples"]) == shape  # _plan.py:30
    assert (rec["dtype"], rec["mem"]) == (_lib.XSW_F32 if dt == np.float32 else _lib.XSW_F64, _lib.MEM_HOST)  # _plan.py:34, :434, :489, :536
    assert type(rec["is_db"]) is bool and rec["is_db"] == is_db  # :436, :491, :538


def check_cost_outputs(rec, outs, parts, shape, out_dtype):
    assert rec["out_dtype"] == (_lib.XSW_F32 if out_dtype == np.float32 else _lib.XSW_F64)  # :472
    assert [o is None for o in outs] == [False] + [not parts] * 3  # :468
    assert all(o is None or (o.shape == shape and o.dtype == out_dtype) for o in outs)  # :484, :531
    assert rec["outputs"] == tuple(None if o is None else o.ctypes.data for o in outs)  # :490, :538


@pytest.mark.parametrize("db_on_device", DB)
@pytest.mark.parametrize("dsig_kind", DSIG)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cross_pol_calls_hand_the_parents_rasters_to_the_library(recorder, shape, dt, dsig_kind, db_on_device):
    options.db_on_device = db_on_device
    inc, s, anc, dsig, cc, ccr = scene(shape, dt, dsig_kind)
    kdt, is_db, scalar, want = parent_inputs(shape, db_on_device, inc, s, dsig, anc)
    assert kdt == dt
    meta = lambda a: a if (a is None or np.isscalar(a)) else _plan.meta(a)
    luts = (object(), object())
    for select in (False, True):
        plan = _engine.cross_plan(shape, meta(inc), meta(s), meta(anc), meta(s), meta(dsig), device=False, dual_select=select)
        del recorder[:]
        out = _engine.cross_from_codes(*luts, plan, cc, inc, s, dsig, dual_select=select, codes=True)
        assert recorder[0] == dict(call="ensure_luts", luts=luts) and len(recorder) == 2  # :433
        rec = recorder[1]
        check_common(rec, shape, dt, is_db)
        assert rec["call"] == "cross" and rec["out_dtype"] == _lib.XSW_F64  # :434
        assert rec["bytes"] == dict(want, code_co=code_bytes(cc))  # :434-435 (None: no pointer)
        assert out.shape == shape and out.dtype == np.uint32 and rec["outputs"] == (out.ctypes.data, None)  # :429, :435
        assert (rec["dsig_cr_scalar"], rec["dual_select"]) == (scalar, select)  # :436
    plan = _engine.cross_plan(shape, meta(inc), meta(s), meta(anc), meta(s), meta(dsig), device=False)
    for parts, out_dtype in ((True, np.float64), (False, np.float32)):
        del recorder[:]
        outs = _engine.cost_cr_from_codes(*luts, plan, cc, ccr, inc, s, dsig, parts=parts, out_dtype=out_dtype)
        assert recorder[0] == dict(call="ensure_luts", luts=luts) and len(recorder) == 2  # :535
        rec = recorder[1]
        check_common(rec, shape, dt, is_db)
        assert rec["call"] == "cost_cr" and rec["bytes"] == dict(want, code_co=code_bytes(cc), code_cr=code_bytes(ccr))  # :536-537
        check_cost_outputs(rec, outs, parts, shape, out_dtype)
        assert rec["dsig_cr_scalar"] == scalar  # :538


@pytest.mark.parametrize("db_on_device", DB)
@pytest.mark.parametrize("parts", [True, False])
@pytest.mark.parametrize("dt,inc_dt", [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)])
@pytest.mark.parametrize("shape", SHAPES)
def test_co_pol_cost_hands_the_parents_rasters_to_the_library(recorder, shape, dt, inc_dt, parts, db_on_device):
    """(float32 sigma0 next to a float64 incidence: float64 kernel rasters, the dB still taken in float32 before the widening)"""
    options.db_on_device = db_on_device
    inc, s, anc, _, cc, _ = scene(shape, dt, "absent")
    inc = inc.astype(inc_dt)
    dt, is_db, _, want = parent_inputs(shape, db_on_device, inc, s, None, anc)
    assert dt == inc_dt
    plan = _plan.CallPlan(_plan.meta(inc), _plan.meta(s), None, None, _plan.meta(anc), device=False)  # crosspol.py:150
    lut = object()
    for out_dtype in (np.float64, np.float32):
        del recorder[:]
        outs = _engine.cost_from_codes(lut, plan, cc, inc, s, anc, dsig_co=SCALAR, parts=parts, out_dtype=out_dtype)
        assert recorder[0] == dict(call="ensure_luts", luts=(lut, None)) and len(recorder) == 2  # :488
        rec = recorder[1]
        check_common(rec, shape, dt, is_db)
        full_anc = np.ascontiguousarray(np.broadcast_to(anc, shape), dtype=np.complex64 if dt == np.float32 else np.complex128)  # :483
        assert rec["call"] == "cost" and rec["bytes"] == dict(inc=want["inc"], sigma0=want["sigma0"], code_co=code_bytes(cc), anc=full_anc.tobytes())
        check_cost_outputs(rec, outs, parts, shape, out_dtype)
        assert rec["dsig_co"] == SCALAR  # :491


def test_an_empty_raster_makes_no_call(recorder):
    inc, s, anc = np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), np.zeros((0, 5), np.complex64)
    plan = _plan.CallPlan(_plan.meta(inc), _plan.meta(s), None, None, _plan.meta(anc), device=False)
    outs = _engine.cost_from_codes(None, plan, np.zeros((0, 5), np.uint32), inc, s, anc)
    assert recorder == [] and outs[0].shape == (0, 5)  # :486
