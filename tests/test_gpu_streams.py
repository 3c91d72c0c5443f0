"""GPU: device-memory calls are ordered on the caller's stream (include/xsw.h, xsarsea_amd/_device.py).

Every case here uses a HELD-BACK PRODUCER: the real inputs are copied into their buffers on the producing stream behind a
`torch.cuda._sleep` of ~100 ms, and until then the buffers hold a different valid raster (another seed), so a read that overtakes
the producer gives finite but wrong results.  Outputs start as NaN and are read on the consuming stream (non_blocking copies into
page-locked memory) before anything synchronises.  Correct code passes whatever the delay is; the delay only makes a missing wait
visible.  So that no case passes vacuously, each asynchronous call is followed by an assertion that the producer was still in
flight when the call returned, and each call that blocks by design (detrend's ratio upload, LUT installs, MEM_DEVICE_SIGMA0_HOST)
by one that the producer had completed."""
import hashlib
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from test_gpu_kernel import assert_dual_select, synthetic_scene
from util import bits_equal, lut_dicts

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The reference's co-pol precondition (a valid ancillary wind somewhere) is answered on the host, which synchronises the caller's
# stream; the asynchronous cases hand the answer in as multi_gpu.invert_from_model_tiled does (`_xsw_tile`), so that the launch
# itself is what races the producer.
ASYNC = dict(_xsw_tile=True)


@pytest.fixture(scope="session")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="session")
def delay_cycles(torch):
    """`torch.cuda._sleep` cycles for ~100 ms on this device, timed once with HIP events (the rate is not hard-coded)."""
    probe = 1 << 22
    torch.cuda._sleep(probe)  # the first launch loads the kernel
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(probe)
    t1.record()
    t1.synchronize()
    ms = max(t0.elapsed_time(t1), 1e-3)
    return int(min(max(probe * 100.0 / ms, 1 << 20), 1 << 36))


@pytest.fixture
def fresh_ctx():
    """A context of its own: its buffers start empty, so that "larger" really grows them."""
    from xsarsea_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def _dev(torch):
    return torch.device("cuda", 0)


def _staged(torch, real, decoy):
    """[(buffer holding `decoy`, source holding `real`)] on the device, everything landed."""
    out = []
    for r, d in zip(real, decoy):
        if r is None:
            out.append((None, None))
            continue
        out.append((torch.from_numpy(np.ascontiguousarray(d)).to(_dev(torch)), torch.from_numpy(np.ascontiguousarray(r)).to(_dev(torch))))
    torch.cuda.synchronize()
    return out


def _held_back(torch, stream, cycles, pairs):
    """On `stream`: the delay, then buffer <- source for every pair.  Returns an event recorded right after the copies."""
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        for buf, src in pairs:
            if buf is not None:
                buf.copy_(src)
        done.record(stream)
    return done


def _read_back(torch, stream, *tensors):
    """The consumer: non_blocking copies into page-locked host memory on `stream`, then (only then) a device synchronisation."""
    hosts = []
    with torch.cuda.stream(stream):
        for t in tensors:
            h = None
            if t is not None:
                h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                h.copy_(t, non_blocking=True)
            hosts.append(h)
    torch.cuda.synchronize()
    return [None if h is None else h.numpy().copy() for h in hosts]


def _nan(torch, shape, dtype):
    fill = complex(float("nan"), float("nan")) if dtype.is_complex else float("nan")
    return torch.full(shape, fill, dtype=dtype, device=_dev(torch))


def _in_flight(done):
    assert not done.query(), "the producer had already finished: the case did not test the ordering (delay too short?)"


def _completed(done):
    assert done.query(), "a blocking entry point returned before the producer it reads had finished"


def _gmf_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(18, 47, n), rng.uniform(0.5, 35, n), rng.uniform(-180, 180, n)


# ------------------------------------------------------------------------------------------------ forward GMF, first call
@pytest.mark.parametrize("where", ["null_stream", "user_stream", "bench_pattern"])
def test_forward_gmf_first_call_after_context_creation(torch, gpu_ctx, delay_cycles, where):
    """gmf_eval_raw(MEM_DEVICE) as the FIRST call of a fresh context, inputs held back on the stream the context was handed:
    bit-equal to the MEM_HOST evaluation of the same arrays (same kernel), 8 times.  bench_pattern: set_stream -> call ->
    use_own_stream, then the consumer on the user stream (bench.cmod5n_device)."""
    from xsarsea_amd import _lib
    n = 300_000
    gid = _lib.GMF_IDS["gmf_cmod5n"]
    real, decoy = _gmf_inputs(n, 1), _gmf_inputs(n, 2)
    ref = gpu_ctx.gmf_eval(gid, *real)
    assert np.isfinite(ref).all() and not np.array_equal(ref, gpu_ctx.gmf_eval(gid, *decoy))
    for rep in range(8):
        ctx = _lib.Context(0)
        try:
            pairs = _staged(torch, real, decoy)
            out = _nan(torch, (n,), torch.float64)
            torch.cuda.synchronize()
            s = torch.cuda.default_stream(_dev(torch)) if where == "null_stream" else torch.cuda.Stream(device=_dev(torch))
            done = _held_back(torch, s, delay_cycles, pairs)
            ctx.set_stream(s.cuda_stream)
            try:
                ctx.gmf_eval_raw(gid, n, _lib.MEM_DEVICE, *(b.data_ptr() for b, _ in pairs), out.data_ptr())
            finally:
                if where == "bench_pattern":
                    ctx.use_own_stream()
            _in_flight(done)
            got, = _read_back(torch, s, out)
        finally:
            ctx.close()
        assert bits_equal(got, ref), f"{where}, repetition {rep}: {int(np.sum(got != ref))} values differ from MEM_HOST"


_CHILD = r"""
import hashlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from xsarsea_amd import _lib
n, cycles = int(sys.argv[2]), int(sys.argv[3])
def inputs(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(18, 47, n), rng.uniform(0.5, 35, n), rng.uniform(-180, 180, n)
dev = torch.device("cuda", 0)
ctx = _lib.default_context(0)
bufs = [torch.from_numpy(a).to(dev) for a in inputs(2)]
srcs = [torch.from_numpy(a).to(dev) for a in inputs(1)]
out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
s = torch.cuda.current_stream(dev)
done = torch.cuda.Event()
torch.cuda._sleep(cycles)
for b, a in zip(bufs, srcs):
    b.copy_(a)
done.record(s)
ctx.set_stream(s.cuda_stream)
ctx.gmf_eval_raw(_lib.GMF_IDS["gmf_cmod5n"], n, _lib.MEM_DEVICE, *(b.data_ptr() for b in bufs), out.data_ptr())
ctx.use_own_stream()
in_flight = not done.query()
h = torch.empty((n,), dtype=torch.float64, pin_memory=True)
h.copy_(out, non_blocking=True)
torch.cuda.synchronize()
print("IN_FLIGHT", int(in_flight))
print("SHA", hashlib.sha256(h.numpy().tobytes()).hexdigest())
"""


def test_forward_gmf_in_fresh_processes(torch, gpu_ctx, delay_cycles):
    """Four fresh processes at once (the start-up of an N-rank bench job): each creates the default context and evaluates held-back
    inputs on torch's current stream; every output hash equals that of the MEM_HOST evaluation here."""
    from xsarsea_amd import _lib
    n = 300_000
    ref = gpu_ctx.gmf_eval(_lib.GMF_IDS["gmf_cmod5n"], *_gmf_inputs(n, 1))
    want = hashlib.sha256(np.ascontiguousarray(ref).tobytes()).hexdigest()
    procs = [subprocess.Popen([sys.executable, "-c", _CHILD, REPO, str(n), str(delay_cycles)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, cwd=REPO) for _ in range(4)]
    results = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=240)
            results.append((p.returncode, out, err))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for rc, out, err in results:
        assert rc == 0, err[-2000:]
        lines = dict(line.split(" ", 1) for line in out.splitlines() if line.startswith(("SHA ", "IN_FLIGHT ")))
        assert lines["IN_FLIGHT"] == "1", "the child's producer had finished before the call returned"
        assert lines["SHA"] == want


# ------------------------------------------------------------------------------------------------ hand-over of context-owned buffers
def _two_streams(torch):
    return torch.cuda.Stream(device=_dev(torch)), torch.cuda.Stream(device=_dev(torch))


@pytest.mark.parametrize("size", ["same", "larger"])
def test_handover_detrend_ratio_row(torch, fresh_ctx, delay_cycles, size):
    """Call 1 on stream A behind the delay, call 2 at once on stream B with another ratio row (the context-owned row is reused,
    or grown): both == numpy's IEEE quotient.  detrend blocks the host on the ratio upload, so call 1 returns after its producer
    and only its kernel (a large raster) can still be reading the row when call 2 uploads its own."""
    from xsarsea_amd import _lib
    rng = np.random.default_rng(11)
    l1, s1 = 4096, 8192
    l2, s2 = (l1, s1) if size == "same" else (64, s1 + 1000)
    sig1, sig1_decoy = rng.gamma(2.0, 0.01, (l1, s1)), rng.gamma(2.0, 0.01, (l1, s1))
    sig2 = rng.gamma(2.0, 0.01, (l2, s2))
    r1, r2 = 10 ** rng.uniform(-1, 1, s1), 10 ** rng.uniform(-1, 1, s2)
    with np.errstate(all="ignore"):
        ref1, ref2 = sig1 / r1[None, :], sig2 / r2[None, :]
    pairs = _staged(torch, [sig1], [sig1_decoy])
    t2 = torch.from_numpy(sig2).to(_dev(torch))
    o1, o2 = _nan(torch, (l1, s1), torch.float64), _nan(torch, (l2, s2), torch.float64)
    torch.cuda.synchronize()
    a, b = _two_streams(torch)
    try:
        done = _held_back(torch, a, delay_cycles, pairs)
        fresh_ctx.set_stream(a.cuda_stream)
        fresh_ctx.detrend_raw(l1, s1, _lib.XSW_F64, _lib.XSW_F64, _lib.MEM_DEVICE, pairs[0][0].data_ptr(), r1, o1.data_ptr())
        _completed(done)
        fresh_ctx.set_stream(b.cuda_stream)
        fresh_ctx.detrend_raw(l2, s2, _lib.XSW_F64, _lib.XSW_F64, _lib.MEM_DEVICE, t2.data_ptr(), r2, o2.data_ptr())
    finally:
        fresh_ctx.use_own_stream()
    g1, = _read_back(torch, a, o1)
    g2, = _read_back(torch, b, o2)
    assert np.array_equal(g1.view(np.int64), ref1.view(np.int64)), "call 1 (stream A)"
    assert np.array_equal(g2.view(np.int64), ref2.view(np.int64)), "call 2 (stream B)"


@pytest.mark.parametrize("size", ["same", "larger"])
def test_handover_nesz_scratch(torch, gpu_ctx, fresh_ctx, delay_cycles, size):
    """nesz_flatten: call 1 on A behind the delay, call 2 at once on B (the context-owned scratch reused, or grown); both equal
    the host route of the same entry point bit for bit."""
    from xsarsea_amd import _lib
    shp1 = (300, 400)
    shp2 = shp1 if size == "same" else (700, 900)

    def scene(shape, seed):
        r = np.random.default_rng(seed)
        inc = np.broadcast_to(np.linspace(20, 45, shape[1]), shape).copy()
        return r.gamma(2.0, 0.01, shape), inc + 0.01 * r.standard_normal(shape)

    n1, i1 = scene(shp1, 1)
    n1d, i1d = scene(shp1, 2)
    n2, i2 = scene(shp2, 3)
    ref1, ref2 = gpu_ctx.nesz_flatten_host(n1, i1), gpu_ctx.nesz_flatten_host(n2, i2)
    assert not np.allclose(ref1, gpu_ctx.nesz_flatten_host(n1d, i1d))
    assert bits_equal(fresh_ctx.nesz_flatten_host(n1, i1), ref1)  # sizes the scratch for call 1 (no growth behind the delay)
    pairs = _staged(torch, [n1, i1], [n1d, i1d])
    t2 = [torch.from_numpy(x).to(_dev(torch)) for x in (n2, i2)]
    o1, o2 = _nan(torch, shp1, torch.float64), _nan(torch, shp2, torch.float64)
    torch.cuda.synchronize()
    a, b = _two_streams(torch)
    try:
        done = _held_back(torch, a, delay_cycles, pairs)
        fresh_ctx.set_stream(a.cuda_stream)
        fresh_ctx.nesz_flatten_raw(*shp1, _lib.XSW_F64, _lib.MEM_DEVICE, pairs[0][0].data_ptr(), pairs[1][0].data_ptr(), o1.data_ptr())
        _in_flight(done)
        fresh_ctx.set_stream(b.cuda_stream)
        fresh_ctx.nesz_flatten_raw(*shp2, _lib.XSW_F64, _lib.MEM_DEVICE, t2[0].data_ptr(), t2[1].data_ptr(), o2.data_ptr())
    finally:
        fresh_ctx.use_own_stream()
    g1, = _read_back(torch, a, o1)
    g2, = _read_back(torch, b, o2)
    assert bits_equal(g1, ref1), "call 1 (stream A)"
    assert bits_equal(g2, ref2), "call 2 (stream B)"


_INVERT_CASES = {  # name: (algo, dual, shape of call 1, shape of call 2 when larger)
    "mono_pruned": ("pruned", False, (48, 333), (96, 500)),
    "dual_select": ("pruned", True, (48, 333), (96, 500)),
    "exact": ("exact", False, (16, 150), (24, 200)),
    "exhaustive": ("exhaustive", False, (16, 150), (24, 200)),  # mono co-pol only
}


@pytest.mark.parametrize("size", ["same", "larger"])
@pytest.mark.parametrize("case", list(_INVERT_CASES))
def test_handover_invert_work_list(torch, gpu_ctx, fresh_ctx, lowres_luts, delay_cycles, case, size):
    """invert_raw(MEM_DEVICE): call 1 on A behind the delay, call 2 at once on B with another scene (the context's work lists
    reused, or grown): both equal the host route of the same rasters bit for bit (float32 rasters, complex64 winds)."""
    from xsarsea_amd import _lib
    algo, dual, shp1, big = _INVERT_CASES[case]
    shp2 = shp1 if size == "same" else big
    co, cr = lut_dicts(*lowres_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    fresh_ctx.upload_luts(co=co, cr=cr)
    sc1, dec1, sc2 = synthetic_scene(*shp1, np.float32, 21), synthetic_scene(*shp1, np.float32, 22), synthetic_scene(*shp2, np.float32, 23)

    def host_ref(sc):
        inc, s_vv, s_vh, dsig, anc = sc
        r = gpu_ctx.invert_host(inc, sigma0_co=s_vv, sigma0_cr=s_vh if dual else None, dsig_cr=dsig if dual else None, anc=anc,
                                algo=algo, dual_select=dual, out_dtype=np.complex64)
        return r[0], (r[1] if dual else None)

    ref1, ref2 = host_ref(sc1), host_ref(sc2)
    assert not bits_equal(ref1[0], host_ref(dec1)[0])
    pick = lambda sc: [sc[0], sc[1], sc[2] if dual else None, sc[3] if dual else None, sc[4]]
    pairs = _staged(torch, pick(sc1), pick(dec1))
    t2 = [None if x is None else torch.from_numpy(x).to(_dev(torch)) for x in pick(sc2)]
    outs1 = [_nan(torch, shp1, torch.complex64), _nan(torch, shp1, torch.complex64) if dual else None]
    outs2 = [_nan(torch, shp2, torch.complex64), _nan(torch, shp2, torch.complex64) if dual else None]
    torch.cuda.synchronize()
    p = lambda t: None if t is None else t.data_ptr()
    run = lambda shp, ins, outs: fresh_ctx.invert_raw(shp[0], shp[1], _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE, *(p(t) for t in ins),
                                                    p(outs[0]), p(outs[1]), algo=_lib.ALGOS[algo], dual_select=dual)
    # sizes the work lists for call 1 (no growth behind the delay), on rasters that have landed
    run(shp1, [src for _, src in pairs], outs1)
    fresh_ctx.synchronize()
    assert bits_equal(outs1[0].cpu().numpy(), ref1[0])
    outs1[0].fill_(complex(float("nan"), float("nan")))
    torch.cuda.synchronize()
    a, b = _two_streams(torch)
    try:
        done = _held_back(torch, a, delay_cycles, pairs)
        fresh_ctx.set_stream(a.cuda_stream)
        run(shp1, [buf for buf, _ in pairs], outs1)
        _in_flight(done)
        fresh_ctx.set_stream(b.cuda_stream)
        run(shp2, t2, outs2)
    finally:
        fresh_ctx.use_own_stream()
    g1 = _read_back(torch, a, *outs1)
    g2 = _read_back(torch, b, *outs2)
    for k in range(2 if dual else 1):
        assert bits_equal(g1[k], ref1[k]), f"call 1 (stream A), output {k}"
        assert bits_equal(g2[k], ref2[k]), f"call 2 (stream B), output {k}"


def test_codes_expanded_on_a_side_stream(torch, gpu_ctx, lowres_luts, delay_cycles):
    """Inversion to grid codes on the launch stream behind the delay; expand_codes_on_stream on a third stream that waits for
    the launch stream by an event (windspeed._engine / multi_gpu gather): == xsw_invert's direct complex output, bit for bit."""
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*lowres_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    shp = (64, 400)
    sc, dec = synthetic_scene(*shp, np.float32, 31), synthetic_scene(*shp, np.float32, 32)
    dev = _dev(torch)
    p = lambda t: None if t is None else t.data_ptr()
    # the reference: the complex winds of one direct call on the same (already landed) rasters
    t_ref = [torch.from_numpy(x).to(dev) for x in sc]
    ref = [torch.empty(shp, dtype=torch.complex128, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    gpu_ctx.invert_raw(*shp, _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE, *(p(t) for t in t_ref), p(ref[0]), p(ref[1]),
                       algo=_lib.ALGO_PRUNED, dual_select=True)
    gpu_ctx.synchronize()
    ref = [r.cpu().numpy() for r in ref]
    pairs = _staged(torch, list(sc), list(dec))
    codes = [torch.full(shp, 0x12345678, dtype=torch.int32, device=dev) for _ in range(2)]
    outs = [_nan(torch, shp, torch.complex128) for _ in range(2)]
    torch.cuda.synchronize()
    launch, side = _two_streams(torch)
    try:
        done = _held_back(torch, launch, delay_cycles, pairs)
        gpu_ctx.set_stream(launch.cuda_stream)
        gpu_ctx.invert_raw(*shp, _lib.XSW_F32, _lib.XSW_F64, _lib.MEM_DEVICE, *(p(buf) for buf, _ in pairs), None, None,
                           algo=_lib.ALGO_PRUNED, dual_select=True, out_code_co=p(codes[0]), out_code_cr=p(codes[1]))
        _in_flight(done)
        landed = torch.cuda.Event()
        landed.record(launch)
        side.wait_event(landed)
        gpu_ctx.expand_codes_on_stream(side.cuda_stream, codes[0].numel(), _lib.XSW_F64, p(codes[0]), p(codes[1]), p(outs[0]), p(outs[1]))
        _in_flight(done)
    finally:
        gpu_ctx.use_own_stream()
    got = _read_back(torch, side, *outs)
    assert bits_equal(got[0], ref[0]) and bits_equal(got[1], ref[1])


# ------------------------------------------------------------------------------------------------ LUT installs while work is queued
@pytest.mark.parametrize("lut_build", ["host", "device"])
def test_lut_switch_while_a_search_is_queued(torch, gpu_ctx, delay_cycles, lut_build):
    """Public API, device tensors, one user stream: call 1 searches the default-resolution CMOD5.N LUT behind the delay, call 2
    (resolution="low") makes ensure_luts reinstall the co-pol table with no synchronisation in between.  Each result equals the
    numpy route with its own LUT, bit for bit (float64 rasters).  lut_build="device": the tables are built by xsw_lut_build."""
    import xsarsea_amd
    from xsarsea_amd import windspeed
    sc, dec = synthetic_scene(40, 300, np.float64, 41), synthetic_scene(40, 300, np.float64, 42)
    inc, s_vv, _, _, anc = sc
    old = xsarsea_amd.options.lut_build
    P = torch.cuda.Stream(device=_dev(torch))
    try:
        xsarsea_amd.options.lut_build = lut_build
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_lo = windspeed.invert_from_model(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
            ref_hi = windspeed.invert_from_model(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n")  # leaves this LUT installed
            assert not bits_equal(ref_lo, ref_hi)
            pairs = _staged(torch, [inc, s_vv, anc], [dec[0], dec[1], dec[4]])
            bufs = [buf for buf, _ in pairs]
            t_lo = [torch.from_numpy(x).to(_dev(torch)) for x in (inc, s_vv, anc)]
            # the device route once on landed rasters: the work lists are sized and the default-resolution LUT is installed
            assert bits_equal(windspeed.invert_from_model(*t_lo[:2], ancillary_wind=t_lo[2], model="gmf_cmod5n").cpu().numpy(), ref_hi)
            torch.cuda.synchronize()
            with torch.cuda.stream(P):
                done = _held_back(torch, P, delay_cycles, pairs)
                hi = windspeed.invert_from_model(bufs[0], bufs[1], ancillary_wind=bufs[2], model="gmf_cmod5n", **ASYNC)
                _in_flight(done)
                lo = windspeed.invert_from_model(t_lo[0], t_lo[1], ancillary_wind=t_lo[2], model="gmf_cmod5n", resolution="low", **ASYNC)
                g_hi, g_lo = _read_back(torch, P, hi, lo)
    finally:
        xsarsea_amd.options.lut_build = old
    assert bits_equal(g_hi, ref_hi), "call 1: default-resolution LUT"
    assert bits_equal(g_lo, ref_lo), "call 2: low-resolution LUT"


def test_lut_install_on_a_busy_user_stream(torch, delay_cycles, default_luts):
    """The context handed a user stream whose producer is still held back: xsw_lut_interp == the host interpolation bit for bit;
    xsw_lut_build == the oracle's table to 1e-10 dB; a noisy LUT (no monotone columns: the mono_rows table decides the route)
    installed there, then pruned == exhaustive.  All of them block: each returns after the producer."""
    from oracle import lut as olut
    from xsarsea_amd import _lib, windspeed
    from xsarsea_amd.windspeed import _engine, get_model
    from xsarsea_amd.windspeed.lut import axis_grid, lerp_axis
    ctx = _lib.Context(0)
    P = torch.cuda.Stream(device=_dev(torch))
    x = np.random.default_rng(1).standard_normal(1 << 20)
    try:
        ctx.set_stream(P.cuda_stream)
        # lut_interp
        m = windspeed.get_model("gmf_cmod5n")
        raw = m._raw_lut()
        inc, wspd, phi = axis_grid(m.inc_range, 0.1), axis_grid(m.wspd_range, 0.1), axis_grid(m.phi_range, 1.0)
        host = lerp_axis(lerp_axis(lerp_axis(raw.values, raw.incidence, inc, 0), raw.wspd, wspd, 1), raw.phi, phi, 2)
        done = _held_back(torch, P, delay_cycles, _staged(torch, [x], [-x]))
        dev = ctx.lut_interp(raw.values, raw.incidence, raw.wspd, raw.phi, inc, wspd, phi)
        _completed(done)
        assert np.array_equal(dev, host)
        # lut_build
        lco = default_luts[0]
        plan = get_model("gmf_cmod5n").device_lut_plan()
        dl = _engine.DeviceLut("gmf_cmod5n", plan[0], plan[1], plan[2], key=None)
        done = _held_back(torch, P, delay_cycles, _staged(torch, [x], [-x]))
        dl.build(ctx)
        _completed(done)
        built = ctx.read_lut(dl.shape)
        assert np.isfinite(built).all() and float(np.max(np.abs(built - lco.values))) <= 1e-10
        # a noisy LUT installed from the host
        rng = np.random.default_rng(9)
        sub = lco.values[::50, ::2, ::2]
        noisy = olut.Lut(sub + 0.2 * rng.standard_normal(sub.shape), lco.incidence[::50], lco.wspd[::2], lco.phi[::2], "dB", "x", "co", "VV")
        done = _held_back(torch, P, delay_cycles, _staged(torch, [x], [-x]))
        ctx.upload_luts(co=lut_dicts(noisy, None)[0])
        _completed(done)
        ctx.use_own_stream()
        inc_s, s_vv, _, _, anc = synthetic_scene(48, 300, np.float64, 43)
        pruned = ctx.invert_host(inc_s, sigma0_co=s_vv, anc=anc, algo="pruned")[0]
        exhaustive = ctx.invert_host(inc_s, sigma0_co=s_vv, anc=anc, algo="exhaustive")[0]
        assert bits_equal(pruned, exhaustive)
    finally:
        torch.cuda.synchronize()
        ctx.close()


# ------------------------------------------------------------------------------------------------ the public entry points on a user stream
def _numpy_route_close(got, ref):
    """Device tensor result vs the numpy route: bit for bit (the narrower dtype of the two when they differ)."""
    if got.dtype != ref.dtype:
        narrow = got.dtype if got.dtype.itemsize < ref.dtype.itemsize else ref.dtype
        got, ref = got.astype(narrow), ref.astype(narrow)
    return bits_equal(got, ref)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["mono", "dual"])
def test_invert_from_model_on_a_user_stream(torch, gpu_ctx, lowres_luts, delay_cycles, mode, dtype):
    """`with torch.cuda.stream(P)`: inputs produced on P behind the delay, invert_from_model, outputs consumed on P; == the numpy
    route of the same rasters (float32: with its sigma0 -> dB on the device too, as the device route does it)."""
    import xsarsea_amd
    from oracle import invert as oinv
    from xsarsea_amd import windspeed
    sc, dec = synthetic_scene(48, 260, dtype, 51), synthetic_scene(48, 260, dtype, 52)
    inc, s_vv, s_vh, dsig, anc = sc
    model = "gmf_cmod5n" if mode == "mono" else ("gmf_cmod5n", "gmf_s1_v2")
    old = xsarsea_amd.options.db_on_device
    P = torch.cuda.Stream(device=_dev(torch))
    try:
        xsarsea_amd.options.db_on_device = dtype == np.float32
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if mode == "mono":
                ref = (windspeed.invert_from_model(inc, s_vv, ancillary_wind=anc, model=model, resolution="low"),)
            else:
                ref = windspeed.invert_from_model(inc, s_vv, s_vh, ancillary_wind=anc, dsig_cr=dsig, model=model, resolution="low")
            pairs = _staged(torch, list(sc), list(dec))

            def call(b):
                if mode == "mono":
                    return (windspeed.invert_from_model(b[0], b[1], ancillary_wind=b[4], model=model, resolution="low", **ASYNC),)
                return windspeed.invert_from_model(b[0], b[1], b[2], ancillary_wind=b[4], dsig_cr=b[3], model=model, resolution="low", **ASYNC)

            call([src for _, src in pairs])  # on landed rasters first: LUTs installed, work lists sized
            torch.cuda.synchronize()
            with torch.cuda.stream(P):
                done = _held_back(torch, P, delay_cycles, pairs)
                res = call([buf for buf, _ in pairs])
                _in_flight(done)
                got = _read_back(torch, P, *res)
    finally:
        xsarsea_amd.options.db_on_device = old
    assert _numpy_route_close(got[0], ref[0]), "co-pol wind"
    if mode == "dual":
        raw = oinv.invert_numpy(oinv.Prepared(*lowres_luts), inc, oinv.to_db(s_vv), oinv.to_db(s_vh), dsig, anc)[1]
        assert_dual_select(got[1], ref[1], raw, "dual wind")


def test_detrend_and_nesz_on_a_user_stream(torch, gpu_ctx, delay_cycles):
    """sigma0_detrend and nesz_flattening under `with torch.cuda.stream(P)`, inputs produced on P behind the delay: == the numpy
    route bit for bit.  nesz is asynchronous; detrend reads the first incidence line on the host (it returns after the producer)."""
    import xsarsea_amd
    from xsarsea_amd.windspeed import nesz_flattening
    rng = np.random.default_rng(6)
    shape = (150, 320)
    inc = np.broadcast_to(np.linspace(20, 45, shape[1]), shape).copy()
    inc_d = np.broadcast_to(np.linspace(25, 40, shape[1]), shape).copy()
    sig, sig_d = rng.gamma(2.0, 0.01, shape), rng.gamma(2.0, 0.01, shape)
    det_ref = xsarsea_amd.sigma0_detrend(sig, inc)
    old = xsarsea_amd.options.nesz_on_device
    try:
        xsarsea_amd.options.nesz_on_device = "device"
        nz_ref = nesz_flattening(sig, inc)
    finally:
        xsarsea_amd.options.nesz_on_device = old
    P = torch.cuda.Stream(device=_dev(torch))
    with torch.cuda.stream(P):
        pairs = _staged(torch, [sig, inc], [sig_d, inc_d])
        done = _held_back(torch, P, delay_cycles, pairs)
        nz = nesz_flattening(pairs[0][0], pairs[1][0])
        _in_flight(done)
        got_nz, = _read_back(torch, P, nz)
        pairs = _staged(torch, [sig, inc], [sig_d, inc_d])
        done = _held_back(torch, P, delay_cycles, pairs)
        det = xsarsea_amd.sigma0_detrend(pairs[0][0], pairs[1][0])
        _completed(done)
        got_det, = _read_back(torch, P, det)
    assert bits_equal(got_nz, nz_ref), "nesz_flattening"
    assert bits_equal(got_det, det_ref), "sigma0_detrend"


def test_sigma0_from_the_host_after_a_held_back_producer(torch, gpu_ctx, lowres_luts, delay_cycles):
    """MEM_DEVICE_SIGMA0_HOST with the device incidence / ancillary wind produced behind the delay on the stream the context was
    set to: == the all-device call on the landed rasters, bit for bit (the call synchronises the context's stream first)."""
    import ctypes
    from xsarsea_amd import _lib
    co, cr = lut_dicts(*lowres_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    shp = (64, 500)
    inc, s_vv, _, _, anc = synthetic_scene(*shp, np.float32, 61)
    dec = synthetic_scene(*shp, np.float32, 62)
    with np.errstate(all="ignore"):
        db_vv = (10 * np.log10(s_vv + 1e-15)).astype(np.float32)
    dev = _dev(torch)
    p = lambda t: None if t is None else t.data_ptr()
    t_inc, t_vv, t_anc = (torch.from_numpy(x).to(dev) for x in (inc, db_vv, anc))
    ref = torch.empty(shp, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.invert_raw(*shp, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE, p(t_inc), p(t_vv), None, None, p(t_anc), p(ref), None,
                       sigma0_is_db=True)
    gpu_ctx.synchronize()
    ref = ref.cpu().numpy()
    flat = s_vv.reshape(-1)

    def stage(which, px0, npx, dst):
        if which != _lib.STAGE_SIGMA0_CO:
            return 0
        o = np.frombuffer((ctypes.c_char * (npx * 4)).from_address(dst), dtype=np.float32)
        with np.errstate(all="ignore"):
            o[...] = 10 * np.log10(flat[px0:px0 + npx] + 1e-15)
        return 1

    pairs = _staged(torch, [inc, anc], [dec[0], dec[4]])
    out = _nan(torch, shp, torch.complex64)
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=dev)
    try:
        done = _held_back(torch, P, delay_cycles, pairs)
        gpu_ctx.set_stream(P.cuda_stream)
        gpu_ctx.invert_raw(*shp, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE_SIGMA0_HOST, p(pairs[0][0]), s_vv.ctypes.data, None, None,
                           p(pairs[1][0]), p(out), None, sigma0_is_db=True, stage=stage)
        _completed(done)
    finally:
        gpu_ctx.use_own_stream()
    got, = _read_back(torch, P, out)
    assert bits_equal(got, ref)


class _CaiV3:
    """Not a torch tensor: a version-3 `__cuda_array_interface__` that names the stream its data is produced on, plus the shape
    attributes every such array has (cupy, numba)."""

    def __init__(self, t, stream):
        self._t = t
        cai = dict(t.__cuda_array_interface__)
        cai.update(version=3, stream=stream.cuda_stream)
        self.__cuda_array_interface__ = cai
        self.shape, self.ndim = tuple(t.shape), t.dim()


def test_cuda_array_interface_v3_stream(torch, gpu_ctx, delay_cycles):
    """Interface objects whose data is produced on P behind the delay, passed while another stream Q is current: the library
    must wait for P (the interface's `stream`), not only for Q.  invert_from_model, nesz_flattening and sigma0_detrend each ==
    the numpy route."""
    import xsarsea_amd
    from xsarsea_amd import windspeed
    from xsarsea_amd.windspeed import nesz_flattening
    sc, dec = synthetic_scene(40, 240, np.float64, 71), synthetic_scene(40, 240, np.float64, 72)
    inc, s_vv, _, _, anc = sc
    rng = np.random.default_rng(7)
    sig, sig_d = rng.gamma(2.0, 0.01, inc.shape), rng.gamma(2.0, 0.01, inc.shape)
    inc_clean = np.broadcast_to(np.linspace(20, 45, inc.shape[1]), inc.shape).copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_co = windspeed.invert_from_model(inc, s_vv, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
    old = xsarsea_amd.options.nesz_on_device
    try:
        xsarsea_amd.options.nesz_on_device = "device"
        ref_nz = nesz_flattening(sig, inc_clean)
    finally:
        xsarsea_amd.options.nesz_on_device = old
    ref_det = xsarsea_amd.sigma0_detrend(sig, inc_clean)
    P, Q = _two_streams(torch)
    # inversion
    pairs = _staged(torch, [inc, s_vv, anc], [dec[0], dec[1], dec[4]])
    wrap = [_CaiV3(buf, P) for buf, _ in pairs]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        landed = [src for _, src in pairs]  # the device route once on landed rasters: LUT installed, work lists sized
        assert bits_equal(windspeed.invert_from_model(landed[0], landed[1], ancillary_wind=landed[2], model="gmf_cmod5n",
                                                      resolution="low").cpu().numpy(), ref_co)
    torch.cuda.synchronize()
    with torch.cuda.stream(Q):
        done = _held_back(torch, P, delay_cycles, pairs)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            co = windspeed.invert_from_model(wrap[0], wrap[1], ancillary_wind=wrap[2], model="gmf_cmod5n", resolution="low", **ASYNC)
        _in_flight(done)
        got_co, = _read_back(torch, Q, co)
    assert bits_equal(got_co, ref_co), "invert_from_model"
    # nesz
    pairs = _staged(torch, [sig, inc_clean], [sig_d, inc_clean[::-1].copy()])
    with torch.cuda.stream(Q):
        done = _held_back(torch, P, delay_cycles, pairs)
        nz = nesz_flattening(_CaiV3(pairs[0][0], P), _CaiV3(pairs[1][0], P))
        _in_flight(done)
        got_nz, = _read_back(torch, Q, nz)
    assert bits_equal(got_nz, ref_nz), "nesz_flattening"
    # detrend (reads the first incidence line on the host: returns after the producer)
    pairs = _staged(torch, [sig, inc_clean], [sig_d, inc_clean[::-1].copy()])
    with torch.cuda.stream(Q):
        done = _held_back(torch, P, delay_cycles, pairs)
        det = xsarsea_amd.sigma0_detrend(_CaiV3(pairs[0][0], P), _CaiV3(pairs[1][0], P))
        _completed(done)
        got_det, = _read_back(torch, Q, det)
    assert bits_equal(got_det, ref_det), "sigma0_detrend"
