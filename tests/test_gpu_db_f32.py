"""GPU: sigma0 -> dB of float32 rasters (xsw_device.hpp: to_db(float), log10_fast) on EVERY float32 argument, against the exact
reference of tests/db_f32_ref.py; and every kernel that inlines to_db at the hard arguments.

How the value is read.  xsw_cost_from_codes stores lut_db - sigma0_db (xsw_cost.hpp: cost_co_at).  On a co-pol table whose
entries are all +0.0, with every code the grid code 0, every incidence on the table's axis and only the residual requested, the
float32 residual of a float32 raster with sigma0_is_db = 0 is -to_db(x) exactly: the dB value is float32-valued, so neither the
subtraction from +0.0 nor the float32 store rounds (+0.0 and -0.0 compare equal).

The sweep.  The bit patterns 0x00000000 .. 0x7FFFFFFF (zero, denormals, every positive value, +inf, the NaNs) and 0x80000000 ..
0xA7FFFFFF (-0.0 down past -1e-15f = 0xA6901D7D: x + 1e-15f runs through tiny positive values, zero and negative values), built on
the device from torch.arange in pieces of 2**26 patterns (8192 x 8192), one test each; one more piece of 2**26 random patterns of
0xA8000000 .. 0xFFFFFFFF, all NaN.  A piece is settled on the device: torch forms y = fl32(x + 1e-15f), L = log10(float64(y)) and
10f * fl32(L); a pixel whose L lies further than 1e-13 |L| from both float32 rounding boundaries around it (db_f32_ref.decided),
and whose kernel value equals that prediction, is settled.  The device library's float64 log10 is only this filter: a settled
pixel needs it right to 1e-13, a pixel it gets wrong is not settled.  Every pixel that is not settled goes to the host with its
kernel value and is judged against the exact logarithm (db_f32_ref.judge): equal to E(x), or a legitimate double rounding -- the
value of the other float32 neighbour, the logarithm within 2e-15 |L| of the boundary -- or the test fails.  About 25 arguments
per binade are not settled; a piece that sends more than 2**16 to the host fails (the filter is then wrong).

Each piece prints its count of host pixels, its double roundings with their patterns, and the largest distance among them."""
import numpy as np
import pytest

import db_f32_ref as ref
import lut_table_shapes as ls
from test_gpu_cost_codes import _cost, _differ, _fill
from test_gpu_forward import default_tables  # noqa: F401 (fixture)
from test_gpu_crosspol_codes import _cross, _fused, _scene
from test_gpu_joint import _joint
from test_gpu_lut_tables import CR
from test_gpu_streams import torch  # noqa: F401 (fixture)
from test_gpu_uncertainty import _unc
from test_gpu_uncertainty_joint import _uj
from util import lut_dicts

pytestmark = pytest.mark.gpu

SIDE = 8192
PIECE = SIDE * SIDE  # 2**26
GUARD = 64
SENTINEL = -7.5e37  # no dB value: |10 log10| <= 451
ZERO_SHAPE = ls.SHAPES["one_block"]  # (3, 9, 5): the smallest table of tests/lut_table_shapes.py
PIECES = [("0x%08X" % p, p) for p in list(range(0, 1 << 31, PIECE)) + list(range(1 << 31, 0xA8000000, PIECE))] + [("random_negative", None)]


def _install_zero_table(ctx):
    inc, wspd, phi = ls.axes("one_block")
    ctx.upload_luts(co=dict(db=np.zeros(ZERO_SHAPE), inc=inc, wspd=wspd, phi=phi), cr=CR)
    return float(inc[0])


@pytest.fixture(scope="module")
def zero_ctx(torch):
    """A context of this module's own with the all-zero co-pol table, and the rasters every piece shares: the incidence (on the
    axis), the codes (grid code 0) and the ancillary wind (not read: only the residual is requested)."""
    from xsarsea_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X box")
    ctx = _lib.Context(0)
    inc0 = _install_zero_table(ctx)
    assert np.array_equal(ctx.read_lut(ZERO_SHAPE), np.zeros(ZERO_SHAPE)) and not np.signbit(ctx.read_lut(ZERO_SHAPE)).any()
    dev = torch.device("cuda", 0)
    shared = dict(inc=torch.full((PIECE,), inc0, dtype=torch.float32, device=dev), code=torch.zeros(PIECE, dtype=torch.int32, device=dev),
                  anc=torch.zeros(PIECE, dtype=torch.complex64, device=dev))
    yield ctx, shared
    shared.clear()
    ctx.close()
    torch.cuda.empty_cache()


def _kernel_db(ctx, torch, _lib, shared, x):
    """to_db(x, 0) of a flat float32 device tensor, as a float32 device tensor: minus the residual on the zero table."""
    n = x.numel()
    out = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    lines, samples = (SIDE, n // SIDE) if n % SIDE == 0 else (1, n)
    ctx.cost_from_codes_raw(lines, samples, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE, shared["inc"].data_ptr(), shared["code"].data_ptr(),
                            x.data_ptr(), shared["anc"].data_ptr(), None, None, None, out.data_ptr() + GUARD * 4, sigma0_is_db=False)
    ctx.synchronize()
    assert bool((out[:GUARD] == SENTINEL).all()) and bool((out[-GUARD:] == SENTINEL).all()), "a guard region was written"
    res = out[GUARD:n + GUARD]
    assert not bool((res == SENTINEL).any()), "a pixel was not written"
    return -res


def _not_settled(torch, x, got):
    """Indices of the pixels the device filter does not settle (module docstring)."""
    dev = x.device
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    y = x + torch.tensor(1e-15, dtype=torch.float32, device=dev)
    L = torch.log10(y.double())
    c = L.float()
    pred = c * torch.tensor(10.0, dtype=torch.float32, device=dev)
    ok = ref.decided(L, c.double(), torch.nextafter(c, inf).double(), torch.nextafter(c, -inf).double(), xp=torch)
    settled = ok & ((got == pred) | (torch.isnan(got) & torch.isnan(pred)))
    return torch.nonzero(~settled).flatten()


@pytest.mark.parametrize("first", [p for _, p in PIECES], ids=[k for k, _ in PIECES])
def test_every_float32_argument(zero_ctx, torch, first):
    from xsarsea_amd import _lib
    ctx, shared = zero_ctx
    dev = torch.device("cuda", 0)
    if first is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(26)
        bits = torch.randint(0xA8000000 - (1 << 32), 0, (PIECE,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
        what = "2**26 random patterns of 0xA8000000 .. 0xFFFFFFFF"
    else:
        start = first - (1 << 32) if first >= (1 << 31) else first  # the int32 that holds the pattern
        bits = torch.arange(start, start + PIECE, dtype=torch.int64, device=dev).to(torch.int32)
        what = f"0x{first:08X} .. 0x{first + PIECE - 1:08X}"
    x = bits.view(torch.float32)
    got = _kernel_db(ctx, torch, _lib, shared, x)
    idx = _not_settled(torch, x, got)
    n_host = int(idx.numel())
    assert n_host <= ref.HOST_MAX, f"{what}: {n_host} pixels not settled on the device: the filter is wrong"
    patterns = bits[idx].cpu().numpy().view(np.uint32)
    values = got[idx].cpu().numpy()
    if first is None:
        assert bool(torch.isnan(got).all()), "a negative argument below -1e-15f is not NaN"
    del x, got, bits, idx
    torch.cuda.empty_cache()
    rep = ref.adjudicate(patterns, values)
    print("\n" + ref.summary(what, rep))
    assert not rep.wrong, f"{what}: {len(rep.wrong)} wrong, first: " + "; ".join(rep.wrong[:5])


def test_the_sweep_sees_a_wrong_value(zero_ctx, torch):
    """The device filter on a piece of one binade with three kernel values nudged by one float32: exactly those reach the host
    beside the undecided ones, and are judged wrong."""
    from xsarsea_amd import _lib
    ctx, shared = zero_ctx
    dev = torch.device("cuda", 0)
    bits = torch.arange(ref.BINADE_2M7, ref.BINADE_2M7 + (1 << 23), dtype=torch.int64, device=dev).to(torch.int32)
    x = bits.view(torch.float32)
    got = _kernel_db(ctx, torch, _lib, shared, x)
    clean = _not_settled(torch, x, got)
    assert set(clean.cpu().numpy().tolist()) >= set((ref.near_boundary(ref.BINADE_2M7) - ref.BINADE_2M7).tolist()), "the device filter settles an argument numpy's does not"
    assert clean.numel() <= 100
    where = [7, 4_000_000, 8_000_000]
    got[where] = torch.nextafter(got[where], torch.zeros(3, dtype=torch.float32, device=dev))
    idx = _not_settled(torch, x, got)
    assert set(where) <= set(idx.cpu().numpy().tolist()) and idx.numel() <= clean.numel() + 3
    rep = ref.adjudicate(bits[idx].cpu().numpy().view(np.uint32), got[idx].cpu().numpy())
    assert len(rep.wrong) == 3


# ------------------------------------------------------------------------------------------------ every consumer kernel
SHAPE = (64, 333)


@pytest.fixture(scope="module")
def hard_scene(zero_ctx, torch):
    """The 64 x 333 float32 scene of tests/test_gpu_crosspol_codes.py with every third co-pol and cross-pol sigma0 a hard argument
    (db_f32_ref.hard_arguments, cycled; the two rasters start at different ones), and the dB rasters the kernels form from them:
    part 1's call on the zero table.  dsig_cr: the raster, and the scalar broadcast formed from the LINEAR cross-pol raster."""
    from xsarsea_amd import _lib
    ctx, shared = zero_ctx
    inc, s_vv, s_vh, dsig, anc = _scene(SHAPE, np.float32)
    hard = ref.hard_arguments()
    n = inc.size
    k = np.arange(0, n, 3)
    s_vv.reshape(-1)[k] = hard[np.arange(k.size) % hard.size]
    s_vh.reshape(-1)[k + 1] = hard[(np.arange(k.size) + 101) % hard.size]
    dev = torch.device("cuda", 0)
    db = []
    for s in (s_vv, s_vh):
        t = torch.from_numpy(np.ascontiguousarray(s).reshape(-1)).to(dev)
        d = _kernel_db(ctx, torch, _lib, {k_: v[:n] for k_, v in shared.items()}, t).cpu().numpy().reshape(SHAPE)
        rep = ref.check(s, d, "hard scene")
        assert not rep.wrong, rep.wrong[:5]
        db.append(d)
    return dict(inc=inc, anc=anc, lin=(s_vv, s_vh), db=tuple(db), dsig=dsig, fill=_fill(s_vh, 0.1))


@pytest.fixture
def default_ctx(gpu_ctx, default_luts):
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    return gpu_ctx


def _same_lists(a, b):
    return {k: _differ(x, y) for k, (x, y) in enumerate(zip(a, b)) if x is not None}


def _both(call):
    """call(s_co, s_cr, is_db) on the linear rasters and on the kernels' dB rasters."""
    return lambda sc: (call(*sc["lin"], False), call(*sc["db"], True))


def test_hard_scene_holds_the_classes(hard_scene):
    for lin, db in zip(hard_scene["lin"], hard_scene["db"]):
        assert np.isneginf(db).any() and np.isposinf(db).any() and np.isnan(db[~np.isnan(lin)]).any() and (db == 0).any()
        assert np.isin(ref.as_bits(ref.hard_arguments()), ref.as_bits(lin)).all(), "a hard argument is not in the scene"


@pytest.mark.parametrize("algo", ["auto", "exact", "exhaustive"])
def test_invert_linear_equals_db(default_ctx, torch, hard_scene, algo):
    """xsw_invert with codes and winds: dual-pol on the default route and with XSW_ALGO_EXACT; XSW_ALGO_EXHAUSTIVE on the co-pol
    raster alone (it takes no cross-pol raster)."""
    from xsarsea_amd import _lib
    from test_gpu_codes import _device_run
    sc = hard_scene
    code = {"auto": _lib.ALGO_AUTO, "exact": _lib.ALGO_EXACT, "exhaustive": _lib.ALGO_EXHAUSTIVE}[algo]
    dual = algo != "exhaustive"
    for name, dsig in (("raster", sc["dsig"]), ("scalar broadcast", sc["fill"])) if dual else (("absent", None),):
        for sel in (False, True) if dual else (False,):
            a, b = (_device_run(default_ctx, torch, _lib, (sc["inc"], s[0], s[1] if dual else None, dsig, sc["anc"]), np.complex64,
                                {"complex", "codes"}, dual_select=sel, is_db=is_db, algo=code) for s, is_db in ((sc["lin"], False), (sc["db"], True)))
            a, b = ({k: v for k, v in o.items() if v is not None} for o in (a, b))
            diff = {k: int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()) if k in ("cc", "ccr") else
                    int((torch.view_as_real(a[k]).view(torch.int32) != torch.view_as_real(b[k]).view(torch.int32)).sum()) for k in a}
            print(f"{algo}, dsig_cr {name}, select {sel}: words that differ between linear and dB rasters {diff}")
            assert not any(diff.values()), (algo, name, sel, diff)
            assert int((a["cc"].view(torch.int32) >= 0).sum()) > 5000, "hardly any pixel was searched"


def test_from_codes_entries_linear_equal_db(default_ctx, torch, hard_scene):
    """Cost co and cr, uncertainty co and cr, joint, uncertainty-joint and cross-pol from codes: the same bits from the linear
    rasters with sigma0_is_db = 0 and from the kernels' dB rasters with sigma0_is_db = 1."""
    from xsarsea_amd import _lib
    sc = hard_scene
    ctx, inc, anc = default_ctx, sc["inc"], sc["anc"]
    f = _fused(ctx, torch, _lib, (inc, sc["db"][0], sc["db"][1], sc["dsig"], anc), np.complex64, False, is_db=True)
    cc, ccr = f["cc"], f["ccr"]
    assert (cc < 0x80000000).sum() > 5000 and (ccr < _lib.CODE_NO_INDEX).sum() > 5000
    failures = {}

    def hold(what, a, b):
        d = _same_lists(a, b)
        print(f"{what}: pixels that differ between linear and dB rasters {d}")
        if any(d.values()):
            failures[what] = d

    for out_t in (np.float32, np.float64):
        o = np.dtype(out_t).name
        hold(f"cost co -> {o}", *_both(lambda s_co, s_cr, db: _cost(ctx, torch, _lib, "co", (inc, cc, s_co, anc), out_t, db))(sc))
        hold(f"uncertainty co -> {o}", *_both(lambda s_co, s_cr, db: _unc(ctx, torch, _lib, "co", (inc, cc, s_co, anc), out_t, db))(sc))
        for name, dsig in (("raster", sc["dsig"]), ("scalar broadcast", sc["fill"])):
            hold(f"cost cr, dsig_cr {name} -> {o}", *_both(lambda s_co, s_cr, db: _cost(ctx, torch, _lib, "cr", (inc, cc, ccr, s_cr, dsig), out_t, db))(sc))
            hold(f"uncertainty cr, dsig_cr {name} -> {o}", *_both(lambda s_co, s_cr, db: _unc(ctx, torch, _lib, "cr", (inc, cc, ccr, s_cr, dsig), out_t, db))(sc))
            hold(f"joint, dsig_cr {name} -> {o}", *_both(lambda s_co, s_cr, db: _joint(ctx, torch, _lib, (inc, cc, s_co, anc, s_cr, dsig), out_t, is_db=db))(sc))
            jc = _joint(ctx, torch, _lib, (inc, cc, sc["db"][0], anc, sc["db"][1], dsig), out_t, want=(1, 0, 0, 0, 0), is_db=True)[0]
            hold(f"uncertainty-joint, dsig_cr {name} -> {o}", *_both(lambda s_co, s_cr, db: _uj(ctx, torch, _lib, (inc, jc, s_co, anc, s_cr, dsig), out_t, is_db=db))(sc))
    for out_c in (np.complex64, np.complex128):
        for name, dsig in (("raster", sc["dsig"]), ("scalar broadcast", sc["fill"])):
            for sel in (False, True):
                a, b = _both(lambda s_co, s_cr, db: _cross(ctx, torch, _lib, inc, cc, s_cr, dsig, out_c, sel, db))(sc)
                hold(f"cross-pol from codes, dsig_cr {name}, select {sel} -> {np.dtype(out_c).name}",
                     [a[0], a[1].real, a[1].imag], [b[0], b[1].real, b[1].imag])
    assert not failures, failures


def test_solves_on_the_kernels_db_rasters(default_tables, torch, hard_scene):
    """The speed solves (co-pol, cross-pol) and the direction solve take sigma0 in dB only -- they have no sigma0_is_db and inline no
    to_db -- so they are run on the dB rasters the kernels form from the hard scene (-inf, +inf, NaN, -150 dB, the dB values of every
    binade edge) and held to their restatements bit for bit; direction and speed are those of the scene's a-priori wind."""
    from xsarsea_amd import _lib
    import test_gpu_dirsolve as tdir
    import test_gpu_solve as tsol
    sc = hard_scene
    t = tsol.Tables(default_tables)
    inc, (db_co, db_cr) = sc["inc"], sc["db"]
    with np.errstate(all="ignore"):
        phi = np.degrees(np.angle(sc["anc"])).astype(np.float32)
        wspd = np.abs(sc["anc"]).astype(np.float32)
    for out_t in (np.float32, np.float64):
        want = t.ref_co(inc, db_co, phi)
        assert (want["flag"] == 0).mean() > 0.1 and (want["flag"] == tsol.sref.BELOW).any() and (want["flag"] == tsol.sref.ABOVE).any()
        tsol._assert_fields(tsol._solve(t.ctx, torch, _lib, "co", (inc, db_co, phi), out_t), want, out_t, "speed solve, co-pol")
        tsol._assert_fields(tsol._solve(t.ctx, torch, _lib, "cr", (inc, db_cr), out_t), t.ref_cr(inc, db_cr), out_t, "speed solve, cross-pol")
        tdir._assert_fields(tdir._dir(t.ctx, torch, _lib, (inc, db_co, wspd), out_t, near=phi), tdir._ref(default_tables, inc, db_co, wspd, phi), out_t,
                            "direction solve")
