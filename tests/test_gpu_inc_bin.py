"""GPU: the incidence bin of every kernel -- `nearest_index` (csrc/xsw_device.hpp) at its thirteen call sites -- on the probes of
tests/inc_bin_cases.py: every node of eight incidence axes, every midpoint between two nodes (exact ties on most axes), one float64
step to either side of both, beyond the ends, +-inf and NaN, as float64 rasters, and the float32 values on a 0.05 degree grid and at
the midpoints as float32 rasters.  The co-pol and the cross-pol table of an install sit on DIFFERENT incidence axes, and every slice
of both names itself: tests/test_inc_bin_cpu.py shows on the CPU that the answer of every kernel below differs, on every probe,
from what either neighbouring slice gives.  So one wrong bin anywhere is one wrong pixel here.

References: the CPU oracle (oracle.cport / oracle.invert) for the inversion -- grid indices equal on every probe, winds through
assert_complex_close at test_random_configurations's tolerances (1e-12 co-pol, 1e-9 cross-pol) -- and for each from-codes kernel
the numpy restatement and the comparison its own GPU test uses: bit for bit.  inc = +-inf answers from slice 0 (every |dim - inc| is
inf and the arg-min of equal values is the first), which is what the oracle and every restatement give without being told.

An MI355X takes 0.01 .. 0.7 s per case (the references of one axis set are built once and shared), 3.2 .. 3.5 s per forced-route
child (LABBOOK section 40 has the counters seen)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import inc_bin_cases as ic
import test_gpu_cost_codes as tcost
import test_gpu_crosspol_codes as tcross
import test_gpu_joint as tjoint
import test_gpu_uncertainty as tunc
import test_gpu_uncertainty_joint as tuj
from conftest import REPO
from test_gpu_route_geometry import LIST_CAP, ROUTES
from test_gpu_streams import torch  # noqa: F401 (fixture)
from util import assert_complex_close, bits_equal, lut_dicts

pytestmark = pytest.mark.gpu

DTYPES = {"f64": np.float64, "f32": np.float32}
_installed = [None]


def install(ctx, name):
    """The LUT pair of set `name` on the session's context: once for all the cases of the set that follow each other."""
    if _installed[0] != name:
        _installed[0] = None
        c = ic.case(name, np.float64)
        co, cr = lut_dicts(c["lco"], c["lcr"])
        ctx.upload_luts(co=co, cr=cr)
        _installed[0] = name
    return ctx


@pytest.fixture(scope="module", params=list(ic.SETS))
def axis_set(request):
    """Module-scoped, so that pytest runs the cases of one set one after the other: one install per set."""
    return request.param


@pytest.fixture(scope="module", autouse=True)
def _own_tables():
    """The session's context comes to this module holding some other module's tables, and leaves it for the next one."""
    _installed[0] = None
    yield
    _installed[0] = None


def want_idx(c, dual):
    idx = c["o_idx"].astype(np.int32)
    if not dual:
        idx[..., 2] = -1  # (the mono call runs no cross-pol search)
    return idx


def check_inversion(c, got, dual, what, co_only=False):
    co, cr, idx = got
    want = want_idx(c, dual)
    cols = slice(0, 2) if co_only else slice(0, 3)
    bad = np.any(idx[..., cols] != want[..., cols], axis=-1)
    print(f"{what}: grid indices differ from the oracle on {int(bad.sum())} of {bad.size} pixels")
    assert not bad.any(), f"{what}: grid indices differ from the oracle on {int(bad.sum())} probes, first at incidence {c['sc']['inc'][bad][:4]!r}"
    assert_complex_close(co, c["o_co"], rtol=1e-12, what=f"{what} co")
    if dual:
        assert_complex_close(cr, c["o_cr"], rtol=1e-9, what=f"{what} cr")


@pytest.mark.parametrize("tag", list(DTYPES))
def test_inversion_indices(gpu_ctx, axis_set, tag):
    """invert_host on host rasters: pruned and exact, mono and dual-pol; both exhaustive kernels (mono co-pol)."""
    c = ic.case(axis_set, DTYPES[tag])
    ctx, sc = install(gpu_ctx, axis_set), c["sc"]
    for algo in ("pruned", "exact"):
        for dual in (False, True):
            got = ctx.invert_host(sc["inc"], sigma0_co=sc["sco"], sigma0_cr=sc["scr"] if dual else None, dsig_cr=sc["dsig"] if dual else None,
                                  anc=sc["anc"], dsig_co=ic.DSIG_CO, sigma0_is_db=True, algo=algo, want_idx=True)
            check_inversion(c, got, dual, f"{axis_set} {tag} {algo} {'dual' if dual else 'mono'}")
    for algo in ("exhaustive", "exhaustive_f64"):
        got = ctx.invert_host(sc["inc"], sigma0_co=sc["sco"], anc=sc["anc"], dsig_co=ic.DSIG_CO, sigma0_is_db=True, algo=algo, want_idx=True)
        check_inversion(c, got, False, f"{axis_set} {tag} {algo}", co_only=True)


def device_inversion(ctx, torch, _lib, sc, dual):
    """invert_raw on device rasters (algo pruned): (co, cr or None, idx) as host arrays."""
    dev = torch.device("cuda", 0)
    inc = sc["inc"]
    t_in = [torch.from_numpy(sc[k]).to(dev) for k in ("inc", "sco", "scr", "dsig", "anc")]
    out_co = torch.full(inc.shape, float("nan"), dtype=torch.complex128, device=dev)
    out_cr = torch.full(inc.shape, float("nan"), dtype=torch.complex128, device=dev) if dual else None
    t_idx = torch.full(inc.shape + (3,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.invert_raw(inc.shape[0], inc.shape[1], _lib.XSW_F32 if inc.dtype == np.float32 else _lib.XSW_F64, _lib.XSW_F64, _lib.MEM_DEVICE,
                   t_in[0].data_ptr(), t_in[1].data_ptr(), t_in[2].data_ptr() if dual else None, t_in[3].data_ptr() if dual else None,
                   t_in[4].data_ptr(), out_co.data_ptr(), out_cr.data_ptr() if dual else None, out_idx=t_idx.data_ptr(), dsig_co=ic.DSIG_CO,
                   sigma0_is_db=True, algo=_lib.ALGO_PRUNED)
    ctx.synchronize()
    return out_co.cpu().numpy(), (out_cr.cpu().numpy() if dual else None), t_idx.cpu().numpy()


@pytest.mark.parametrize("tag", list(DTYPES))
def test_inversion_on_device_rasters(gpu_ctx, torch, axis_set, tag):  # noqa: F811
    from xsarsea_amd import _lib
    c = ic.case(axis_set, DTYPES[tag])
    ctx = install(gpu_ctx, axis_set)
    for dual in (False, True):
        check_inversion(c, device_inversion(ctx, torch, _lib, c["sc"], dual), dual, f"{axis_set} {tag} device rasters {'dual' if dual else 'mono'}")


@pytest.mark.parametrize("tag", list(DTYPES))
def test_band_kernel_chooses_the_cross_pol_slice(gpu_ctx, torch, tag):  # noqa: F811
    """Dual-pol, pruned, device rasters, the `default` axes: k_invert_band itself resolves most probes -- it hands few of them to
    k_invert_band2, k_invert_blocks and k_invert_list (timing(), stats_chain()) -- so the cross-pol slice of those probes is the one its
    own nearest_index call in wave_tail chose (csrc/xsw_band.hpp), not load_pixel's."""
    from xsarsea_amd import _lib
    c = ic.case("default", DTYPES[tag])
    ctx = install(gpu_ctx, "default")
    ctx.timing_enable(True)
    ctx.stats_enable(2)
    try:
        got = device_inversion(ctx, torch, _lib, c["sc"], True)
        tm, ch = ctx.timing(), ctx.stats_chain()
    finally:
        ctx.stats_enable(False)
        ctx.timing_enable(False)
    check_inversion(c, got, True, f"default {tag} device rasters dual, chain statistics")
    live = int(np.sum(c["i_inc"] >= 0))
    left = tm["last_band2_pixels"] + tm["last_list_pixels"] + tm["last_blocks_pixels"]
    print(f"default {tag}: {live} probes, handed on by k_invert_band: band2 {tm['last_band2_pixels']}, list {tm['last_list_pixels']}, "
          f"blocks {tm['last_blocks_pixels']}; candidates scored after it {ch}")
    # a probe that a later kernel answers is on a list and scores at least one candidate there; the one-kernel path (no band kernel
    # at all) writes no list but scores every probe in k_invert_list.  Fewer than half the probes by both counts: k_invert_band ran
    # and answered the others itself.
    assert 0 <= left < 0.5 * live and ch["cand_band2"] + ch["cand_blocks"] + ch["cand_list"] < 0.5 * live, (tm, ch, live)


# ------------------------------------------------------------------------------------------------ forced routes
@pytest.fixture(scope="module")
def route_problem(tmp_path_factory):
    """Tables, rasters and the oracle's answers for the children (no GPU in here).  Each raster gets two more lines -- the midpoint
    probes with sigma0_co = +inf dB: a co-pol problem that is not finite is k_invert_list's whatever the route, so these ties also go
    through that kernel's load_pixel, and list G overflows under XSW_LIST_CAP_TEST=64."""
    c0 = ic.case("default", np.float64)
    lco, lcr = c0["lco"], c0["lcr"]
    d = {"co": lco.values, "inc_co": lco.incidence, "w": lco.wspd, "phi": lco.phi, "cr": lcr.values, "inc_cr": lcr.incidence, "wcr": lcr.wspd}
    for tag, dt in DTYPES.items():
        sc = ic.case("default", dt)["sc"]
        row = 1 if tag == "f32" else ic.CLASSES.index("mid")
        more = {k: np.repeat(v[row:row + 1], 2, axis=0) for k, v in sc.items()}
        more["sco"][...] = np.inf
        more["inc"][1] = np.where(np.isnan(more["inc"][1]), 33.0, more["inc"][1])  # (the second line has no padding)
        sc = {k: np.ascontiguousarray(np.concatenate([v, more[k]])) for k, v in sc.items()}
        o_co, o_cr, o_idx = ic.oracle_answer(lco, lcr, sc)
        assert np.sum(np.isinf(sc["sco"]) & ~np.isnan(sc["inc"])) > 4 * LIST_CAP
        d.update({f"{tag}/{k}": v for k, v in sc.items()})
        d.update({f"{tag}/o_co": o_co, f"{tag}/o_cr": o_cr, f"{tag}/o_idx": o_idx.astype(np.int32)})
    path = tmp_path_factory.mktemp("inc_bin") / "problem.npz"
    np.savez(path, **d)
    return str(path)


_CHILD = r"""
import sys, time
t0 = time.perf_counter()
import numpy as np
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
import torch
from oracle import lut as olut
from util import lut_dicts, assert_complex_close
from xsarsea_amd import _lib
d = np.load({npz!r})
ctx = _lib.Context(0)
dev = torch.device("cuda", 0)

def close(got, ref, rtol):
    try:
        assert_complex_close(got, ref, rtol=rtol)
        return "ok"
    except AssertionError as e:
        return "FAIL:" + str(e).replace(" ", "_")

lco = olut.Lut(d["co"], d["inc_co"], d["w"], d["phi"], "dB", "x", "co", "VV")
lcr = olut.Lut(d["cr"], d["inc_cr"], d["wcr"], None, "dB", "x", "cr", "VH")
co, cr = lut_dicts(lco, lcr)
ctx.upload_luts(co=co, cr=cr)
for tag in ("f64", "f32"):
    inc, sco, scr, dsig, anc = (d[tag + "/" + k] for k in ("inc", "sco", "scr", "dsig", "anc"))
    o_co, o_cr, o_idx = (d[tag + "/" + k] for k in ("o_co", "o_cr", "o_idx"))
    t_in = [torch.from_numpy(a).to(dev) for a in (inc, sco, scr, dsig, anc)]
    xdt = _lib.XSW_F32 if tag == "f32" else _lib.XSW_F64
    for mode in ("mono", "dual"):
        dual = mode == "dual"
        want_idx = o_idx.copy()
        if not dual:
            want_idx[..., 2] = -1
        for path in ("host", "device"):
            ctx.timing_enable(True)
            ctx.stats_enable(2)
            if path == "host":
                got_co, got_cr, idx = ctx.invert_host(inc, sigma0_co=sco, sigma0_cr=scr if dual else None, dsig_cr=dsig if dual else None, anc=anc,
                                                      dsig_co={dsig_co!r}, sigma0_is_db=True, algo="pruned", want_idx=True)
                tm = dict(last_band2_pixels=-1, last_list_pixels=-1, last_blocks_pixels=-1)
            else:
                out_co = torch.full(inc.shape, float("nan"), dtype=torch.complex128, device=dev)
                out_cr = torch.full(inc.shape, float("nan"), dtype=torch.complex128, device=dev) if dual else None
                t_idx = torch.full(inc.shape + (3,), -7, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ctx.invert_raw(inc.shape[0], inc.shape[1], xdt, _lib.XSW_F64, _lib.MEM_DEVICE, t_in[0].data_ptr(), t_in[1].data_ptr(),
                               t_in[2].data_ptr() if dual else None, t_in[3].data_ptr() if dual else None, t_in[4].data_ptr(), out_co.data_ptr(),
                               out_cr.data_ptr() if dual else None, out_idx=t_idx.data_ptr(), dsig_co={dsig_co!r}, sigma0_is_db=True,
                               algo=_lib.ALGO_PRUNED)
                tm = ctx.timing()
                got_co, got_cr, idx = out_co.cpu().numpy(), (out_cr.cpu().numpy() if dual else None), t_idx.cpu().numpy()
            ch = ctx.stats_chain()
            ctx.stats_enable(False)
            ctx.timing_enable(False)
            print("RESULT", tag, mode, path, int(np.sum(np.any(idx != want_idx, axis=-1))), close(got_co, o_co, 1e-12),
                  close(got_cr, o_cr, 1e-9) if dual else "ok", tm["last_band2_pixels"], tm["last_list_pixels"], tm["last_blocks_pixels"],
                  ch["cand_band2"], ch["cand_blocks"], ch["cand_list"], ch["pixels_refined"])
ctx.close()
print("SECONDS %.2f" % (time.perf_counter() - t0))
"""
FIELDS = ("idx_mismatch", "co", "cr", "band2_px", "list_px", "blocks_px", "cand_band2", "cand_blocks", "cand_list", "refined")


@pytest.mark.parametrize("route", ["no-band", "all-blocks", "cap64"])
def test_forced_routes(route, route_problem):
    """Three routes of tests/test_gpu_route_geometry.py on the `default` axes, one child process each (the routing switches are read
    once per process): the general kernel alone, every window through the block pyramid, work lists of 64 entries."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("XSW_") or k == "XSW_LIB"}
    env.update(ROUTES[route])
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, npz=route_problem, dsig_co=ic.DSIG_CO)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[:1] == ["RESULT"]:
            rows[tuple(t[1:4])] = {k: (v if k in ("co", "cr") else int(v)) for k, v in zip(FIELDS, t[4:])}
    print(f"route {route}: process {time.perf_counter() - t0:.1f} s" + "".join("\n  " + ln for ln in r.stdout.splitlines()))
    assert len(rows) == 8, r.stdout[-2000:]
    for key, v in rows.items():
        assert v["idx_mismatch"] == 0, f"{route} {key}: grid indices differ from the oracle on {v['idx_mismatch']} pixels"
        assert v["co"] == "ok", f"{route} {key}: co-pol wind {v['co']}"
        assert v["cr"] == "ok", f"{route} {key}: cross-pol wind {v['cr']}"
        assert v["cand_list"] > 0, (route, key, "k_invert_list scored nothing", v)
        if route == "no-band":  # the one-kernel path: no list is written
            assert v["cand_band2"] == 0 and v["cand_blocks"] == 0, (route, key, v)
        if route == "cap64" and key[2] == "device":
            assert v["list_px"] > LIST_CAP, (route, key, "list G did not overflow", v)


# ------------------------------------------------------------------------------------------------ from-codes kernels
@pytest.mark.parametrize("tag", list(DTYPES))
def test_from_codes_kernels(gpu_ctx, torch, axis_set, tag):  # noqa: F811
    """The seven from-codes entries on the oracle's winning codes, each against its restatement as its own GPU test compares it."""
    from xsarsea_amd import _lib
    c = ic.case(axis_set, DTYPES[tag])
    ctx, sc, ref, cc, ccr = install(gpu_ctx, axis_set), c["sc"], c["ref"], c["cc"], c["ccr"]
    inc, sco, scr, dsig, anc = (sc[k] for k in ("inc", "sco", "scr", "dsig", "anc"))
    what = f"{axis_set} {tag}"
    live = c["i_inc"] >= 0
    assert np.all(cc[live] < 0x80000000) and np.all(ccr[live] < _lib.CODE_NO_INDEX) and np.all(cc[~live] == _lib.CODE_NAN_RE)

    got = tcost._cost(ctx, torch, _lib, "co", (inc, cc, sco, anc), np.float64, True, dsig_co=ic.DSIG_CO)
    tcost._assert_fields(got, ref["cost_co"], np.float64, f"{what} cost_from_codes")
    got = tcost._cost(ctx, torch, _lib, "cr", (inc, cc, ccr, scr, dsig), np.float64, True)
    tcost._assert_fields(got, ref["cost_cr"], np.float64, f"{what} cost_cr_from_codes")

    got = tcross._cross(ctx, torch, _lib, inc, cc, scr, dsig, np.complex128, False, is_db=True)
    bad = got[0] != ref["cross"][0]
    print(f"{what} cross_from_codes: codes differ from the restatement on {int(bad.sum())} pixels")
    assert not bad.any(), f"{what} cross_from_codes: {int(bad.sum())} codes differ from the restatement, first at incidence {inc[bad][:4]!r}"
    assert np.array_equal(got[0], ccr), f"{what} cross_from_codes: not the oracle's cross-pol indices"
    assert bits_equal(got[1], ref["cross"][1]), f"{what} cross_from_codes: winds differ from the restatement"

    got = tjoint._joint(ctx, torch, _lib, (inc, cc, sco, anc, scr, dsig), np.float64, dsig_co=ic.DSIG_CO)
    tjoint._assert_equal(got, ref["joint"], np.float64, f"{what} joint_from_codes")

    got = tunc._unc(ctx, torch, _lib, "co", (inc, cc, sco, anc), np.float64, True, dsig_co=ic.DSIG_CO)
    tunc._assert_fields("co", got, ref["unc_co"], np.float64, f"{what} uncertainty_from_codes")
    got = tunc._unc(ctx, torch, _lib, "cr", (inc, cc, ccr, scr, dsig), np.float64, True)
    tunc._assert_fields("cr", got, ref["unc_cr"], np.float64, f"{what} uncertainty_cr_from_codes")

    got = tuj._uj(ctx, torch, _lib, (inc, ref["joint"]["code"], sco, anc, scr, dsig), np.float64, dsig_co=ic.DSIG_CO)
    tuj._assert_fields(got, ref["unc_joint"], np.float64, f"{what} uncertainty_joint_from_codes")
    assert np.all(got[6][live] == 0) and not np.isnan(got[0][live]).any()  # error bars on every probe: nothing compares NaN with NaN
