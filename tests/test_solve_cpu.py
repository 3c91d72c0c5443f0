"""CPU: wind speed at a known direction.  The numpy restatement tests/solve_ref.py -- a bisection over the
leading monotone rows, then a scan -- is held to its plain meaning (the first bracketing cell by a linear scan, a second
function), to the forward restatement tests/forward_ref.py by the round trip, and to hand-made tables where every answer is known;
the Python layer (`retrieve_wspd`) is run with the engine's two calls replaced by the restatement, and its refusals without the
shared library."""
import numpy as np
import pytest

import forward_ref as fref
import solve_ref as sref
from conftest import golden
from test_forward_cpu import _bits_equal, array_model, no_library  # noqa: F401 (fixtures)
from util import small_luts

from xsarsea_amd import _lib, windspeed
from xsarsea_amd.windspeed import _engine, retrieve

N_SCENE = 40000


def _scene(table, ai, aw, ap, n, seed, noise):
    """(inc, s, phi) inside the axes: coordinates also on nodes (forward_ref.points, no margins, its NaN pixels kept), s the
    restated forward value at a uniform speed (+ N(0, noise) dB), and for every seventh pixel exactly a node value c(k)."""
    rng = np.random.default_rng(seed)
    axes = (ai, aw) if ap is None else (ai, aw, ap)
    cols = fref.points(rng, axes, n, (0.0, 0.0, 0.0))
    inc, w = cols[0], cols[1]
    phi = None if ap is None else cols[2]
    s = (fref.eval_cr(table, ai, aw, inc, w) if ap is None else fref.eval_co(table, ai, aw, ap, inc, w, phi))["sigma0_db"]
    on = np.flatnonzero((np.arange(n) % 7 == 0) & np.isfinite(s))
    s[on] = sref.node_values(table, ai, ap, inc[on], None if ap is None else phi[on], rng.integers(0, len(aw), len(on)))
    if noise:
        s = s + rng.normal(0.0, noise, n)
    return inc, s, phi


def _same_bracket_and_speed(a, b, what):
    differ = int(np.sum(a["k"] != b["k"])) + int(np.sum(~((a["wspd"] == b["wspd"]) | (np.isnan(a["wspd"]) & np.isnan(b["wspd"])))))
    print(f"{what}: pixels whose bracket or speed differs from the linear scan: {differ}; solved share {(a['k'] >= 0).mean():.3f}, "
          f"TAIL {(a['flag'] & sref.TAIL > 0).mean():.3f}")
    assert differ == 0, what
    assert _bits_equal(a["sens"], b["sens"])


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_restatement_equals_linear_scan_default_table(default_luts, noise):
    lco, lcr = default_luts
    co = (np.asarray(lco.values, dtype=np.float64), lco.incidence, lco.wspd, lco.phi)
    mono = sref.mono_rows(co[0])
    print(f"mono_rows of the default table: {mono.min()} .. {mono.max()}")
    assert mono.min() >= 2 and mono.max() == len(lco.wspd) and mono.min() < len(lco.wspd)  # CMOD5.N turns over at low incidence
    inc, s, phi = _scene(*co, N_SCENE, 31, noise)
    got, scan = sref.solve_co(*co, inc, s, phi, mono=mono), sref.solve_co_scan(*co, inc, s, phi)
    _same_bracket_and_speed(got, scan, f"co-pol, noise {noise}")
    assert (got["k"] >= 0).mean() > 0.5 and (got["flag"] & sref.TAIL > 0).any()
    # round trip against the forward restatement (its axis order differs: to rounding, with two orders of margin)
    ok = got["k"] >= 0
    back = fref.eval_co(*co, inc[ok], got["wspd"][ok], phi[ok])["sigma0_db"]
    err = np.abs(back - s[ok]).max()
    print(f"round trip: {err:.3g} dB")
    assert err <= 1e-10
    cr = (np.asarray(lcr.values, dtype=np.float64), lcr.incidence, lcr.wspd)
    inc, s, _ = _scene(*cr, None, N_SCENE, 32, noise)
    got, scan = sref.solve_cr(*cr, inc, s), sref.solve_cr_scan(*cr, inc, s)
    _same_bracket_and_speed(got, scan, f"cross-pol, noise {noise}")
    ok = got["k"] >= 0
    assert ok.mean() > 0.5 and np.abs(fref.eval_cr(*cr, inc[ok], got["wspd"][ok])["sigma0_db"] - s[ok]).max() <= 1e-10


@pytest.mark.parametrize("name", ["phi180", "phi360", "phi90", "nonuniform", "turnover", "falling"])
def test_restatement_equals_linear_scan_small_tables(name):
    if name == "nonuniform":
        co, cr = fref.nonuniform_tables()
    elif name in ("turnover", "falling"):
        co, cr = getattr(sref, f"{name}_table")()[:4], sref.nonmonotone_cr()
    else:
        lco, lcr = small_luts(golden(f"kernel_small_{name}_f64.npz"))
        co, cr = (lco.values, lco.incidence, lco.wspd, lco.phi), (lcr.values, lcr.incidence, lcr.wspd)
    for noise in (0.0, 0.5):
        inc, s, phi = _scene(*co, 3000, 5, noise)
        got = sref.solve_co(*co, inc, s, phi)
        _same_bracket_and_speed(got, sref.solve_co_scan(*co, inc, s, phi), f"{name} co-pol, noise {noise}")
        ok = got["k"] >= 0
        assert ok.any() and np.abs(fref.eval_co(*co, inc[ok], got["wspd"][ok], phi[ok])["sigma0_db"] - s[ok]).max() <= 1e-10
        inc, s, _ = _scene(*cr, None, 3000, 6, noise)
        got = sref.solve_cr(*cr, inc, s)
        _same_bracket_and_speed(got, sref.solve_cr_scan(*cr, inc, s), f"{name} cross-pol, noise {noise}")
        ok = got["k"] >= 0
        assert ok.any() and np.abs(fref.eval_cr(*cr, inc[ok], got["wspd"][ok])["sigma0_db"] - s[ok]).max() <= 1e-10


def test_exact_on_an_affine_table():
    co, ai, aw, ap = fref.affine_table()
    k = fref.AFFINE
    rng = np.random.default_rng(5)
    inc = rng.integers(ai[0] * 8, ai[-1] * 8 + 1, 600) / 8
    w = rng.integers(aw[0] * 8, aw[-1] * 8 + 1, 600) / 8
    p = rng.integers(ap[0] * 8, ap[-1] * 8 + 1, 600) / 8
    s = k["a"] + k["b"] * inc + k["c"] * w + k["d"] * p + k["e"] * w * p
    out = sref.solve_co(co, ai, aw, ap, inc, s, p, fold_phi=False)
    assert np.array_equal(out["wspd"], w) and not out["flag"].any()
    assert np.array_equal(out["sens"], 1.0 / (k["c"] + k["e"] * p))
    cr = co[:, :, 1]
    s = k["a"] + k["b"] * inc + (k["c"] + k["e"] * ap[1]) * w + k["d"] * ap[1]
    out = sref.solve_cr(cr, ai, aw, inc, s, monotone=True)
    assert np.array_equal(out["wspd"], w) and not out["flag"].any()
    assert not sref.cr_monotone(cr, aw) and sref.cr_monotone(cr[:, :2], aw[:2])  # (1, 2, 4, 8 is no uniform axis)


def _one(table, ai, aw, ap, inc, s, phi=0.0, **kw):
    out = sref.solve_co(table, ai, aw, ap, np.array([inc]), np.array([s]), np.array([phi]), **kw)
    return float(out["wspd"][0]), float(out["sens"][0]), int(out["flag"][0]), int(out["k"][0])


def test_hand_made_tables():
    """At inc = 20, phi = 0 the turnover table's column is its first row, c = -20 -16 -12 -12 -18 -22 -14 -6 at the speeds
    1 2 4 5 7 8 10 12; M = min(4, 3) = 3 there (the two slices' monotone rows differ)."""
    co, ai, aw, ap, mono = sref.turnover_table()
    assert np.array_equal(sref.mono_rows(co), mono)
    t = (co, ai, aw, ap)
    nan = float("nan")
    assert _one(*t, 20.0, -16.0) == (2.0, 0.25, 0, 0)           # s on a node value: the cell below it
    assert _one(*t, 20.0, -20.0) == (1.0, 0.25, 0, 0)           # s == c(0)
    assert _one(*t, 20.0, -12.0) == (4.0, 0.5, 0, 1)            # the top of cell 1, not the flat cell after it
    assert _one(*t, 20.0, -15.0) == (2.5, 0.5, 0, 1)            # the first of three crossings
    assert _one(*t, 20.0, -8.0) == (11.5, 0.25, sref.TAIL, 6)   # above the leading rows: found by the scan
    assert _one(*t, 20.0, -21.0) == (7.75, -0.25, sref.TAIL, 4)  # below c(0), met where the table falls
    w, sens, flag, k = _one(*t, 20.0, -5.0)
    assert np.isnan(w) and np.isnan(sens) and (flag, k) == (sref.ABOVE, -1)
    w, sens, flag, k = _one(*t, 20.0, -23.0)
    assert np.isnan(w) and np.isnan(sens) and (flag, k) == (sref.BELOW, -1)
    # M = 1 and M = 0: the scan alone, from row 0
    for m in (1, 0):
        assert _one(*t, 20.0, -15.0, mono=[m, m, m]) == (2.5, 0.5, sref.TAIL, 1)
        assert _one(*t, 20.0, -20.0, mono=[m, m, m]) == (1.0, 0.25, sref.TAIL, 0)
    # M = n_w: a table that rises throughout is bisected over all its rows
    rising = np.repeat(co[2:3], 3, axis=0)
    assert np.array_equal(sref.mono_rows(rising), [8, 8, 8])
    assert _one(rising, ai, aw, ap, 24.0, -11.0) == (11.0, 1.0, 0, 6)
    assert _one(rising, ai, aw, ap, 24.0, -10.0) == (12.0, 1.0, 0, 6)  # the last node
    assert _one(rising, ai, aw, ap, 24.0, -9.5)[2] == sref.ABOVE
    # a flat cell holding s: w = aw[k], the sensitivity is infinite
    flat = co.copy()
    flat[:, 1] = flat[:, 0]
    assert _one(flat, ai, aw, ap, 20.0, -20.0) == (1.0, float("inf"), 0, 0)
    assert _one(flat, ai, aw, ap, 20.0, -20.0, mono=[0, 0, 0]) == (1.0, float("inf"), sref.TAIL, 0)
    # the gate: NaN and outside coordinates, a sigma0 that is not finite
    for inc, s, phi in ((nan, -15.0, 0.0), (20.0, nan, 0.0), (20.0, -15.0, nan), (19.0, -15.0, 0.0), (28.5, -15.0, 0.0), (20.0, -15.0, 17.0),
                        (20.0, float("inf"), 0.0), (20.0, float("-inf"), 0.0)):
        w, sens, flag, k = _one(*t, inc, s, phi)
        assert np.isnan(w) and np.isnan(sens) and (flag, k) == (sref.NAN, -1), (inc, s, phi)
    assert _one(*t, 20.0, -15.0, -16.0, fold_phi=False)[2] == sref.NAN and _one(*t, 20.0, -13.0, -16.0) == (2.5, 0.5, 0, 1)  # folded: phi = 16
    # an all-falling table: the scan alone; c = -12 -14 -18 -26 at the speeds 1 2 4 8
    co, ai, aw, ap, mono = sref.falling_table()
    assert np.array_equal(sref.mono_rows(co), mono)
    t = (co, ai, aw, ap)
    assert _one(*t, 20.0, -16.0) == (3.0, -0.5, sref.TAIL, 1)
    assert _one(*t, 20.0, -12.0) == (1.0, -0.5, sref.TAIL, 0)
    assert _one(*t, 20.0, -11.0)[2] == sref.ABOVE and _one(*t, 20.0, -30.0)[2] == sref.BELOW
    # a cross-pol table that is not monotone: scanned from row 0; the same table declared monotone is bisected
    cr, ai, aw = sref.nonmonotone_cr()
    assert not sref.cr_monotone(cr, aw)
    out = sref.solve_cr(cr, ai, aw, np.full(4, 20.0), np.array([-25.0, -30.0, -11.0, -31.0]))
    assert np.array_equal(out["wspd"][:2], [2.25, 1.0]) and np.array_equal(out["flag"], [sref.TAIL, sref.TAIL, sref.ABOVE, sref.BELOW])
    rising = np.sort(cr, axis=1)
    assert sref.cr_monotone(rising, aw) and not sref.solve_cr(rising, ai, aw, np.full(2, 20.0), np.array([-25.0, -12.0]))["flag"].any()


# ------------------------------------------------------------------------------------------------ the Python layer, no device
@pytest.fixture
def ref_engine(monkeypatch):
    """`_engine.wspd_solve` / `wspd_solve_cr` replaced by the restatement on the LUT object they are handed; records the calls."""
    calls = []

    def outs(r, details, out_dtype):
        with np.errstate(all="ignore"):
            return [r["wspd"].astype(out_dtype)] + ([r["sens"].astype(out_dtype), r["flag"]] if details else [])

    def wspd_solve(lut, plan, inc, sigma0_db, phi, fold_phi=True, details=False, out_dtype=np.float64):
        calls.append(dict(kind="co", lut=lut, plan=plan, fold_phi=fold_phi, details=details, out_dtype=out_dtype, sigma0_db=sigma0_db, phi=phi))
        return outs(sref.solve_co(lut.values, lut.incidence, lut.wspd, lut.phi, inc, sigma0_db, phi, fold_phi=fold_phi), details, out_dtype)

    def wspd_solve_cr(lut, plan, inc, sigma0_db, details=False, out_dtype=np.float64):
        calls.append(dict(kind="cr", lut=lut, plan=plan, details=details, out_dtype=out_dtype, sigma0_db=sigma0_db))
        return outs(sref.solve_cr(lut.values, lut.incidence, lut.wspd, inc, sigma0_db), details, out_dtype)

    monkeypatch.setattr(_engine, "wspd_solve", wspd_solve)
    monkeypatch.setattr(_engine, "wspd_solve_cr", wspd_solve_cr)
    return calls


def _small(name="phi180"):
    lco, lcr = small_luts(golden(f"kernel_small_{name}_f64.npz"))
    return (lco.values, lco.incidence, lco.wspd, lco.phi), (lcr.values, lcr.incidence, lcr.wspd)


def _rasters(co, shape=(5, 7), seed=8):
    table, ai, aw, ap = co
    rng = np.random.default_rng(seed)
    inc, w, p = rng.uniform(ai[0], ai[-1], shape), rng.uniform(aw[0], aw[-1], shape), rng.uniform(-170.0, 170.0, shape)
    return inc, fref.eval_co(table, ai, aw, ap, inc, w, p)["sigma0_db"], p


def test_retrieve_wspd(array_model, ref_engine, no_library):
    co, cr = _small()
    m = array_model("gmf_solvetest", *co)
    mcr = array_model("gmf_solvetest_cr", *cr, pol="VH")
    inc, s_db, p = _rasters(co)
    want = sref.solve_co(*co, inc, s_db, p)
    got = windspeed.retrieve_wspd(inc, s_db, p, model="gmf_solvetest", units="dB")
    assert isinstance(got, np.ndarray) and _bits_equal(got, want["wspd"]) and np.isfinite(got).any()
    c = ref_engine[-1]
    assert c["kind"] == "co" and c["fold_phi"] is True and c["details"] is False and c["out_dtype"] == np.float64 and c["lut"] is m._lut(units="dB")
    assert c["sigma0_db"] is s_db and c["phi"] is p and c["plan"].dtype == np.float64 and c["plan"].shape == inc.shape
    # units: linear by default, 10 log10(sigma0 + 1e-15) in sigma0's own dtype by the engine's helper
    lin = 10 ** (s_db / 10)
    got = windspeed.retrieve_wspd(inc, lin, p, model=m)
    assert np.array_equal(ref_engine[-1]["sigma0_db"], 10 * np.log10(lin + 1e-15))
    assert _bits_equal(got, sref.solve_co(*co, inc, 10 * np.log10(lin + 1e-15), p)["wspd"])
    lin32 = lin.astype(np.float32)
    windspeed.retrieve_wspd(inc.astype(np.float32), lin32, p.astype(np.float32), model=m)
    assert ref_engine[-1]["sigma0_db"].dtype == np.float32 and ref_engine[-1]["plan"].dtype == np.float32
    assert np.array_equal(ref_engine[-1]["sigma0_db"], 10 * np.log10(lin32 + np.float32(1e-15)))
    # details, out_dtype, fold_phi
    r = windspeed.retrieve_wspd(inc, s_db, p, model=m, units="dB", details=True, out_dtype=np.float32)
    assert isinstance(r, windspeed.RetrievedWspd) and r["wspd"] is r.wspd and r.wspd.dtype == np.float32 and r.flag.dtype == np.uint8
    with np.errstate(all="ignore"):
        assert _bits_equal(r.wspd, want["wspd"].astype(np.float32)) and _bits_equal(r.dwspd_dsigma0, want["sens"].astype(np.float32))
    assert np.array_equal(r.flag, want["flag"])
    unfolded = windspeed.retrieve_wspd(inc, s_db, p, model=m, units="dB", fold_phi=False, details=True)
    assert ref_engine[-1]["fold_phi"] is False and np.all(unfolded.flag[p < 0] == _lib.SOLVE_NAN) and (p < 0).any()
    # scalar phi is expanded; wind=: the angle alone, by the array module
    assert _bits_equal(windspeed.retrieve_wspd(inc, s_db, 30, model=m, units="dB"), sref.solve_co(*co, inc, s_db, np.full(inc.shape, 30.0))["wspd"])
    wind = 7.0 * np.exp(1j * np.deg2rad(p))
    got = windspeed.retrieve_wspd(inc, s_db, wind=wind, model=m, units="dB")
    assert np.array_equal(ref_engine[-1]["phi"], np.degrees(np.angle(wind)))
    assert _bits_equal(got, sref.solve_co(*co, inc, s_db, np.degrees(np.angle(wind)))["wspd"])
    # cross-pol: neither phi nor wind; both units
    table, ai, aw = cr
    wcr = np.random.default_rng(2).uniform(aw[0], aw[-1], inc.shape)
    s_cr = fref.eval_cr(*cr, inc, wcr)["sigma0_db"]
    r = windspeed.retrieve_wspd(inc, s_cr, model=mcr, units="dB", details=True)
    want = sref.solve_cr(*cr, inc, s_cr)
    assert ref_engine[-1]["kind"] == "cr" and _bits_equal(r.wspd, want["wspd"]) and _bits_equal(r.dwspd_dsigma0, want["sens"]) and np.array_equal(r.flag, want["flag"])
    ok = np.isfinite(r.wspd)  # (the lowest solution: not wcr where the table turns over)
    assert ok.any() and np.abs(fref.eval_cr(*cr, inc[ok], r.wspd[ok])["sigma0_db"] - s_cr[ok]).max() <= 1e-10
    lin = 10 ** (s_cr / 10)
    assert _bits_equal(windspeed.retrieve_wspd(inc, lin, model=mcr), sref.solve_cr(*cr, inc, 10 * np.log10(lin + 1e-15))["wspd"])
    # resolution passes through to to_lut
    windspeed.retrieve_wspd(inc, s_db, p, model=m, units="dB", resolution="high")
    assert ref_engine[-1]["lut"] is m._lut(units="dB", resolution="high")
    assert "retrieve_wspd" in windspeed.__all__ and windspeed.RetrievedWspd is retrieve.RetrievedWspd
    assert (_lib.SOLVE_NAN, _lib.SOLVE_BELOW, _lib.SOLVE_ABOVE, _lib.SOLVE_TAIL) == (sref.NAN, sref.BELOW, sref.ABOVE, sref.TAIL)


def test_retrieve_wspd_refusals(array_model, ref_engine, no_library, xr_env):
    co, cr = _small()
    m = array_model("gmf_solvetest_ref", *co)
    mcr = array_model("gmf_solvetest_ref_cr", *cr, pol="VH")
    inc, s, p = _rasters(co)
    wind = 7.0 * np.exp(1j * np.deg2rad(p))
    ret = windspeed.retrieve_wspd
    with pytest.raises(TypeError, match="xarray / dask"):
        ret(xr_env.xr.DataArray(inc, dims=("line", "sample")), s, p, model=m)
    with pytest.raises(TypeError, match="xarray / dask"):
        ret(inc, s, wind=xr_env.xr.DataArray(wind, dims=("line", "sample")), model=m)
    with pytest.raises(ValueError, match="not both"):
        ret(inc, s, p, wind=wind, model=m)
    with pytest.raises(ValueError, match="phi"):
        ret(inc, s, model=m)
    with pytest.raises(ValueError, match="takes no phi"):
        ret(inc, s, p, model=mcr)
    with pytest.raises(ValueError, match="takes no phi"):
        ret(inc, s, wind=wind, model=mcr)
    with pytest.raises(ValueError, match="one shape"):
        ret(inc, s[:, :3], p, model=m)
    with pytest.raises(ValueError, match="one shape"):
        ret(inc, s, p[:2], model=m)
    with pytest.raises(ValueError, match="shape"):
        ret(inc, s, wind=wind[:2], model=m)
    with pytest.raises(ValueError, match="Unit not known"):
        ret(inc, s, p, model=m, units="db")
    with pytest.raises(ValueError, match="out_dtype"):
        ret(inc, s, p, model=m, out_dtype=np.int32)
    with pytest.raises(TypeError, match="complex"):
        ret(inc, s, wind=p, model=m)
    with pytest.raises(TypeError, match="float32 or float64"):
        ret(inc, s.astype(np.int32), p, model=m)
    with pytest.raises(TypeError, match="sigma0 must be"):
        ret(inc, 0.01, p, model=m)
    with pytest.raises(KeyError):
        ret(inc, s, p, model="gmf_no_such_model")

    class DeviceArray:  # a device array by its interface; never dereferenced
        def __init__(self, a):
            self.__cuda_array_interface__ = dict(shape=a.shape, typestr=a.dtype.str, data=(0, False), version=3)

    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, DeviceArray(s), p, model=m)
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, s, wind=DeviceArray(wind), model=m)
    with pytest.raises(ValueError, match="one container kind"):  # refused before the scalar is expanded, or sigma0 converted, on the device
        ret(DeviceArray(inc), s, 30.0, model=m)
    assert not ref_engine


def test_pair_gathers_stay_8_byte_loads():
    """As the forward kernels (csrc/xsw_forward.hpp: next_entry): the table pairs and the axis pair of the solution's cell are only
    8-byte aligned, so the built gfx950 code of the eight kernels holds 8-byte global loads and no wider one, no scratch, no LDS."""
    from xsarsea_amd import _build
    _build.build()
    kernels = _build.kernel_mnemonics("k_wspd_solve_")
    assert len(kernels) == 8 and sum("k_wspd_solve_co" in k for k in kernels) == 4, sorted(kernels)
    for name, ops in kernels.items():
        loads = {m: c for m, c in ops.items() if m.startswith("global_load")}
        print(name, loads)
        assert loads.get("global_load_dwordx2", 0) >= (4 if "k_wspd_solve_co" in name else 2), (name, loads)
        assert not any(m.startswith(("global_load_dwordx3", "global_load_dwordx4")) for m in loads), (name, loads)
        assert not any(m.startswith(("scratch_", "ds_")) for m in ops), name
