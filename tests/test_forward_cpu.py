"""CPU: the forward operator on rasters.  The numpy restatement tests/forward_ref.py is pinned bit for bit
to `LutModel.__call__`'s 1-D call (the three host `lerp_axis` passes, i.e. the reference's `lut.interp`); its fold and Jacobian
are checked on tables where they are known exactly; the Python layer (`simulate_sigma0`, `LutModel.__call__` on rasters) is run
with the engine's two calls replaced by the restatement, and its refusals without the shared library."""
import numpy as np
import pytest

import forward_ref as fref
from conftest import golden
from util import small_luts

from xsarsea_amd import _lib, windspeed
from xsarsea_amd.windspeed import _engine, forward, models
from xsarsea_amd.windspeed.lut import Lut

N = 400


def _tables(name):
    """((co, ai, aw, ap), (cr, ai, awcr)) of a golden's small LUTs or the non-uniform pair."""
    if name == "nonuniform":
        return fref.nonuniform_tables()
    lco, lcr = small_luts(golden(f"kernel_small_{name}_f64.npz"))
    return (lco.values, lco.incidence, lco.wspd, lco.phi), (lcr.values, lcr.incidence, lcr.wspd)


@pytest.fixture
def array_model():
    """make(name, table, axes..., pol) -> a registered ArrayLutModel over a dB table; unregistered afterwards."""
    made = []

    def make(name, table, ai, aw, ap=None, pol="VV"):
        made.append(name)
        return models.ArrayLutModel(name, Lut(table, ai, aw, ap, units="dB", resolution="high"), pol=pol)

    yield make
    for n in made:
        models.Model._available_models.pop(n, None)


def _diagonal(model, cols, batch=40):
    """The diagonal of LutModel.__call__'s 1-D call (an outer product over its arguments), in batches."""
    out = []
    for k in range(0, len(cols[0]), batch):
        a = np.asarray(model(*(c[k:k + batch] for c in cols), units="dB"))
        out.append(np.einsum("iii->i" if a.ndim == 3 else "ii->i", a))
    return np.concatenate(out)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64)[~np.isnan(a)], np.asarray(b, dtype=np.float64).view(np.uint64)[~np.isnan(b)]) \
        and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("name", ["phi180", "phi360", "phi90", "nonuniform"])
def test_restatement_equals_lutmodel_copol(array_model, name):
    (co, ai, aw, ap), _ = _tables(name)
    cols = fref.points(np.random.default_rng(11), (ai, aw, ap), N)
    for ax, x in zip((ai, aw, ap), cols):
        assert all(np.any(x == node) for node in ax), "every node of every axis is among the points"
        assert np.isnan(x).sum() == 1
    got = fref.eval_co(co, ai, aw, ap, *cols, fold_phi=False)["sigma0_db"]
    want = _diagonal(array_model(f"gmf_fwdtest_{name}", co, ai, aw, ap), cols)
    finite = np.isfinite(want).mean()
    print(f"{name}: finite share {finite:.3f}")
    assert finite >= 0.75 and 1 - finite >= 0.05
    assert _bits_equal(got, want)


@pytest.mark.parametrize("name", ["phi180", "nonuniform"])
def test_restatement_equals_lutmodel_crosspol(array_model, name):
    _, (cr, ai, aw) = _tables(name)
    cols = fref.points(np.random.default_rng(12), (ai, aw), N)
    got = fref.eval_cr(cr, ai, aw, *cols)["sigma0_db"]
    want = _diagonal(array_model(f"gmf_fwdtest_cr_{name}", cr, ai, aw, pol="VH"), cols)
    finite = np.isfinite(want).mean()
    print(f"{name} cross-pol: finite share {finite:.3f}")
    assert finite >= 0.75 and 1 - finite >= 0.05
    assert _bits_equal(got, want)


def test_fold():
    phi = np.concatenate([np.linspace(-720.0, 720.0, 2881), [100.0, 260.0, -0.0, 359.999]])
    for last in (90.0, 180.0, 360.0):
        p, reflected = fref.fold(phi, last)
        raw = np.where(np.fmod(phi, 360.0) < 0, np.fmod(phi, 360.0) + 360.0, np.fmod(phi, 360.0))
        assert np.all((raw >= 0) & (raw < 360.0)) and np.all((p >= 0) & (p <= 360.0))
        assert np.array_equal(reflected, raw > last)
        if last == 360.0:
            assert not reflected.any()
    (co, ai, aw, ap), _ = _tables("phi180")
    rng = np.random.default_rng(3)
    ph = rng.uniform(-400, 400, 500)
    inc, w = rng.uniform(ai[0], ai[-1], 500), rng.uniform(aw[0], aw[-1], 500)
    a, b = fref.eval_co(co, ai, aw, ap, inc, w, ph), fref.eval_co(co, ai, aw, ap, inc, w, -ph)
    assert np.isfinite(a["sigma0_db"]).all()
    # phi and -phi agree on a 0..180 table; the fold of -phi is 360 - fold(phi) before the reflection, which is not always the
    # same float64: equal to the last bits, and exactly so where phi is a multiple of 1/8 degree
    assert np.allclose(a["sigma0_db"], b["sigma0_db"], rtol=0, atol=1e-9)
    q = np.round(ph * 8) / 8
    a, b = fref.eval_co(co, ai, aw, ap, inc, w, q), fref.eval_co(co, ai, aw, ap, inc, w, -q)
    assert _bits_equal(a["sigma0_db"], b["sigma0_db"]) and _bits_equal(a["dwspd"], b["dwspd"])
    both = a["reflected"] != b["reflected"]
    assert both.any() and np.array_equal(a["dphi"][both], -b["dphi"][both])
    # dphi changes sign exactly where reflected
    plain = fref.eval_co(co, ai, aw, ap, inc, w, fref.fold(q, 180.0)[0], fold_phi=False)
    assert np.array_equal(a["dphi"], np.where(a["reflected"], -plain["dphi"], plain["dphi"])) and a["reflected"].any() and not a["reflected"].all()
    # a 0..360 table never reflects; a 0..90 table leaves 100 and 260 degrees outside
    (co, ai, aw, ap), _ = _tables("phi360")
    assert not fref.eval_co(co, ai, aw, ap, inc, w, ph)["reflected"].any()
    (co, ai, aw, ap), _ = _tables("phi90")
    out = fref.eval_co(co, ai, aw, ap, inc[:2], w[:2], np.array([100.0, 260.0]))
    assert np.isnan(out["sigma0_db"]).all() and np.isnan(out["dphi"]).all() and np.isnan(out["dwspd"]).all()
    assert np.isfinite(fref.eval_co(co, ai, aw, ap, inc[:2], w[:2], np.array([80.0, 280.0]))["sigma0_db"]).all()


def test_jacobian_exact_on_an_affine_table():
    co, ai, aw, ap = fref.affine_table()
    k = fref.AFFINE
    rng = np.random.default_rng(5)
    inc = rng.integers(ai[0] * 8, ai[-1] * 8 + 1, 600) / 8
    w = rng.integers(aw[0] * 8, aw[-1] * 8 + 1, 600) / 8
    p = rng.integers(ap[0] * 8, ap[-1] * 8 + 1, 600) / 8
    out = fref.eval_co(co, ai, aw, ap, inc, w, p, fold_phi=False)
    assert np.array_equal(out["sigma0_db"], k["a"] + k["b"] * inc + k["c"] * w + k["d"] * p + k["e"] * w * p)
    assert np.array_equal(out["dwspd"], k["c"] + k["e"] * p) and np.array_equal(out["dphi"], k["d"] + k["e"] * w)
    cr = co[:, :, 1]
    out = fref.eval_cr(cr, ai, aw, inc, w)
    assert np.array_equal(out["dwspd"], np.full(600, k["c"] + k["e"] * ap[1])) and np.array_equal(out["sigma0_db"], k["a"] + k["b"] * inc + (k["c"] + k["e"] * ap[1]) * w + k["d"] * ap[1])


# ------------------------------------------------------------------------------------------------ the Python layer, no device
@pytest.fixture
def no_library(monkeypatch):
    """The shared library cannot be loaded and no context can be made: a refusal that reaches either fails the test."""
    def boom(*a, **k):
        raise AssertionError("the shared library was asked for")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


@pytest.fixture
def ref_engine(monkeypatch):
    """`_engine.lut_eval` / `lut_eval_cr` replaced by the restatement on the LUT object they are handed; records the calls."""
    calls = []

    def lut_eval(lut, plan, inc, wspd, phi, fold_phi=True, jacobian=False, out_dtype=np.float64):
        calls.append(dict(kind="co", lut=lut, plan=plan, fold_phi=fold_phi, jacobian=jacobian, out_dtype=out_dtype))
        r = fref.eval_co(lut.values, lut.incidence, lut.wspd, lut.phi, inc, wspd, phi, fold_phi=fold_phi)
        return [r[k].astype(out_dtype) for k in (("sigma0_db", "dwspd", "dphi") if jacobian else ("sigma0_db",))]

    def lut_eval_cr(lut, plan, inc, wspd, jacobian=False, out_dtype=np.float64):
        calls.append(dict(kind="cr", lut=lut, plan=plan, jacobian=jacobian, out_dtype=out_dtype))
        r = fref.eval_cr(lut.values, lut.incidence, lut.wspd, inc, wspd)
        return [r[k].astype(out_dtype) for k in (("sigma0_db", "dwspd") if jacobian else ("sigma0_db",))]

    monkeypatch.setattr(_engine, "lut_eval", lut_eval)
    monkeypatch.setattr(_engine, "lut_eval_cr", lut_eval_cr)
    return calls


def _rasters(ai, aw, ap, shape=(5, 7), seed=8):
    rng = np.random.default_rng(seed)
    return rng.uniform(ai[0], ai[-1], shape), rng.uniform(aw[0], aw[-1], shape), rng.uniform(ap[0] - 3, ap[-1] + 3, shape)


def test_lutmodel_call_on_rasters(array_model, ref_engine, no_library):
    """`model(inc2d, wspd2d, phi2d, units="dB")`: pointwise, no fold, equal to the diagonal of the 1-D call.  (Before this route
    existed the call raised NotImplementedError("Only scalar or 1D array are implemented for LutModel").)"""
    (co, ai, aw, ap), (cr, _, awcr) = _tables("phi180")
    m = array_model("gmf_fwdtest_call", co, ai, aw, ap)
    inc, w, p = _rasters(ai, aw, ap)
    got = m(inc, w, p, units="dB")
    assert isinstance(got, np.ndarray) and got.shape == inc.shape and got.dtype == np.float64
    assert ref_engine[-1]["kind"] == "co" and ref_engine[-1]["fold_phi"] is False and ref_engine[-1]["lut"] is m._lut(units="dB")
    assert _bits_equal(got.ravel(), _diagonal(m, (inc.ravel(), w.ravel(), p.ravel())))
    assert np.isnan(got).any() and np.isfinite(got).any()  # beyond the last direction: NaN, not folded
    assert _bits_equal(m(inc, w, p), got)  # units=None resolves to the table's own dB
    assert _bits_equal(m(inc[None], w[None], p[None], units="dB")[0], got)  # three axes
    mcr = array_model("gmf_fwdtest_call_cr", cr, ai, awcr, pol="VH")
    wcr = np.random.default_rng(1).uniform(awcr[0], awcr[-1], inc.shape)
    assert _bits_equal(mcr(inc, wcr, units="dB").ravel(), _diagonal(mcr, (inc.ravel(), wcr.ravel())))
    assert ref_engine[-1]["kind"] == "cr"
    n_calls = len(ref_engine)
    # refusals, none of which reaches the engine: linear units, another shape, a missing / a surplus direction
    with pytest.raises(NotImplementedError, match="simulate_sigma0"):
        m(inc, w, p, units="linear")
    lin = array_model("gmf_fwdtest_call_lin", 10 ** (co / 10), ai, aw, ap)
    lin._table.attrs["units"] = "linear"
    with pytest.raises(NotImplementedError, match="simulate_sigma0"):
        lin(inc, w, p)
    with pytest.raises(NotImplementedError, match="Only scalar or 1D array are implemented for LutModel"):
        m(inc, w[:, :3], p)
    with pytest.raises(ValueError, match="Unit not known"):
        m(inc, w, p, units="db")
    with pytest.raises(NotImplementedError):
        m(inc, w[0], p)
    with pytest.raises(ValueError, match="takes no phi"):
        mcr(inc, wcr, p, units="dB")
    with pytest.raises(ValueError, match="needs phi"):
        m(inc, w, units="dB")
    assert len(ref_engine) == n_calls
    # scalar and 1-D behaviour is untouched, the outer-product meaning of three 1-D arrays included
    assert np.asarray(m(inc[0, :3], w[0, :4], p[0, :5], units="dB")).shape == (3, 4, 5)
    assert isinstance(m(float(inc[0, 0]), float(w[0, 0]), float(p[0, 0]), units="dB"), float)


def test_simulate_sigma0(array_model, ref_engine, no_library):
    (co, ai, aw, ap), (cr, _, awcr) = _tables("phi180")
    m = array_model("gmf_fwdtest_sim", co, ai, aw, ap)
    mcr = array_model("gmf_fwdtest_sim_cr", cr, ai, awcr, pol="VH")
    inc, w, p = _rasters(ai, aw, ap)
    p = p * 2 - 90  # beyond the table: folded
    want = fref.eval_co(co, ai, aw, ap, inc, w, p)
    got = windspeed.simulate_sigma0(inc, w, p, model="gmf_fwdtest_sim")
    assert _bits_equal(got, want["sigma0_db"]) and np.isfinite(got).all()
    assert ref_engine[-1]["fold_phi"] is True and ref_engine[-1]["lut"] is m._lut(units="dB") and ref_engine[-1]["out_dtype"] == np.float64
    jac = windspeed.simulate_sigma0(inc, w, p, model=m, jacobian=True, out_dtype=np.float32)
    assert isinstance(jac, windspeed.SimulatedSigma0) and jac["dwspd"] is jac.dwspd and jac.sigma0.dtype == np.float32
    assert all(_bits_equal(jac[k], want[n].astype(np.float32)) for k, n in (("sigma0", "sigma0_db"), ("dwspd", "dwspd"), ("dphi", "dphi")))
    assert _bits_equal(windspeed.simulate_sigma0(inc, w, p, model=m, fold_phi=False), fref.eval_co(co, ai, aw, ap, inc, w, p, fold_phi=False)["sigma0_db"])
    assert _bits_equal(windspeed.simulate_sigma0(inc, w, p, model=m, units="linear"), 10 ** (want["sigma0_db"] / 10))
    # wind=: the array module's modulus and degrees(angle); Python scalars are expanded
    wind = w * np.exp(1j * np.deg2rad(p))
    want_w = fref.eval_co(co, ai, aw, ap, inc, np.abs(wind), np.degrees(np.angle(wind)))
    assert _bits_equal(windspeed.simulate_sigma0(inc, wind=wind, model=m), want_w["sigma0_db"])
    assert _bits_equal(windspeed.simulate_sigma0(inc, 7.5, 30, model=m), fref.eval_co(co, ai, aw, ap, inc, np.full(inc.shape, 7.5), np.full(inc.shape, 30.0))["sigma0_db"])
    f32 = windspeed.simulate_sigma0(inc.astype(np.float32), wind=wind.astype(np.complex64), model=m)
    assert ref_engine[-1]["plan"].dtype == np.float32 and f32.dtype == np.float64
    # cross-pol: no direction, dphi None; wind= gives its modulus
    wcr = np.random.default_rng(2).uniform(awcr[0], awcr[-1], inc.shape)
    want_cr = fref.eval_cr(cr, ai, awcr, inc, wcr)
    jac = windspeed.simulate_sigma0(inc, wcr, model=mcr, jacobian=True)
    assert _bits_equal(jac.sigma0, want_cr["sigma0_db"]) and _bits_equal(jac.dwspd, want_cr["dwspd"]) and jac.dphi is None
    assert _bits_equal(windspeed.simulate_sigma0(inc, wind=wind, model=mcr), fref.eval_cr(cr, ai, awcr, inc, np.abs(wind))["sigma0_db"])
    # resolution passes through to to_lut
    windspeed.simulate_sigma0(inc, w, p, model=m, resolution="high")
    assert ref_engine[-1]["lut"] is m._lut(units="dB", resolution="high")


def test_simulate_sigma0_refusals(array_model, ref_engine, no_library, xr_env):
    (co, ai, aw, ap), (cr, _, awcr) = _tables("phi180")
    m = array_model("gmf_fwdtest_ref", co, ai, aw, ap)
    mcr = array_model("gmf_fwdtest_ref_cr", cr, ai, awcr, pol="VH")
    inc, w, p = _rasters(ai, aw, ap)
    wind = w * np.exp(1j * np.deg2rad(p))
    sim = windspeed.simulate_sigma0
    with pytest.raises(TypeError, match="xarray / dask"):
        sim(xr_env.xr.DataArray(inc, dims=("line", "sample")), w, p, model=m)
    with pytest.raises(ValueError, match="not both"):
        sim(inc, w, wind=wind, model=m)
    with pytest.raises(ValueError, match="not both"):
        sim(inc, phi=p, wind=wind, model=m)
    with pytest.raises(ValueError, match="give the wind"):
        sim(inc, model=m)
    with pytest.raises(ValueError, match="phi"):
        sim(inc, w, model=m)
    with pytest.raises(ValueError, match="takes no phi"):
        sim(inc, w, p, model=mcr)
    with pytest.raises(ValueError, match="one shape"):
        sim(inc, w[:, :3], p, model=m)
    with pytest.raises(ValueError, match="shape"):
        sim(inc, wind=wind[:2], model=m)
    with pytest.raises(ValueError, match="linear"):
        sim(inc, w, p, model=m, units="linear", jacobian=True)
    with pytest.raises(ValueError, match="Unit not known"):
        sim(inc, w, p, model=m, units="db")
    with pytest.raises(ValueError, match="out_dtype"):
        sim(inc, w, p, model=m, out_dtype=np.int32)
    with pytest.raises(TypeError, match="complex"):
        sim(inc, wind=w, model=m)
    with pytest.raises(KeyError):
        sim(inc, w, p, model="gmf_no_such_model")

    class DeviceArray:  # a device array by its interface; never dereferenced
        def __init__(self, a):
            self.__cuda_array_interface__ = dict(shape=a.shape, typestr=a.dtype.str, data=(0, False), version=3)

    with pytest.raises(ValueError, match="one container kind"):
        sim(inc, DeviceArray(w), p, model=m)
    with pytest.raises(ValueError, match="one container kind"):
        sim(inc, wind=DeviceArray(wind), model=m)
    with pytest.raises(ValueError, match="one container kind"):  # refused before the scalar is expanded on the device
        sim(DeviceArray(inc), 7.5, p, model=m)
    assert not ref_engine
    assert "simulate_sigma0" in windspeed.__all__ and windspeed.SimulatedSigma0 is forward.SimulatedSigma0


def test_pair_gathers_stay_8_byte_loads():
    """The table pairs co[i][w][p_lo .. p_lo + 1] / cr[i][w_lo .. w_lo + 1] are only 8-byte aligned: the built gfx950 code of every
    instantiation of the two kernels holds 8-byte global loads and no 16-byte one (csrc/xsw_forward.hpp: next_entry), no scratch
    and no LDS."""
    from xsarsea_amd import _build
    _build.build()
    kernels = _build.kernel_mnemonics("k_lut_eval_")
    assert len(kernels) == 8 and sum("k_lut_eval_co" in k for k in kernels) == 4, sorted(kernels)
    for name, ops in kernels.items():
        loads = {m: c for m, c in ops.items() if m.startswith("global_load")}
        print(name, loads)
        assert loads.get("global_load_dwordx2", 0) >= (8 if "k_lut_eval_co" in name else 4), (name, loads)
        assert not any(m.startswith(("global_load_dwordx3", "global_load_dwordx4")) for m in loads), (name, loads)
        assert not any(m.startswith(("scratch_", "ds_")) for m in ops), name
