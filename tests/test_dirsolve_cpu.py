"""CPU: wind direction at a known speed.  The numpy restatement tests/dirsolve_ref.py is held to the forward
restatement tests/forward_ref.py (its node values are that file's intermediate values bit for bit; every solution and every mirror
image round-trips through it), to the plain meaning of its count (sign changes of the forward interpolant on a dense direction
grid, a second function), and to hand-made tables where every answer is known; the Python layer (`retrieve_dir`, `retrieve_wind`)
is run with the engine's calls replaced by the restatements, and its refusals without the shared library."""
import importlib

import numpy as np
import pytest

import dirsolve_ref as dref
import forward_ref as fref
import solve_ref as sref
from conftest import golden
from test_forward_cpu import _bits_equal, array_model, no_library  # noqa: F401 (fixtures)
from util import small_luts

from xsarsea_amd import _lib, windspeed
from xsarsea_amd.windspeed import _engine

N_SCENE = 40000
ROUND_TRIP_DB = 1e-10  # what section 17's round trip allows


def _tables(name):
    if name == "nonuniform":
        return fref.nonuniform_tables()
    lco, lcr = small_luts(golden(f"kernel_small_{name}_f64.npz"))
    return (np.asarray(lco.values, dtype=np.float64), lco.incidence, lco.wspd, lco.phi), (np.asarray(lcr.values, dtype=np.float64), lcr.incidence, lcr.wspd)


@pytest.fixture(scope="module")
def default_co(default_luts):
    lco = default_luts[0]
    return np.asarray(lco.values, dtype=np.float64), lco.incidence, lco.wspd, lco.phi


def _scene(co, n, seed, noise=0.3, inc_range=None, w_range=None):
    """(inc, s, w, phi_true) inside the axes: s the restated forward value at a random true direction plus N(0, noise) dB."""
    table, ai, aw, ap = co
    rng = np.random.default_rng(seed)
    inc = rng.uniform(*(inc_range or (ai[0], ai[-1])), n)
    w = rng.uniform(*(w_range or (aw[0], aw[-1])), n)
    p = rng.uniform(ap[0], ap[-1], n)
    s = fref.eval_co(table, ai, aw, ap, inc, w, p, fold_phi=False)["sigma0_db"] + rng.normal(0.0, noise, n)
    return inc, s, w, p


# ------------------------------------------------------------------------------------------------ node values
def _check_node_values(co, seed, n=4000):
    """d(pl), d(ph) against forward_ref.eval_co's statements (incidence for the four corners, then speed: its u0, u1), and through
    its OUTPUTS: the direction lerp of d(pl), d(ph) is its sigma0_db and its slope is its dphi, bit for bit."""
    table, ai, aw, ap = co
    inc, w, p = fref.points(np.random.default_rng(seed), (ai, aw, ap), n, (0.0, 0.0, 0.0))
    ok = ~(np.isnan(inc) | np.isnan(w) | np.isnan(p))
    inc, w, p = inc[ok], w[ok], p[ok]
    D = dref.node_values(table, ai, aw, inc, w)
    il, ih, _ = fref._cell(ai, inc)
    wl, wh, _ = fref._cell(aw, w)
    pl, ph, _ = fref._cell(ap, p)
    v = [[fref._lerp(table[il, r, q], table[ih, r, q], ai[il], ai[ih], inc)[1] for q in (pl, ph)] for r in (wl, wh)]
    u0 = fref._lerp(v[0][0], v[1][0], aw[wl], aw[wh], w)[1]
    u1 = fref._lerp(v[0][1], v[1][1], aw[wl], aw[wh], w)[1]
    at = np.arange(len(inc))
    assert _bits_equal(D[at, pl], u0) and _bits_equal(D[at, ph], u1)
    sp, db = fref._lerp(D[at, pl], D[at, ph], ap[pl], ap[ph], p)
    want = fref.eval_co(table, ai, aw, ap, inc, w, p, fold_phi=False)
    assert np.isfinite(want["sigma0_db"]).all() and _bits_equal(db, want["sigma0_db"]) and _bits_equal(sp, want["dphi"])


def test_node_values_are_the_forward_intermediates_default_table(default_co):
    _check_node_values(default_co, 41)


@pytest.mark.parametrize("name", ["phi180", "phi360", "phi90", "nonuniform"])
def test_node_values_are_the_forward_intermediates_small_tables(name):
    _check_node_values(_tables(name)[0], 42, 1500)


# ------------------------------------------------------------------------------------------------ count, round trip, mirror
def _check_count_and_round_trip(co, inc, s, w, p_true, what):
    table, ai, aw, ap = co
    near = np.where(np.arange(len(inc)) % 2 == 0, p_true, -p_true)  # half of the references on the mirrored side
    fold = ap[-1] <= 180.0  # a table that goes on past 180 degrees holds its own mirror images, and a rough one is not symmetric
    signs = (1.0, -1.0) if fold else (1.0,)
    r = dref.solve(*co, inc, s, w, near=near, fold_phi=fold)
    D = dref.node_values(table, ai, aw, inc, w)
    assert not np.any(D == s[:, None]), "sigma0 off the node values"
    dense = dref.count_dense(*co, inc, s, w)
    differ = int(np.sum(dense != r["n"]))
    shares = {c: round(float((r["n"] == c).mean()), 4) for c in range(4)}
    print(f"{what}: count differs from the dense count on {differ} pixels; shares of count {shares}, BELOW {(r['flag'] == dref.BELOW).mean():.4f}, "
          f"ABOVE {(r['flag'] == dref.ABOVE).mean():.4f}")
    assert differ == 0
    assert np.array_equal(r["count"], np.minimum(r["n"], 255)) and np.array_equal(r["flag"] == dref.MORE, r["n"] > 2)
    assert np.array_equal((r["flag"] & 7) != 0, r["n"] == 0) and not np.any(r["flag"] == dref.NAN)
    worst = 0.0
    for name, have in (("phi1", r["n"] >= 1), ("phi2", r["n"] >= 2), ("phi_near", r["n"] >= 1)):
        assert np.array_equal(np.isfinite(r[name]), have)
        for sign in signs:  # the solution and its mirror image, folded back by the forward restatement
            back = fref.eval_co(*co, inc[have], w[have], sign * r[name][have], fold_phi=True)["sigma0_db"]
            worst = max(worst, float(np.abs(back - s[have]).max())) if have.any() else worst
    print(f"{what}: round trip through forward_ref, solutions and mirror images: {worst:.3g} dB")
    assert worst <= ROUND_TRIP_DB
    # the selection: no candidate is nearer to the reference than the one chosen (among the two stored, where there are at most two)
    two = (r["n"] >= 1) & (r["n"] <= 2)
    chosen = dref.distance(r["phi_near"], near)
    for name in ("phi1", "phi2"):
        for sign in signs:
            with np.errstate(invalid="ignore"):
                assert not np.any(two & (dref.distance(sign * r[name], near) < chosen))
    # BELOW / ABOVE: the closest node is the column's arg-min / arg-max node
    below, above = r["flag"] == dref.BELOW, r["flag"] == dref.ABOVE
    assert np.array_equal(r["phi_closest"][below], ap[D[below].argmin(axis=1)]) and np.array_equal(r["phi_closest"][above], ap[D[above].argmax(axis=1)])
    assert np.isfinite(r["phi_closest"]).all()
    return r, shares


def test_count_round_trip_mirror_default_table(default_co):
    """The issue's own scene: incidence 18..46 degrees, 1..30 m/s, 0.3 dB of noise; every class of the answer is populated."""
    inc, s, w, p = _scene(default_co, N_SCENE, 61, inc_range=(18.0, 46.0), w_range=(1.0, 30.0))
    r, shares = _check_count_and_round_trip(default_co, inc, s, w, p, "default table")
    assert shares[2] > 0.5 and shares[1] > 0.05 and (r["flag"] == dref.BELOW).mean() > 0.03 and (r["flag"] == dref.ABOVE).mean() > 0.03
    assert shares[3] == 0 and r["n"].max() == 2  # CMOD5.N: never three


@pytest.mark.parametrize("name", ["phi180", "phi360", "phi90", "nonuniform"])
def test_count_round_trip_mirror_small_tables(name):
    co = _tables(name)[0]
    inc, s, w, p = _scene(co, 3000, 62)
    r, _ = _check_count_and_round_trip(co, inc, s, w, p, name)
    assert (r["n"] >= 1).any()
    assert (name == "phi360") == (co[3][-1] > 180.0)


# ------------------------------------------------------------------------------------------------ edge rules
def _one(t, s, inc=20.0, w=2.0, near=None, fold_phi=True):
    r = dref.solve(*t, np.array([inc]), np.array([s]), np.array([w]), near=None if near is None else np.array([near]), fold_phi=fold_phi)
    return {k: v[0] for k, v in r.items()}


def _columns_on_their_own_nodes(co, inc, w):
    """Every pixel's column with sigma0 on each of its node values in turn: n against the independent statement `strict crossings
    + nodes that equal s` (no two neighbouring nodes of these columns are equal, so no flat run is among them)."""
    table, ai, aw, ap = co
    D = dref.node_values(table, ai, aw, inc, w)
    assert not np.any(D[:, 1:] == D[:, :-1])
    n_phi = D.shape[1]
    inc2, w2 = (np.repeat(a[:, None], n_phi, axis=1) for a in (inc, w))
    r = dref.solve(*co, inc2, D, w2)
    x = D[:, None, :]                                           # [pixel][j of s][node]
    strict = ((D[:, None, :-1] - x.transpose(0, 2, 1)) * (D[:, None, 1:] - x.transpose(0, 2, 1)) < 0).sum(axis=2)
    touching = (D[:, None, :] == x.transpose(0, 2, 1)).sum(axis=2)
    assert np.array_equal(r["n"], strict + touching) and (r["n"] >= 1).all()
    return r


def test_sigma0_on_every_node_value_is_counted_once(default_co):
    rng = np.random.default_rng(5)
    r = _columns_on_their_own_nodes(default_co, rng.uniform(18.0, 46.0, 12), rng.uniform(1.0, 30.0, 12))
    assert set(np.unique(r["n"])) == {1, 2}  # (1: the column's extremes)
    for name in ("phi180", "phi360", "phi90", "nonuniform"):
        co = _tables(name)[0]
        _columns_on_their_own_nodes(co, rng.uniform(co[1][0], co[1][-1], 8), rng.uniform(co[2][0], co[2][-1], 8))
    # the wavy column: s on its minima (nodes 1, 3) touches twice, each counted once, by the cell ABOVE the node
    g = _one(dref.wavy_table(), -14.0)
    assert (g["n"], g["phi1"], g["phi2"], g["flag"]) == (2, 30.0, 90.0, 0)
    g = _one(dref.wavy_table(), -10.0)  # nodes 0, 2, 4: node 0 by cell 0, node 2 by cell 2, node 4 by cell 4 (which rises past it)
    assert (g["n"], g["phi1"], g["phi2"], g["flag"]) == (3, 0.0, 60.0, dref.MORE)


def test_hand_made_tables():
    nan, inf = float("nan"), float("inf")
    # four crossings: MORE, the first two stored; between the nodes of incidence and speed the column is row + 3
    t = dref.wavy_table()
    g = _one(t, -12.0)
    assert (g["phi1"], g["phi2"], g["sens1"], g["sens2"], g["count"], g["flag"]) == (15.0, 45.0, -7.5, 7.5, 4, dref.MORE)
    g = _one(t, -9.0, inc=22.0, w=4.0)
    assert (g["phi1"], g["phi2"], g["count"], g["flag"]) == (15.0, 45.0, 4, dref.MORE)
    g = _one(t, -8.0)  # the last node: counted by the last cell
    assert (g["phi1"], g["count"], g["flag"]) == (180.0, 1, 0) and np.isnan(g["phi2"]) and np.isnan(g["sens2"])
    g = _one(t, -7.5)
    assert (g["count"], g["flag"], g["phi_closest"]) == (0, dref.ABOVE, 180.0) and all(np.isnan(g[k]) for k in ("phi1", "phi2", "sens1", "sens2"))
    g = _one(t, -14.5)
    assert (g["count"], g["flag"], g["phi_closest"]) == (0, dref.BELOW, 30.0)  # the FIRST of the two minima
    # the saturating count
    g = _one(dref.zigzag_table(301), -12.0)
    assert (g["n"], g["count"], g["flag"]) == (300, 255, dref.MORE) and abs(g["phi1"] - 0.3) < 1e-12 and abs(g["phi2"] - 0.9) < 1e-12  # (cells of 0.6 degrees)
    g = _one(dref.zigzag_table(257), -12.0)
    assert (g["n"], g["count"]) == (256, 255)
    g = _one(dref.zigzag_table(256), -12.0)
    assert (g["n"], g["count"]) == (255, 255)
    # flat runs at s: once, at the end of the run; the run that ends on the last node in the last cell, which is flat
    g = _one(dref.flat_table(), -12.0)
    assert (g["phi1"], g["sens1"], g["phi2"], g["sens2"], g["count"], g["flag"]) == (90.0, -10.0, 150.0, inf, 2, 0)
    assert g["phi_closest"] == 30.0  # the first node of the first run
    # NaN nodes: the cells on either side hold nothing, not even s on the last node behind a NaN
    t = dref.nan_table()
    g = _one(t, -12.0)
    assert (g["phi1"], g["sens1"], g["count"], g["flag"], g["phi_closest"]) == (90.0, 9.0, 1, 0, 180.0) and np.isnan(g["phi2"])
    g = _one(t, -15.0)
    assert (g["count"], g["flag"], g["phi_closest"]) == (0, dref.BELOW, 72.0)
    first_nan = dref._table([nan, -10.0, -9.0])
    g = _one(first_nan, -12.0)
    assert (g["count"], g["flag"], g["phi_closest"]) == (0, dref.NAN, 90.0) and np.isnan(g["phi1"])  # neither below nor above a NaN d(0)
    all_nan = dref._table([nan, nan, nan])
    g = _one(all_nan, -12.0)
    assert (g["count"], g["flag"]) == (0, dref.NAN) and np.isnan(g["phi_closest"])
    # a monotone column on a non-uniform axis: one solution or none
    t = dref.monotone_table()
    g = _one(t, -10.0)
    assert (g["phi1"], g["sens1"], g["count"], g["flag"]) == (35.0, -15.0, 1, 0) and np.isnan(g["phi2"])
    assert _one(t, -8.0)["phi1"] == 0.0 and _one(t, -16.0)["phi1"] == 180.0 and _one(t, -16.0)["count"] == 1
    assert _one(t, -7.0)["flag"] == dref.ABOVE and _one(t, -7.0)["phi_closest"] == 0.0
    assert _one(t, -17.0)["flag"] == dref.BELOW and _one(t, -17.0)["phi_closest"] == 180.0
    # the gate
    for inc, s, w in ((nan, -10.0, 2.0), (20.0, nan, 2.0), (20.0, -10.0, nan), (19.5, -10.0, 2.0), (24.5, -10.0, 2.0), (20.0, -10.0, 1.5),
                      (20.0, -10.0, 6.5), (20.0, inf, 2.0), (20.0, -inf, 2.0)):
        g = _one(t, s, inc=inc, w=w, near=10.0)
        assert (g["count"], g["flag"]) == (0, dref.NAN) and all(np.isnan(g[k]) for k in dref.REALS), (inc, s, w)


def test_selection_rules():
    """The wavy column at s = -12: solutions 15, 45, 75, 105 with sens -7.5, 7.5, -7.5, 7.5; candidates in scan order +15, -15, +45, ..."""
    t = dref.wavy_table()
    sel = lambda near, **kw: tuple(_one(t, -12.0, near=near, **kw)[k] for k in ("phi_near", "sens_near"))
    assert sel(100.0) == (105.0, 7.5)        # the FOURTH solution: the selection runs over all of them, not only the two stored
    assert sel(70.0) == (75.0, -7.5)
    assert sel(30.0) == (15.0, -7.5)         # a tie between 15 and 45: the earlier one
    assert sel(0.0) == (15.0, -7.5)          # a tie between +15 and its mirror image: +15 comes first
    assert sel(-30.0) == (-15.0, 7.5)        # a tie between -15 and -45; the sensitivity of a mirror image is negated
    assert sel(-100.0) == (-105.0, -7.5)
    assert sel(200.0) == (-105.0, -7.5)      # 200 is -160: 55 degrees from -105, 95 from +105
    assert sel(180.0) == (105.0, 7.5)        # a tie between +105 and -105
    assert sel(-30.0, fold_phi=False) == (15.0, -7.5) and sel(200.0, fold_phi=False) == (105.0, 7.5)
    for near in (100.0, 30.0, -30.0, 0.0, 200.0):
        assert sel(near + 360.0) == sel(near) == sel(near - 360.0) == sel(near + 720.0)
    for near in (float("nan"), float("inf")):
        g = _one(t, -12.0, near=near)
        assert np.isnan(g["phi_near"]) and np.isnan(g["sens_near"]) and g["count"] == 4 and g["phi1"] == 15.0
    g = _one(t, -7.5, near=10.0)  # no solution: nothing to select
    assert np.isnan(g["phi_near"]) and np.isnan(g["sens_near"])
    assert np.isnan(_one(t, -12.0)["phi_near"])  # no reference given
    assert np.array_equal(dref.distance(np.array([10.0, 350.0, -170.0, 190.0, 370.0]), 0.0), [10.0, 10.0, 170.0, 170.0, 10.0])


# ------------------------------------------------------------------------------------------------ the Python layer, no device
@pytest.fixture
def ref_engine(monkeypatch):
    """`_engine.dir_solve` and `_engine.wspd_solve_cr` replaced by the restatements on the LUT object they are handed; records the calls."""
    calls = []
    names = dict(zip(_engine.DIR_REALS + _engine.DIR_BYTES, dref.FIELDS))

    def dir_solve(lut, plan, inc, sigma0_db, wspd, near=None, fold_phi=True, outputs=("phi1", "phi2"), out_dtype=np.float64):
        calls.append(dict(kind="dir", lut=lut, plan=plan, near=near, fold_phi=fold_phi, outputs=tuple(outputs), out_dtype=out_dtype, sigma0_db=sigma0_db, wspd=wspd))
        r = dref.solve(lut.values, lut.incidence, lut.wspd, lut.phi, inc, sigma0_db, wspd, near=near, fold_phi=fold_phi)
        with np.errstate(all="ignore"):
            return {k: (r[names[k]] if k in _engine.DIR_BYTES else r[names[k]].astype(out_dtype)) for k in outputs}

    def wspd_solve_cr(lut, plan, inc, sigma0_db, details=False, out_dtype=np.float64):
        calls.append(dict(kind="cr", lut=lut, plan=plan, sigma0_db=sigma0_db, out_dtype=out_dtype))
        r = sref.solve_cr(lut.values, lut.incidence, lut.wspd, inc, sigma0_db)
        return [r["wspd"].astype(out_dtype)] + ([r["sens"].astype(out_dtype), r["flag"]] if details else [])

    monkeypatch.setattr(_engine, "dir_solve", dir_solve)
    monkeypatch.setattr(_engine, "wspd_solve_cr", wspd_solve_cr)
    return calls


def _rasters(co, shape=(5, 7), seed=8):
    inc, s, w, p = _scene(co, int(np.prod(shape)), seed)
    return tuple(a.reshape(shape) for a in (inc, s, w, p))


def test_retrieve_dir(array_model, ref_engine, no_library):
    co, cr = _tables("phi180")
    m = array_model("gmf_dirtest", *co)
    inc, s_db, w, p = _rasters(co)
    want = dref.solve(*co, inc, s_db, w, near=p)
    pair = windspeed.retrieve_dir(inc, s_db, w, model="gmf_dirtest", units="dB")
    assert isinstance(pair, tuple) and _bits_equal(pair[0], want["phi1"]) and _bits_equal(pair[1], want["phi2"]) and np.isfinite(pair[0]).any()
    c = ref_engine[-1]
    assert c["outputs"] == ("phi1", "phi2") and c["near"] is None and c["fold_phi"] is True and c["out_dtype"] == np.float64
    assert c["lut"] is m._lut(units="dB") and c["sigma0_db"] is s_db and c["wspd"] is w and c["plan"].dtype == np.float64 and c["plan"].shape == inc.shape
    got = windspeed.retrieve_dir(inc, s_db, w, near=p, model=m, units="dB")
    assert isinstance(got, np.ndarray) and _bits_equal(got, want["phi_near"]) and ref_engine[-1]["outputs"] == ("phi_near",) and ref_engine[-1]["near"] is p
    # units: linear by default, 10 log10(sigma0 + 1e-15) in sigma0's own dtype
    lin = 10 ** (s_db / 10)
    got = windspeed.retrieve_dir(inc, lin, w, near=p, model=m)
    assert np.array_equal(ref_engine[-1]["sigma0_db"], 10 * np.log10(lin + 1e-15))
    assert _bits_equal(got, dref.solve(*co, inc, 10 * np.log10(lin + 1e-15), w, near=p)["phi_near"])
    f32 = [a.astype(np.float32) for a in (inc, lin, w, p)]
    windspeed.retrieve_dir(f32[0], f32[1], f32[2], near=f32[3], model=m)
    assert ref_engine[-1]["sigma0_db"].dtype == np.float32 and ref_engine[-1]["plan"].dtype == np.float32
    windspeed.retrieve_dir(f32[0], f32[1], w, near=f32[3], model=m)  # one float64 raster: the call computes in float64
    assert ref_engine[-1]["plan"].dtype == np.float64
    # details, with and without a reference; out_dtype; fold_phi
    r = windspeed.retrieve_dir(inc, s_db, w, near=p, model=m, units="dB", details=True, out_dtype=np.float32)
    assert isinstance(r, windspeed.RetrievedDir) and r["phi1"] is r.phi1 and r.phi1.dtype == np.float32 and r.count.dtype == np.uint8 and r.flag.dtype == np.uint8
    with np.errstate(all="ignore"):
        for mine, theirs in zip(windspeed.RetrievedDir.FIELDS, dref.FIELDS):
            assert np.array_equal(r[mine], want[theirs]) if theirs in ("count", "flag") else _bits_equal(r[mine], want[theirs].astype(np.float32)), mine
    r = windspeed.retrieve_dir(inc, s_db, w, model=m, units="dB", details=True)
    assert r.phi_near is None and r.dphi_near_dsigma0 is None and _bits_equal(r.phi_closest, want["phi_closest"]) and np.array_equal(r.count, want["count"])
    assert "phi_near" not in ref_engine[-1]["outputs"] and "sens_near" not in ref_engine[-1]["outputs"] and len(ref_engine[-1]["outputs"]) == 7
    windspeed.retrieve_dir(inc, s_db, w, near=-p, model=m, units="dB", fold_phi=False)
    assert ref_engine[-1]["fold_phi"] is False
    # scalars are expanded; wind=: the angle alone, by the array module
    assert _bits_equal(windspeed.retrieve_dir(inc, s_db, 7, near=30, model=m, units="dB"),
                       dref.solve(*co, inc, s_db, np.full(inc.shape, 7.0), near=np.full(inc.shape, 30.0))["phi_near"])
    wind = 7.0 * np.exp(1j * np.deg2rad(p - 90.0))
    got = windspeed.retrieve_dir(inc, s_db, w, wind=wind, model=m, units="dB")
    assert np.array_equal(ref_engine[-1]["near"], np.degrees(np.angle(wind)))
    assert _bits_equal(got, dref.solve(*co, inc, s_db, w, near=np.degrees(np.angle(wind)))["phi_near"])
    windspeed.retrieve_dir(inc, s_db, w, model=m, units="dB", resolution="high")
    assert ref_engine[-1]["lut"] is m._lut(units="dB", resolution="high")
    assert {"retrieve_dir", "RetrievedDir", "retrieve_wind"} <= set(windspeed.__all__) and windspeed.RetrievedDir is importlib.import_module("xsarsea_amd.windspeed.retrieve_dir").RetrievedDir
    assert (_lib.DIR_NAN, _lib.DIR_BELOW, _lib.DIR_ABOVE, _lib.DIR_MORE) == (dref.NAN, dref.BELOW, dref.ABOVE, dref.MORE)


def test_retrieve_wind(array_model, ref_engine, no_library):
    """The composition of the two restatements: speed from the cross-pol table, direction from the co-pol table at that speed."""
    co, cr = _tables("phi180")
    m, mcr = array_model("gmf_windtest", *co), array_model("gmf_windtest_cr", *cr, pol="VH")
    inc, s_co, w, p = _rasters(co, (6, 9), 9)
    rng = np.random.default_rng(3)
    s_cr = fref.eval_cr(*cr, inc, w)["sigma0_db"] + rng.normal(0.0, 0.1, inc.shape)
    s_cr[0, :3] = (np.nan, 40.0, -90.0)  # no speed: NaN, above, below the cross-pol table
    near = np.where(rng.random(inc.shape) < 0.5, p, -p)
    near[1, 0] = np.nan
    speed = sref.solve_cr(*cr, inc, s_cr)["wspd"]
    phi = dref.solve(*co, inc, s_co, speed, near=near)["phi_near"]
    want = speed * np.exp(1j * np.radians(phi))
    got = windspeed.retrieve_wind(inc, s_co, s_cr, near=near, model=(m, "gmf_windtest_cr"), units="dB")
    assert got.dtype == np.complex128 and _bits_equal(got.real, want.real) and _bits_equal(got.imag, want.imag)
    assert [c["kind"] for c in ref_engine[-2:]] == ["cr", "dir"] and ref_engine[-1]["lut"] is m._lut(units="dB") and ref_engine[-2]["lut"] is mcr._lut(units="dB")
    assert np.isnan(got[0, :3]).all() and np.isnan(got[1, 0]) and np.isfinite(got).mean() > 0.3
    assert np.array_equal(np.isnan(got), np.isnan(speed) | np.isnan(phi))
    ok = np.isfinite(got)
    assert np.allclose(np.abs(got[ok]), speed[ok], rtol=1e-15) and np.abs(fref.eval_co(*co, inc[ok], np.abs(got[ok]), np.degrees(np.angle(got[ok])))["sigma0_db"] - s_co[ok]).max() < 1e-9
    # wind=, linear units, complex64 out
    wind = 3.0 * np.exp(1j * np.radians(np.nan_to_num(near, nan=5.0)))
    ang = np.degrees(np.angle(wind))
    got = windspeed.retrieve_wind(inc, s_co, s_cr, wind=wind, model=(m, mcr), units="dB")
    want = speed * np.exp(1j * np.radians(dref.solve(*co, inc, s_co, speed, near=ang)["phi_near"]))
    assert _bits_equal(got.real, want.real) and _bits_equal(got.imag, want.imag)
    lin_co, lin_cr = 10 ** (s_co / 10), 10 ** (np.nan_to_num(s_cr, nan=-20.0) / 10)
    got = windspeed.retrieve_wind(inc, lin_co, lin_cr, near=near, model=(m, mcr), out_dtype=np.float32)
    sp = sref.solve_cr(*cr, inc, 10 * np.log10(lin_cr + 1e-15))["wspd"]
    want = (sp * np.exp(1j * np.radians(dref.solve(*co, inc, 10 * np.log10(lin_co + 1e-15), sp, near=near)["phi_near"]))).astype(np.complex64)
    assert got.dtype == np.complex64 and _bits_equal(got.real.astype(np.float64), want.real.astype(np.float64)) and _bits_equal(got.imag.astype(np.float64), want.imag.astype(np.float64))


def test_refusals(array_model, ref_engine, no_library, xr_env):
    co, cr = _tables("phi180")
    m, mcr = array_model("gmf_dirtest_ref", *co), array_model("gmf_dirtest_ref_cr", *cr, pol="VH")
    inc, s, w, p = _rasters(co)
    wind = 7.0 * np.exp(1j * np.deg2rad(p))
    xa = lambda a: xr_env.xr.DataArray(a, dims=("line", "sample"))

    class DeviceArray:  # a device array by its interface; never dereferenced
        def __init__(self, a):
            self.__cuda_array_interface__ = dict(shape=a.shape, typestr=a.dtype.str, data=(0, False), version=3)

    ret = windspeed.retrieve_dir
    for args, kw in (((xa(inc), s, w), {}), ((inc, s, xa(w)), {}), ((inc, s, w), dict(near=xa(p))), ((inc, s, w), dict(wind=xa(wind)))):
        with pytest.raises(TypeError, match="xarray / dask"):
            ret(*args, model=m, **kw)
    with pytest.raises(ValueError, match="not both"):
        ret(inc, s, w, near=p, wind=wind, model=m)
    with pytest.raises(ValueError, match="cross-pol model"):
        ret(inc, s, w, model=mcr)
    with pytest.raises(ValueError, match="cross-pol model"):
        ret(inc, s, w, near=p, model=mcr)
    with pytest.raises(ValueError, match="one shape"):
        ret(inc, s[:, :3], w, model=m)
    with pytest.raises(ValueError, match="one shape"):
        ret(inc, s, w[:2], model=m)
    with pytest.raises(ValueError, match="inc, sigma0, wspd, near must have one shape"):
        ret(inc, s, w, near=p[:2], model=m)
    with pytest.raises(ValueError, match="shape"):
        ret(inc, s, w, wind=wind[:2], model=m)
    with pytest.raises(ValueError, match="Unit not known"):
        ret(inc, s, w, model=m, units="db")
    with pytest.raises(ValueError, match="out_dtype"):
        ret(inc, s, w, model=m, out_dtype=np.int32)
    with pytest.raises(TypeError, match="complex"):
        ret(inc, s, w, wind=p, model=m)
    with pytest.raises(TypeError, match="float32 or float64"):
        ret(inc, s, w.astype(np.int32), model=m)
    with pytest.raises(TypeError, match="sigma0 must be"):
        ret(inc, 0.01, w, model=m)
    with pytest.raises(TypeError, match="inc must be"):
        ret(30.0, s, w, model=m)
    with pytest.raises(KeyError):
        ret(inc, s, w, model="gmf_no_such_model")
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, DeviceArray(s), w, model=m)
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, s, DeviceArray(w), model=m)
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, s, w, near=DeviceArray(p), model=m)
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, s, w, wind=DeviceArray(wind), model=m)
    with pytest.raises(ValueError, match="one container kind"):  # refused before a scalar is expanded, or sigma0 converted, on the device
        ret(DeviceArray(inc), s, 7.0, near=30.0, model=m)

    ret = windspeed.retrieve_wind
    with pytest.raises(ValueError, match="one of near= and wind="):
        ret(inc, s, s, model=(m, mcr))
    with pytest.raises(ValueError, match="one of near= and wind="):
        ret(inc, s, s, near=p, wind=wind, model=(m, mcr))
    for bad in (None, m, "gmf_dirtest_ref", (m,), (m, mcr, m)):
        with pytest.raises(ValueError, match=r"model=\(co-pol model, cross-pol model\)"):
            ret(inc, s, s, near=p, model=bad)
    for bad in ((mcr, m), (m, m), (mcr, mcr)):
        with pytest.raises(ValueError, match=r"model=\(co-pol model, cross-pol model\), not"):
            ret(inc, s, s, near=p, model=bad)
    with pytest.raises(KeyError):
        ret(inc, s, s, near=p, model=(m, "gmf_no_such_model"))
    with pytest.raises(TypeError, match="xarray / dask"):
        ret(inc, s, xa(s), near=p, model=(m, mcr))
    with pytest.raises(ValueError, match="Unit not known"):
        ret(inc, s, s, near=p, model=(m, mcr), units="db")
    with pytest.raises(ValueError, match="out_dtype"):
        ret(inc, s, s, near=p, model=(m, mcr), out_dtype=np.complex128)
    with pytest.raises(ValueError, match="one shape"):
        ret(inc, s, s[:2], near=p, model=(m, mcr))
    with pytest.raises(ValueError, match="one shape"):
        ret(inc, s, s, near=p[:, :2], model=(m, mcr))
    with pytest.raises(ValueError, match="shape"):
        ret(inc, s, s, wind=wind[:2], model=(m, mcr))
    with pytest.raises(TypeError, match="sigma0_cr must be"):
        ret(inc, s, 0.001, near=p, model=(m, mcr))
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, s, DeviceArray(s), near=p, model=(m, mcr))
    with pytest.raises(ValueError, match="one container kind"):
        ret(inc, s, s, wind=DeviceArray(wind), model=(m, mcr))
    assert not ref_engine


def test_kernel_walks_aligned_pairs_without_scratch():
    """The built gfx950 code of the four instantiations: the rows are walked as 16-byte loads (rows are 32-byte aligned and the walk
    starts at entry 0), and the kernel holds no scratch and no LDS access; the committed resources file says the same."""
    import os
    from xsarsea_amd import _build
    _build.build()
    kernels = _build.kernel_mnemonics("k_dir_solve_co")
    assert len(kernels) == 4, sorted(kernels)
    for name, ops in kernels.items():
        loads = {k: c for k, c in ops.items() if k.startswith("global_load")}
        print(name, loads)
        assert loads.get("global_load_dwordx4", 0) >= 4, (name, loads)
        assert not any(k.startswith(("scratch_", "ds_")) for k in ops), name
    res = [r for r in _build.kernel_resources() if "k_dir_solve_co" in r["kernel"]]
    assert len(res) == 4 and all(r["scratch_bytes"] == 0 and r["lds_bytes"] == 0 for r in res)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dirsolve_kernel_resources.tsv")) as f:
        rows = [ln.split("\t") for ln in f.read().splitlines() if ln and not ln.startswith("#")][1:]
    assert len(rows) == 4 and all(r[3] == "0" and r[4] == "0" for r in rows)
