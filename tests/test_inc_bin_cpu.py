"""CPU: the incidence bin (`nearest_index`, csrc/xsw_device.hpp) restated in tests/inc_bin_ref.py, held to the specification
`np.argmin(np.abs(inc_dim - inc))` and to the C oracle on the probes of tests/inc_bin_cases.py; the counts that keep those probes
honest; the tables in which a slice names itself; the host's uniform-axis verdict and bin arithmetic, asked of the compiled
csrc/xsw_lutplan.hpp; and the order a descending incidence axis is given before its install."""
import numpy as np
import pytest

import inc_bin_cases as ic
import inc_bin_ref as ibr
from test_host_lutplan import ask, hexv, same_bits  # noqa: F401 (fixture)

DTYPES = {"f64": np.float64, "f32": np.float32}


def all_axes():
    """Every incidence axis an install of tests/inc_bin_cases.py holds: {label: (axis, thinned probes)}."""
    out = {}
    for name in ic.SETS:
        co, cr = ic.set_axes(name)
        out[name + "/co"], out[name + "/cr"] = (co, name == "long"), (cr, name == "long")
    return out


def every_probe(ax, thin):
    """Float64 and float32 probes of one axis as float64, NaN left out."""
    p32 = np.concatenate([ic.probes32(ax, thin)[c] for c in ic.CLASSES32]).astype(np.float64)
    return np.concatenate([ic.flat_probes(ax, thin), p32[~np.isnan(p32)]])


@pytest.mark.parametrize("label", list(all_axes()))
def test_restatement_is_argmin_on_both_paths(label):
    ax, thin = all_axes()[label]
    xs = every_probe(ax, thin)
    want = ibr.argmin_indices(ax, xs)
    got, fell = ibr.nearest_indices(ax, xs, "host")
    assert np.array_equal(got, want), (label, "host path", xs[got != want][:5])
    got, _ = ibr.nearest_indices(ax, xs, "bisect")
    assert np.array_equal(got, want), (label, "bisection", xs[got != want][:5])
    if ax.size >= 2:  # the walk on any axis: wherever it starts and whether or not it settles, the invariant decides
        got, fell_forced = ibr.nearest_indices(ax, xs, "uniform")
        assert np.array_equal(got, want), (label, "uniform path forced", xs[got != want][:5])
        if ibr.uniform_axis(ax):
            assert not fell.any() and not fell_forced.any(), (label, "the walk fell through to the bisection", xs[fell | fell_forced][:5])
    assert np.array_equal(ibr.nearest_indices(ax, [np.inf, -np.inf])[0], [0, 0])


def test_uniform_verdict_and_bin_arithmetic_are_the_headers(ask):  # noqa: F811
    """uniform_axis, inc0 / inv_incstep (co_scalars) and inc_cr0 / inv_inccrstep (cr_scalars) of csrc/xsw_lutplan.hpp on every axis."""
    axes = all_axes()
    w, phi = hexv(ic.W_AX[:4]), hexv(ic.PHI_AX[:4])
    got_ax = ask(*["axis " + hexv(ax) for ax, _ in axes.values()])
    got_co = ask(*["coscal 1 1 %s %s %s" % (hexv(ax), w, phi) for ax, _ in axes.values()])
    got_cr = ask(*["cr %s %s %s" % (hexv(ax), hexv(ic.WCR_AX[:3]), hexv(np.zeros((ax.size, 3)))) for ax, _ in axes.values()])
    for (label, (ax, _)), g_ax, g_co, g_cr in zip(axes.items(), got_ax, got_co, got_cr):
        uniform = ibr.uniform_axis(ax)
        x0, inv_step = ibr.plan(ax)
        assert g_ax[:2] == [1, int(uniform)], label
        assert g_co[18] == int(uniform) and same_bits(g_co[26:28], [x0, inv_step]), (label, g_co[18], g_co[26:28])
        assert g_cr[5] == int(uniform) and same_bits(g_cr[9:11], [x0, inv_step]), (label, g_cr[5], g_cr[9:11])
    for name, (co, cr, _) in ic.SETS.items():
        assert ibr.uniform_axis(ic.set_axes(name)[0]) == (co in ic.UNIFORM) and ibr.uniform_axis(ic.set_axes(name)[1]) == (cr in ic.UNIFORM), name
    f32 = ic.AXES["float32_stored"]
    assert not ibr.uniform_axis(f32) and np.max(np.abs(f32 - ic.AXES["default"])) < 2e-6  # looks uniform; off by up to 2e-6 degree
    assert ibr.plan(ic.AXES["one"]) == (33.0, 0.0)


def test_probe_counts():
    """What keeps the probe set honest: exact ties, and probes on which a rounded bin is not the arg-min."""
    ax = ic.AXES["default"]
    mids = ic.probes(ax)["mid"]
    ties = int(np.sum(np.abs(ax[:-1] - mids) == np.abs(ax[1:] - mids)))
    assert ties >= 150, ties
    b = ic.AXES["binary"]
    mb = ic.probes(b)["mid"]
    assert np.all(np.abs(b[:-1] - mb) == np.abs(b[1:] - mb))
    nu = ic.AXES["nonuniform"]
    mn = ic.probes(nu)["mid"]
    assert np.all(np.abs(nu[:-1] - mn) == np.abs(nu[1:] - mn)) and np.all(mn == [0.5 * (lo + hi) for lo, hi in zip(nu[:-1], nu[1:])])
    xs = ic.flat_probes(ax)
    assert xs.size == 3 * 331 + 3 * 330 + 6
    want = ibr.argmin_indices(ax, xs)
    x0, inv_step = ibr.plan(ax)
    with np.errstate(all="ignore"):
        g = (xs - x0) * inv_step
        rint = np.clip(np.rint(g), 0, ax.size - 1).astype(np.int64)
        floor = np.clip(np.floor(g + 0.5), 0, ax.size - 1).astype(np.int64)
    n_rint, n_floor = int(np.sum(rint != want)), int(np.sum(floor != want))
    print(f"default: {ties} exact ties among 330 midpoints; of {xs.size} probes rint differs on {n_rint}, floor(. + 0.5) on {n_floor}")
    assert n_rint >= 100 and n_floor >= 100, (n_rint, n_floor)
    # ... among the float32 values on the 0.05 degree grid too (17.25, 17.75, ... are exact in float32 and midway between two nodes)
    x32 = ic.probes32(ax)["grid"].astype(np.float64)
    with np.errstate(all="ignore"):
        r32 = np.clip(np.rint((x32 - x0) * inv_step), 0, ax.size - 1).astype(np.int64)
    assert x32.size >= 660 and int(np.sum(r32 != ibr.argmin_indices(ax, x32))) >= 20
    for name in ic.SETS:
        sizes = {tag: int(np.sum(~np.isnan(ic.build_raster(name, dt)["inc"]))) for tag, dt in DTYPES.items()}
        print(f"{name}: probes per raster (NaN ones left out) {sizes}")
    assert int(np.sum(~np.isnan(ic.build_raster("default", np.float64)["inc"]))) == 1989 + (3 * 34 + 3 * 33 + 6)


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("name", list(ic.SETS))
def test_tables_name_their_slice(name, tag):
    """Every probe's answer, in every kernel, differs from what slice i - 1 and slice i + 1 would give; and the co-pol and cross-pol
    bins of one probe differ on at least a third of the probes, so that swapping them shows."""
    ic.assert_self_identifying(name, DTYPES[tag])
    c = ic.case(name, DTYPES[tag])
    live = c["i_inc"] >= 0
    assert np.array_equal(live, ~np.isnan(c["sc"]["inc"])) and live.sum() >= 20
    assert np.mean(c["i_inc"][live] != c["i_inc_cr"][live]) >= 1.0 / 3.0
    if tag == "f64":  # the +-inf probes answer from slice 0 of both tables
        inf = np.isinf(c["sc"]["inc"])
        assert inf.sum() == 4 and np.all(c["i_inc"][inf] == 0) and np.all(c["i_inc_cr"][inf] == 0) and np.all(c["o_idx"][inf] >= 0)
    nan_row = ~live
    assert np.all(c["o_idx"][nan_row] == -1) and np.all(np.isnan(c["o_co"][nan_row].real)) and np.all(c["o_co"][nan_row].imag == 0)  # windspeed.py:198-201


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("name", list(ic.SETS))
def test_c_oracle_takes_the_restatements_bin(name, tag):
    """oracle/invert_c.c's nearest_index through oracle.cport: the winning co-pol speed row is 6 + i_inc % 16 on these tables (the
    sigma0 term outweighs everything else by two orders of magnitude), which with the test above names the slice; the whole index
    triple equals the numpy oracle's, so the cross-pol bin is numpy's arg-min too."""
    from oracle import cport
    c = ic.case(name, DTYPES[tag])
    lco, lcr = c["lco"], c["lcr"]
    co_ax, cr_ax = ic.set_axes(name)
    shape = c["sc"]["inc"].shape
    i_co = ibr.nearest_indices(co_ax, c["sc"]["inc"])[0].reshape(shape)
    i_cr = ibr.nearest_indices(cr_ax, c["sc"]["inc"])[0].reshape(shape)
    assert np.array_equal(i_co, c["i_inc"]) and np.array_equal(i_cr, c["i_inc_cr"])
    _, _, idx_c = cport.invert_numpy(ic.oinv.Prepared(lco, lcr, ic.DSIG_CO), c["sc"]["inc"], c["sc"]["sco"], c["sc"]["scr"], c["sc"]["dsig"],
                                     c["sc"]["anc"], return_idx=True)
    live = i_co >= 0
    assert np.array_equal(idx_c[..., 0][live], 6 + i_co[live] % 16)
    o_co, o_cr, idx_np = ic.oracle_answer(lco, lcr, c["sc"], numpy_only=True)
    assert np.array_equal(idx_c, idx_np) and np.array_equal(idx_c, c["o_idx"])


@pytest.mark.parametrize("kind", ["co", "cr"])
def test_descending_incidence_axis(kind):
    """`_engine._ascending` sorts a LUT whose stored incidence axis descends.  Away from ties the slice a pixel reads holds the
    values the reference reads; on an exact tie between two nodes the sorted order decides, so the LOWER incidence wins where the
    reference (first minimum in stored order) takes the higher one."""
    from xsarsea_amd.windspeed import _engine
    from oracle import lut as olut
    stored = np.linspace(40.0, 36.0, 17)  # 0.25 degree steps downwards: every midpoint ties exactly
    rng = np.random.default_rng(4)
    if kind == "co":
        lut = olut.Lut(rng.normal(size=(17, 5, 4)), stored, np.linspace(1.0, 5.0, 5), np.linspace(0.0, 180.0, 4), "dB", "x", "co", "VV")
        d = _engine._co_dict(lut)
    else:
        lut = olut.Lut(rng.normal(size=(17, 6)), stored, np.linspace(1.0, 6.0, 6), None, "dB", "x", "cr", "VH")
        d = _engine._cr_dict(lut)
    assert np.array_equal(d["inc"], stored[::-1]) and np.array_equal(d["db"], lut.values[::-1])
    xs = ic.flat_probes(d["inc"])
    got, _ = ibr.nearest_indices(d["inc"], xs)       # what the device reads after the install
    ref = ibr.argmin_indices(stored, xs)             # windspeed.py:212 on the stored axis
    tie = np.abs(stored[None, :] - xs[:, None])
    tie = np.sum(tie == tie.min(axis=1, keepdims=True), axis=1) > 1
    assert tie.sum() == 16 + 2 and np.array_equal(xs[tie & np.isfinite(xs)], ic.probes(d["inc"])["mid"])  # (+-inf tie over the whole axis)
    for j in np.flatnonzero(~tie):
        assert np.array_equal(d["db"][got[j]], lut.values[ref[j]]), xs[j]
    for j in np.flatnonzero(tie & np.isfinite(xs)):
        lo, hi = d["inc"][got[j]], stored[ref[j]]
        assert lo < xs[j] < hi and hi - xs[j] == xs[j] - lo, xs[j]
    # +-inf: slice 0 of the installed table, which is the stored table's last
    for j in np.flatnonzero(np.isinf(xs)):
        assert got[j] == 0 and ref[j] == 0 and d["inc"][0] == stored[-1]
