"""Incidence axes, probes and LUT pairs for the incidence-bin tests (tests/test_inc_bin_cpu.py without a GPU,
tests/test_gpu_inc_bin.py on one).  Everything here is numpy on the host and deterministic.

Every per-pixel kernel that reads a LUT starts with `nearest_index` (csrc/xsw_device.hpp): the device form of
`np.argmin(np.abs(inc_dim - inc))`, first minimum.  The probes sit where that choice can go wrong -- on the nodes, on the midpoints
between two nodes (exact ties on many of them), one float64 step to either side of both, beyond the ends, at +-inf and NaN -- and
the tables are made so that a wrong slice cannot hide: the answer of every kernel differs from what either neighbouring slice
would give (`assert_self_identifying`, on the CPU oracle, before any device runs).

AXES        one incidence axis per edge of the function (uniform with ties and near-ties, all ties, coarse, not uniform, float32
            values that look uniform and are not, two nodes, one node, 2048 nodes)
SETS        one LUT install per axis: that axis for the co-pol table and a DIFFERENT one for the cross-pol table, so that a swap of
            i_inc and i_inc_cr shows
probes      the float64 probes of one axis, by class;  probes32: the float32 ones (every float32 k * 0.05 inside the axis, the
            float32 roundings of the midpoints)
case(name)  the whole problem of one set: tables, a float64 and a float32 raster (one line per probe class, the co-pol axis'
            probes then the cross-pol axis', padded with NaN incidences), the oracle's answer and grid codes
"""
import functools

import numpy as np

import inc_bin_ref as ibr
from oracle import invert as oinv
from oracle import lut as olut

DSIG_CO = 0.1
N_W, N_PHI, N_WCR = 32, 37, 28
W_AX = np.linspace(1.0, 16.5, N_W)        # 0.5 m/s steps, exact
PHI_AX = np.linspace(0.0, 180.0, N_PHI)   # 5 degree steps: phi_180
WCR_AX = np.linspace(2.0, 15.5, N_WCR)    # the co-pol speed rows 2 .. 29

_DEFAULT = np.linspace(17.0, 50.0, 331)
AXES = {
    "default": _DEFAULT,                                                  # uniform; 190 of its 330 midpoints tie exactly, the others nearly
    "binary": np.linspace(16.0, 48.0, 129),                               # uniform, 0.25 degree steps: every midpoint ties exactly
    "coarse": np.linspace(17.0, 50.0, 34),
    "nonuniform": 17.0 + np.concatenate([[0.0], np.cumsum(np.tile([0.5, 0.75, 1.25], 14))]),  # bisection; binary fractions: ties
    "float32_stored": _DEFAULT.astype(np.float32).astype(np.float64),     # looks uniform, is not to 1e-12: bisection
    "two": np.array([24.0, 31.5]),
    "one": np.array([33.0]),                                              # inv_step = 0, not uniform
    "long": np.linspace(17.0, 50.0, 2048),                                # the walk's start bin comes from a large g
}
UNIFORM = ("default", "binary", "coarse", "two", "long")  # what uniform_axis must say (tests/test_inc_bin_cpu.py asks the header)
# set -> (co-pol axis, cross-pol axis, shift of the cross-pol axis in degrees)
SETS = {
    "default": ("default", "coarse", 0.37),
    "binary": ("binary", "binary", 0.125),        # (thinned to every 4th node below: 1 degree steps from 16.125)
    "coarse": ("coarse", "default", -0.37),
    "nonuniform": ("nonuniform", "float32_stored", 0.0),
    "float32_stored": ("float32_stored", "nonuniform", 0.37),
    "two": ("two", "one", 0.0),
    "one": ("one", "two", 0.0),
    "long": ("long", "long", 0.2),
}
CLASSES = ("node", "node_dn", "node_up", "mid", "mid_dn", "mid_up", "ends")
CLASSES32 = ("grid", "mid", "ends")


def set_axes(name):
    co, cr, shift = SETS[name]
    cr_ax = AXES[cr][::4] if name == "binary" else AXES[cr]
    return AXES[co].copy(), cr_ax + shift


def _thin(n):
    """`long`: every 8th node / midpoint plus the first and last 16."""
    k = np.arange(n)
    return k[(k % 8 == 0) | (k < 16) | (k >= n - 16)]


def probes(ax, thin=False):
    """{class: float64 probes} of one axis: every node, its two float64 neighbours, every midpoint 0.5 * (a[i] + a[i + 1]), its two
    neighbours, and the ends a[0] - 3, a[0] - 1e-9, a[-1] + 1e-9, a[-1] + 3, +inf, -inf, NaN."""
    ax = np.asarray(ax, dtype=np.float64)
    nodes, mids = ax, 0.5 * (ax[:-1] + ax[1:])
    if thin:
        nodes, mids = nodes[_thin(nodes.size)], mids[_thin(mids.size)]
    return {"node": nodes, "node_dn": np.nextafter(nodes, -np.inf), "node_up": np.nextafter(nodes, np.inf),
            "mid": mids, "mid_dn": np.nextafter(mids, -np.inf), "mid_up": np.nextafter(mids, np.inf),
            "ends": np.array([ax[0] - 3.0, ax[0] - 1e-9, ax[-1] + 1e-9, ax[-1] + 3.0, np.inf, -np.inf, np.nan])}


def probes32(ax, thin=False):
    """{class: float32 probes}: every float32 value k * 0.05 inside the axis, the float32 roundings of the midpoints, the ends."""
    ax = np.asarray(ax, dtype=np.float64)
    k = np.arange(int(np.ceil(ax[0] / 0.05)) - 1, int(np.floor(ax[-1] / 0.05)) + 2)
    grid = (k * 0.05).astype(np.float32)
    grid = grid[(grid >= ax[0]) & (grid <= ax[-1])]
    mids = 0.5 * (ax[:-1] + ax[1:])
    if thin:
        mids = mids[_thin(mids.size)]
    return {"grid": grid, "mid": mids.astype(np.float32),
            "ends": np.array([ax[0] - 3.0, ax[-1] + 3.0, np.inf, -np.inf, np.nan], dtype=np.float32)}


def flat_probes(ax, thin=False):
    """The float64 probes of one axis in one array (classes in order), NaN left out."""
    p = np.concatenate([probes(ax, thin)[c] for c in CLASSES])
    return p[~np.isnan(p)]


def build_luts(name):
    """(co-pol, cross-pol) dB tables of one set, [n_inc, N_W, N_PHI] and [n_inc_cr, N_WCR], strictly increasing along speed.
    Slice i of the co-pol table crosses 0 dB at speed row 6 + i % 16 with a slope of 3 + 0.37 (i % 5) dB per row, the same in every
    direction (the a-priori wind alone picks the direction); slice i of the cross-pol table at row 5 + i % 12 with 2 + 0.3 (i % 3) dB
    per row (steps for which no two neighbouring slices hold the same value in any row).  With sigma0 within
    0.6 dB of 0 the zero crossing decides the winning speed row, so the row names the slice among its neighbours, and the slope --
    the curvature of the cost -- does so in the error bars."""
    inc_co, inc_cr = set_axes(name)
    i = np.arange(inc_co.size)
    co = (3.0 + 0.37 * (i % 5))[:, None, None] * (np.arange(N_W)[None, :, None] - (6 + i % 16)[:, None, None]) + np.zeros(N_PHI)[None, None, :]
    i = np.arange(inc_cr.size)
    cr = (2.0 + 0.3 * (i % 3))[:, None] * (np.arange(N_WCR)[None, :] - (5 + i % 12)[:, None])
    return (olut.Lut(np.ascontiguousarray(co), inc_co, W_AX.copy(), PHI_AX.copy(), "dB", "x", "co", "VV"),
            olut.Lut(np.ascontiguousarray(cr), inc_cr, WCR_AX.copy(), None, "dB", "x", "cr", "VH"))


def shifted(lut, d):
    """`lut` with slice i replaced by slice i + d (clamped): what a kernel that took the neighbouring slice would read."""
    n = len(lut.incidence)
    v = np.ascontiguousarray(np.asarray(lut.values)[np.clip(np.arange(n) + d, 0, n - 1)])
    return olut.Lut(v, lut.incidence, lut.wspd, lut.phi, lut.units, lut.resolution, lut.name, lut.pol)


def build_raster(name, dtype):
    """dict(inc, sco, scr, dsig, anc) of `dtype`: one line per probe class, the co-pol axis' probes then the cross-pol axis', padded
    with NaN incidences.  sigma0 is in dB, within 0.6 dB of 0; the a-priori wind has 3 .. 7 m/s and points 50 .. 130 degrees off the
    antenna, to either side; dsig_cr lies in 0.1 .. 0.2."""
    f32 = np.dtype(dtype) == np.float32
    thin = name == "long"
    per_axis = [(probes32 if f32 else probes)(ax, thin) for ax in set_axes(name)]
    lines = [np.concatenate([p[c] for p in per_axis]).astype(np.float64) for c in (CLASSES32 if f32 else CLASSES)]
    width = max(ln.size for ln in lines)
    inc = np.full((len(lines), width), np.nan)
    for r, ln in enumerate(lines):
        inc[r, :ln.size] = ln
    j = np.arange(inc.size, dtype=np.float64).reshape(inc.shape)
    sco, scr = 0.6 * np.sin(0.7 * j), 0.6 * np.sin(0.9 * j + 1.0)
    dsig = 0.1 + 0.05 * (1.0 + np.sin(0.13 * j))
    anc = (5.0 + 2.0 * np.sin(0.31 * j)) * np.exp(1j * np.deg2rad(90.0 + 40.0 * np.sin(0.17 * j)))
    anc = np.where(j % 3 == 0, np.conj(anc), anc)
    cdt = np.complex64 if f32 else np.complex128
    return dict(inc=np.ascontiguousarray(inc, dtype=dtype), sco=sco.astype(dtype), scr=scr.astype(dtype), dsig=dsig.astype(dtype),
                anc=np.ascontiguousarray(anc, dtype=cdt))


def oracle_answer(lco, lcr, sc, numpy_only=False):
    """The CPU oracle on one raster (sigma0 in dB): (co, cr, idx) of the dual-pol call.  The C restatement where it is built
    (identical arithmetic), the numpy restatement otherwise."""
    p = oinv.Prepared(lco, lcr, DSIG_CO)
    if not numpy_only:
        try:
            from oracle import cport
            cport.lib()
            return cport.invert_numpy(p, sc["inc"], sc["sco"], sc["scr"], sc["dsig"], sc["anc"], return_idx=True, reference_layout=False)
        except Exception:
            pass
    return oinv.invert_numpy(p, sc["inc"], sc["sco"], sc["scr"], sc["dsig"], sc["anc"], return_idx=True)


def codes_of(lco, lcr, o_co, o_cr, o_idx):
    """The oracle's answer as the grid codes the kernels store (include/xsw.h: out_code_co, out_code_cr without the select)."""
    import crosspol_codes_ref as xref
    iw, ip, icr = (o_idx[..., k].astype(np.int64) for k in range(3))
    assert np.all((iw < 0) | ((ip > 0) & (ip < len(lco.phi) - 1))), "a winning direction on the border: the sign of Im does not name the -phi solution"
    flat = iw * len(lco.phi) + ip + ((o_co.imag < 0).astype(np.int64) << 30)  # 0 < phi < 180: Im < 0 is the -phi solution (windspeed.py:234-242)
    cc = np.where(iw >= 0, flat, np.where(np.isnan(o_co.imag), xref.CODE_NAN, xref.CODE_NAN_RE)).astype(np.uint32)
    ccr = np.where(icr >= 0, icr, np.where(np.isnan(o_cr.imag), xref.CODE_NO_INDEX, xref.CODE_NAN_RE)).astype(np.uint32)
    return cc, ccr


def from_codes_refs(lco, lcr, sc, cc, ccr):
    """What every from-codes kernel must give on raster `sc` with the codes (cc, ccr): the existing CPU restatements."""
    import cost_codes_ref as cref
    import crosspol_codes_ref as xref
    import joint_ref as jref
    import uncertainty_joint_ref as ujref
    import uncertainty_ref as uref
    p = oinv.Prepared(lco, lcr)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    inc, sco, scr, dsig, anc = f64(sc["inc"]), f64(sc["sco"]), f64(sc["scr"]), f64(sc["dsig"]), np.asarray(sc["anc"], dtype=np.complex128)
    joint = jref.joint(cc, inc, sco, anc, DSIG_CO, scr, dsig, p)
    return dict(cost_co=cref.cost_co(cc, inc, sco, anc, DSIG_CO, p), cost_cr=cref.cost_cr(cc, ccr, inc, scr, dsig, p),
                cross=xref.cross_from_codes(cc, inc, scr, dsig, xref.tables(lco, lcr)), joint=joint,
                unc_co=uref.unc_co(cc, inc, sco, anc, DSIG_CO, p), unc_cr=uref.unc_cr(cc, ccr, inc, scr, dsig, p),
                unc_joint=ujref.unc_joint(joint["code"], inc, sco, anc, DSIG_CO, scr, dsig, p))


def bins(name, sc):
    """(i_inc, i_inc_cr) of every pixel by the specification, -1 where the incidence is NaN."""
    inc_co, inc_cr = set_axes(name)
    shape = sc["inc"].shape
    return ibr.argmin_indices(inc_co, sc["inc"]).reshape(shape), ibr.argmin_indices(inc_cr, sc["inc"]).reshape(shape)


def _differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return ~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind in "fc" else a != b


def assert_self_identifying(name, dtype):
    """On the oracle and the restatements alone: with the co-pol (cross-pol) slice forced to either neighbour, the winning (iw, ip)
    (icr) and the output of every from-codes kernel that reads that table differ on EVERY probe whose neighbour exists; and every
    probe but the NaN ones has an answer, an interior grid point and error bars (flag 0), so that no comparison is NaN against NaN."""
    c = case(name, dtype)
    lco, lcr, sc, ref = c["lco"], c["lcr"], c["sc"], c["ref"]
    i_co, i_cr = c["i_inc"], c["i_inc_cr"]
    live = i_co >= 0
    assert np.array_equal(c["o_idx"][..., 0] >= 0, live) and np.array_equal(c["o_idx"][..., 2] >= 0, live), name
    for k in ("unc_co", "unc_cr", "unc_joint"):
        assert np.all(ref[k]["flag"][live] == 0), (name, k, np.unique(ref[k]["flag"][live], return_counts=True))
    assert np.all(ref["joint"]["code"][live] < 0x80000000) and np.all(np.isfinite(ref["joint"]["Jsig_cr"][live])), name
    for which, d in (("co", -1), ("co", 1), ("cr", -1), ("cr", 1)):
        n_ax = len(lco.incidence) if which == "co" else len(lcr.incidence)
        i_ax = i_co if which == "co" else i_cr
        has = live & (i_ax + d >= 0) & (i_ax + d < n_ax)
        if not has.any():
            continue
        l2co, l2cr = (shifted(lco, d), lcr) if which == "co" else (lco, shifted(lcr, d))
        _, _, idx2 = oracle_answer(l2co, l2cr, sc)
        r2 = from_codes_refs(l2co, l2cr, sc, c["cc"], c["ccr"])
        if which == "co":
            differ = {"inversion (iw, ip)": np.any(idx2[..., :2] != c["o_idx"][..., :2], axis=-1),
                      "cost_co J": _differs(r2["cost_co"]["J"], ref["cost_co"]["J"]),
                      "joint (code, J)": (r2["joint"]["code"] != ref["joint"]["code"]) | _differs(r2["joint"]["J"], ref["joint"]["J"]),
                      "unc_co wspd_std": _differs(r2["unc_co"]["wspd_std"], ref["unc_co"]["wspd_std"]),
                      "unc_joint wspd_std": _differs(r2["unc_joint"]["wspd_std"], ref["unc_joint"]["wspd_std"])}
        else:
            differ = {"inversion icr": idx2[..., 2] != c["o_idx"][..., 2],
                      "cost_cr J": _differs(r2["cost_cr"]["J"], ref["cost_cr"]["J"]),
                      "cross code": r2["cross"][0] != ref["cross"][0],
                      "joint (code, J)": (r2["joint"]["code"] != ref["joint"]["code"]) | _differs(r2["joint"]["J"], ref["joint"]["J"]),
                      "unc_cr wspd_std": _differs(r2["unc_cr"]["wspd_std"], ref["unc_cr"]["wspd_std"]),
                      "unc_joint wspd_std": _differs(r2["unc_joint"]["wspd_std"], ref["unc_joint"]["wspd_std"])}
        for what, m in differ.items():
            assert np.all(m[has]), f"{name} {np.dtype(dtype).name}: {what} does not tell {which} slice i from slice i{d:+d} on {int(np.sum(has & ~m))} of {int(has.sum())} probes"


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """The problem of one set and raster dtype, built once per process: dict(lco, lcr, sc, i_inc, i_inc_cr, o_co, o_cr, o_idx, cc,
    ccr, ref).  Nothing in it is written to afterwards."""
    lco, lcr = build_luts(name)
    sc = build_raster(name, dtype)
    o_co, o_cr, o_idx = oracle_answer(lco, lcr, sc)
    cc, ccr = codes_of(lco, lcr, o_co, o_cr, o_idx)
    i_inc, i_inc_cr = bins(name, sc)
    return dict(lco=lco, lcr=lcr, sc=sc, i_inc=i_inc, i_inc_cr=i_inc_cr, o_co=o_co, o_cr=o_cr, o_idx=o_idx, cc=cc, ccr=ccr,
                ref=from_codes_refs(lco, lcr, sc, cc, ccr))
