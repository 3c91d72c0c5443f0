"""k_invert_band with no kernel argument carried across its passes in lanes of a VGPR (xsw_band.hpp: kernargs_again): the tail
(lists, caps, masks, output pointers, the store's tables, the dual select) and stage 1's hand-over decisions read their arguments
again from the kernel-argument segment.  No candidate and no score changes, so everything equals `algo="exhaustive"` on the same
context bit for bit, with equal indices.  The exhaustive route is mono co-pol only: of a dual-pol launch the co-pol winds and
indices are held against it, the cross-pol / selected output against the general kernel's full search (`algo="exact"`).
The other two tests pin what any later change to the kernel's index arithmetic or to the passes' row counts has to keep: pixel
indices at every raster edge, and windows at the first and the last row of the table."""
import numpy as np
import pytest

import lut_tables_ref as ltr
import prune_model as pm
from test_gpu_band_cs_lds import _cmod_lut, _install
from test_gpu_band_pool import _classes_scene
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import torch  # noqa: F401 (fixture)
from util import bits_equal, lut_dicts

pytestmark = pytest.mark.gpu

SENT = -7777.0  # what the outputs hold before the launch: no wind, index or code of a real pixel


@pytest.fixture(scope="module")
def ctx_default(gpu_ctx, default_luts):
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)
    yield gpu_ctx
    gpu_ctx.upload_luts(co=co, cr=cr)  # (the last test installs tables of its own)


def _device(ctx, torch, arrs, want, dual_select=False, guard=1):
    """xsw_invert (pruned) on device rasters.  want: subset of {"co", "cr", "idx", "cc", "ccr"}.  Every output is a raster of
    `guard` extra lines above and below the one the call writes, all pre-filled with SENT; returns the host copies, guards included."""
    from xsarsea_amd import _lib
    dev = torch.device("cuda", 0)
    inc, s_co, s_cr, dsig, anc = arrs
    lines, samples = inc.shape
    f32 = inc.dtype == np.float32
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]
    kinds = dict(co=torch.complex64 if f32 else torch.complex128, cr=torch.complex64 if f32 else torch.complex128, idx=torch.int32, cc=torch.int32,
                 ccr=torch.int32)
    o, ptr = {}, {}
    for k in want:
        shape = (lines + 2 * guard, samples) + ((3,) if k == "idx" else ())
        o[k] = torch.full(shape, SENT, dtype=kinds[k], device=dev)
        ptr[k] = o[k][guard:].data_ptr()
    torch.cuda.synchronize()
    p = lambda x: None if x is None else x.data_ptr()
    ctx.invert_raw(lines, samples, _lib.XSW_F32 if f32 else _lib.XSW_F64, _lib.XSW_F32 if f32 else _lib.XSW_F64, _lib.MEM_DEVICE, p(t[0]), p(t[1]), p(t[2]),
                   p(t[3]), p(t[4]), ptr.get("co"), ptr.get("cr"), out_idx=ptr.get("idx"), algo=_lib.ALGO_PRUNED, dual_select=dual_select,
                   out_code_co=ptr.get("cc"), out_code_cr=ptr.get("ccr"))
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _inside(got, guard=1):
    """The raster the call wrote, after checking that the guard lines still hold the sentinel and no pixel inside does."""
    out = {}
    for k, v in got.items():
        body = v[guard:v.shape[0] - guard]
        edge = np.concatenate([v[:guard].ravel(), v[v.shape[0] - guard:].ravel()])
        assert np.all(edge == np.asarray(SENT).astype(v.dtype)), (k, "a store outside the raster")
        if k in ("co", "cr"):
            assert not np.any(body.real == SENT), (k, "a pixel was not stored")
        elif k == "idx":
            assert not np.any(body == int(SENT)), (k, "a pixel was not stored")
        out[k] = body
    return out


_REF = {}


def _reference(ctx, key, arrs):
    """Computed once per scene: the exhaustive sweep (co-pol winds, indices, codes) and, for a dual-pol scene, the general
    kernel's full search with and without the dual select."""
    if key not in _REF:
        inc, s_co, s_cr, dsig, anc = arrs
        cdt = np.complex64 if inc.dtype == np.float32 else np.complex128
        ex = ctx.invert_host(inc, sigma0_co=s_co, anc=anc, algo="exhaustive", want_idx=True, want_codes=True, out_dtype=cdt)
        r = dict(co=ex[0], idx=ex[2], cc=ex[3][0])
        if s_cr is not None:
            for sel in (False, True):
                d = ctx.invert_host(inc, sigma0_co=s_co, sigma0_cr=s_cr, dsig_cr=dsig, anc=anc, algo="exact", want_idx=True, want_codes=True,
                                    dual_select=sel, out_dtype=cdt)
                # (an index triplet is (speed, direction, cross-pol speed): the first two are the exhaustive sweep's)
                assert bits_equal(d[0], r["co"]) and np.array_equal(d[2][..., :2], r["idx"][..., :2])
                r["cr", sel], r["ccr", sel], r["idx", sel] = d[1], d[3][1], d[2]
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _same(got, ref, what, sel=False):
    for k, v in got.items():
        want = ref[k, sel] if (k, sel) in ref else ref[k]
        if k in ("co", "cr"):
            assert bits_equal(v, want), (what, k)
        else:
            assert np.array_equal(v.view(np.uint32), np.asarray(want).view(np.uint32)), (what, k)


@pytest.mark.parametrize("dual", [False, True], ids=["mono", "dual"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(7, 130), (9, 333)], ids=["7x130", "9x333"])
def test_arguments_read_again_behind_the_passes(ctx_default, torch, shape, dtype, dual):
    """Every combination of outputs the device-raster call offers: the tail picks its lists, caps, output pointers, the store's
    tables and the dual select from the kernel-argument segment after the last barrier, and what is null must stay unwritten."""
    inc, s_vv, s_vh, dsig, anc = synthetic_scene(shape[0], shape[1], dtype, 60 + shape[0])
    arrs = (inc, s_vv, s_vh, dsig, anc) if dual else (inc, s_vv, None, None, anc)
    ref = _reference(ctx_default, (shape, np.dtype(dtype).name, dual), arrs)
    combos = [({"co"}, False), ({"cc"}, False), ({"co", "idx"}, False)]
    if dual:
        combos = [({"co", "cr"}, False), ({"cc", "ccr"}, False), ({"co", "cr", "idx"}, False), ({"co", "cr"}, True),
                  ({"cc", "ccr"}, True), ({"co", "cr", "idx", "cc", "ccr"}, True)]
    for want, sel in combos:
        got = _inside(_device(ctx_default, torch, arrs, want, dual_select=sel))
        _same(got, ref, (shape, sorted(want), sel), sel)


@pytest.mark.parametrize("samples", [1, 63, 64, 65, 129, 577])
@pytest.mark.parametrize("lines", [1, 3, 4, 5])
def test_scalar_line_and_strip_index(ctx_default, torch, lines, samples):
    """The line, the strip number and the pixel index of every lane, put together again behind the passes: heights that leave
    waves past the last line, widths that leave part-filled strips and (577: 10 strips) strips in more than one of the 8 column
    ranges.  NaN in the first and the last pixel; outputs pre-filled, with guard lines around them."""
    inc, s_vv, anc = _classes_scene(lines, samples, 300 + 7 * lines + samples)
    inc = np.where(np.isnan(inc), 38.0, inc)  # (the generator blanks the first three samples: live pixels at every width)
    s_vv = np.where(np.isnan(s_vv), 0.02, s_vv)
    s_vv[0, 0] = np.nan
    s_vv[-1, -1] = np.nan
    arrs = (inc.astype(np.float32), s_vv.astype(np.float32), None, None, anc.astype(np.complex64))
    ref = _reference(ctx_default, ("strip", lines, samples), arrs)
    got = _inside(_device(ctx_default, torch, arrs, {"co", "idx", "cc"}))
    _same(got, ref, (lines, samples))
    assert np.isnan(got["co"][0, 0].real) and np.isnan(got["co"][-1, -1].real)
    if samples > 1:
        assert np.isfinite(got["co"].real).any()


def _stage1_model(lco, grid, monos, inc, s_lin, a, dsig=0.1):
    """What stage 1 of k_invert_band parks for one pixel, by tests/prune_model.py (the head of band_pruned_argmin: three rays, the
    window, the band radius, the tail cut; then table_bins): (eligible, incidence bin, w_lo, w_hi, bin_hi) or None."""
    from oracle import invert as oinv
    wspd, phi = np.asarray(lco.wspd), np.asarray(lco.phi)
    n_w, n_phi = len(wspd), len(phi)
    phi_180 = (180.0 - (phi[-1] - phi[0])) < 2.0
    with np.errstate(all="ignore"):
        s = float(oinv.to_db(np.float64(s_lin)))
    ar, b = float(a.real), float(a.imag)
    if phi_180:
        b = abs(b)
    if not (np.isfinite(inc) and np.isfinite(s) and np.isfinite(ar) and np.isfinite(b)):
        return None
    i_inc = int(np.argmin(np.abs(np.asarray(lco.incidence) - float(inc))))
    sl = lco.values[i_inc]
    cphi, sphi = np.cos(np.radians(phi)), np.sin(np.radians(phi))
    w0, inv_wstep = wspd[0], (n_w - 1) / (wspd[-1] - wspd[0])
    phi0, inv_dphi = phi[0], (n_phi - 1) / (phi[-1] - phi[0])
    inv, wh = 1.0 / dsig, 0.5 * wspd
    sn, ah, bh = -s * inv, 0.5 * ar, 0.5 * b
    m2 = ah * ah + bh * bh
    theta = np.degrees(np.arctan2(b, ar))
    if theta < phi0:
        theta += 360.0
    ipr = int(np.clip(np.rint((theta - phi0) * inv_dphi), 0, n_phi - 1))
    npairs, rbest, seed = (n_w + 1) >> 1, np.inf, 0
    for q, ipq in enumerate((ipr, max(ipr - 2, 0), min(ipr + 2, n_phi - 1))):
        ur = 2.0 * (ah * cphi[ipq] + bh * sphi[ipq])
        lo, hi = (0, npairs) if q == 0 else (max(seed - 4, 0), min(seed + 4, npairs))
        col = sl[:, ipq]
        for _ in range(int(npairs).bit_length() if q == 0 else 3):
            mid = min((lo + hi) >> 1, npairs - 1)
            ja = wh[2 * mid] * (wh[2 * mid] - ur) + (col[2 * mid] * inv + sn) ** 2
            jb = wh[2 * mid + 1] * (wh[2 * mid + 1] - ur) + (col[2 * mid + 1] * inv + sn) ** 2 if 2 * mid + 1 < n_w else np.inf
            rbest = min(rbest, ja, jb)
            if lo < hi:
                lo, hi = (mid + 1, hi) if jb < ja else (lo, mid)
        if q == 0:
            seed = lo
    j_ub = (rbest + m2) * (1.0 + 1e-9) + 1e-9
    w_lo, w_hi, ip_lo, ip_hi = pm.search_window(np.sqrt(ar * ar + b * b), theta, rbest + m2, w0, inv_wstep, n_w, phi0, phi[-1], inv_dphi, n_phi)
    d = pm.band_radius(j_ub, dsig)
    mono = monos[i_inc]
    if w_hi >= mono and ip_hi >= ip_lo and s + d < pm.tail_min(sl, mono, ip_lo, ip_hi):
        w_hi = mono - 1
    elig = w_hi < mono and w_hi >= w_lo and ip_hi >= ip_lo
    _, b_hi = pm.table_bins(grid[i_inc][0], grid[i_inc][1], grid[i_inc][2], ltr.INV_BINS, s - d, s + d)
    return elig, i_inc, w_lo, w_hi, b_hi


@pytest.mark.parametrize("n_phi", [61, 181])
def test_row_count_fold_at_the_table_edges(ctx_default, n_phi):
    """A small CMOD5.N table (101 speeds, 5 incidences).  A pass counts the rows min(rb - 1, w_hi) - max(ra, w_lo) + 1 of a
    direction and addresses slice and inverse-table rows from the slot's words: shown on the CPU before the GPU result is compared, the scene holds windows that start at row 0, windows that end at the last
    row, bands with no threshold above them (bin_hi = -1) and pixels of the first and of the last incidence slice."""
    lco = _cmod_lut(n_phi, 180.0)
    _install(ctx_default, lco)
    n_w, n_inc = len(lco.wspd), len(lco.incidence)
    lines, samples = 6, 200
    inc, s_vv, anc = _classes_scene(lines, samples, 17)
    inc = np.where(np.isnan(inc), 38.0, inc)
    phi = np.asarray(lco.phi)
    k = np.arange(40)
    ip = (k * 7) % n_phi
    e = np.exp(1j * np.radians(phi[ip]))
    # line 0: calm pixels of the first slice (windows from row 0); line 1: pixels at the top of the last slice, sigma0 a little
    # above the table's largest value (windows to the last row, no threshold above the band); lines 2 and 3: the same on the
    # other slice
    for ln, i_inc, top in ((0, 0, False), (1, n_inc - 1, True), (2, n_inc - 1, False), (3, 0, True)):
        inc[ln, 10:50] = lco.incidence[i_inc]
        row = n_w - 1 if top else 1
        s_vv[ln, 10:50] = 10.0 ** (lco.values[i_inc, row, ip if not top else 0 * ip] / 10.0) * (1.01 if top else 1.0)
        anc[ln, 10:50] = (np.asarray(lco.wspd)[row] * (0.998 if top else 0.5)) * (e if not top else 1.0 + 0j)
    monos = [pm.mono_rows(lco.values[i]) for i in range(n_inc)]
    grid = ltr.inv_grid(np.asarray(lco.values), monos)
    seen = dict(row0=0, last_row=0, no_bin_hi=0, first_slice=0, last_slice=0)
    for i in [(ln, sm) for ln in range(lines) for sm in range(samples) if ln < 4 and 10 <= sm < 50 or (ln * samples + sm) % 11 == 0]:
        m = _stage1_model(lco, grid, monos, inc[i], s_vv[i], anc[i])
        if m is None or not m[0]:
            continue
        _, i_inc, w_lo, w_hi, b_hi = m
        seen["row0"] += w_lo == 0
        seen["last_row"] += w_hi == n_w - 1
        seen["no_bin_hi"] += b_hi < 0
        seen["first_slice"] += i_inc == 0
        seen["last_slice"] += i_inc == n_inc - 1
    print("pixels of the band rule with each condition:", seen)
    assert all(v > 0 for v in seen.values()), seen
    got = ctx_default.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="pruned", want_idx=True)
    ex = ctx_default.invert_host(inc, sigma0_co=s_vv, anc=anc, algo="exhaustive", want_idx=True)
    assert bits_equal(got[0], ex[0])
    assert np.array_equal(got[2], ex[2])
