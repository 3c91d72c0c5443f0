"""k_invert_band's passes start from the offsets stage 1 leaves in the slot (csrc/xsw_band.hpp: BandSlot; csrc/xsw_bandslot.hpp):
the byte offsets of the incidence slice and of the two inverse-table rows, the doubled a-priori halves and |a/2|^2.  Same
candidates, same doubles: everything must equal `algo="exact"` bit for bit -- winds, grid codes, indices -- on small rasters with a
ragged tile in both directions, written into sentinel-filled outputs.

tests/band_slot_cases.py builds the rasters so that k_invert_band itself (not the kernels it hands pixels to) meets each window
class, windows of more than 128 directions and (on the table with 361 directions) of more than one chunk, part-filled last
passes, s - d below the threshold grid (bin 0), no threshold above s + d (the reserved offset), the first and the last incidence
slice, the last direction, and NaN holes.  That these occur among the pixels the kernel keeps is shown on the CPU (the model of
stage 1 there); that it decides at least half of the searchable pixels of every case is asserted from the device's own hand-over
counters.  Shares on these rasters, k_invert_band / handed on (list + band2 + blocks), the same before and after the change:
see LABBOOK 41."""
import collections

import numpy as np
import pytest

import band_slot_cases as bc
from test_gpu_streams import torch  # noqa: F401 (fixture)
from util import lut_dicts

pytestmark = pytest.mark.gpu

SENT = -7777.0  # what the outputs hold before the launch: no wind, index or code of a real pixel
SHAPES = {"5x70": (5, 70), "9x200": (9, 200)}
TABLES = ("default", "pad4", "wide")


@pytest.fixture(scope="module")
def tables(default_luts):
    """{name: (co-pol LUT, cross-pol LUT, Tables)}, made once."""
    out = {}
    for name in TABLES:
        lco, lcr = default_luts if name == "default" else bc.luts(name)
        out[name] = (lco, lcr, bc.Tables(lco))
    return out


@pytest.fixture(scope="module")
def ctx_tables(gpu_ctx, default_luts):
    """The session's context; installs a table pair on demand and puts the default pair back afterwards."""
    state = {"name": None}

    def install(name, pair):
        if state["name"] != name:
            co, cr = lut_dicts(*pair)
            gpu_ctx.upload_luts(co=co, cr=cr)
            state["name"] = name
        return gpu_ctx

    yield install
    co, cr = lut_dicts(*default_luts)
    gpu_ctx.upload_luts(co=co, cr=cr)


_SCENES = {}


def _scene(tables, table, shape):
    """(rasters, kept pixels by the model, searchable pixels) of one (table, shape), made once and read-only."""
    key = (table, shape)
    if key not in _SCENES:
        lco, lcr, tab = tables[table]
        lines, samples = SHAPES[shape]
        arrs = bc.scene(lco, lcr, lines, samples, seed=7 + lines)
        kept, crowd = bc.survey(tab, arrs[0], arrs[1], arrs[4])
        # (fewer wide windows per wave than stage 1's live arc asks for: the windows the model finds are the ones the passes sweep)
        assert crowd < bc.ARC_CROWD, crowd
        for a in arrs:
            a.setflags(write=False)
        _SCENES[key] = (arrs, kept, bc.searchable(arrs[0], arrs[1], arrs[4]))
    return _SCENES[key]


def _invert(ctx, torch, arrs, dual, algo, stats=False):
    """One float32 -> complex64 inversion on device rasters into sentinel-filled outputs with a guard line above and below:
    ({output: host copy, guards included}, timing(), stats() or None)."""
    from xsarsea_amd import _lib
    dev = torch.device("cuda", 0)
    inc, s_co, s_cr, dsig, anc = arrs
    if not dual:
        s_cr = dsig = None
    lines, samples = inc.shape
    t = [None if a is None else torch.from_numpy(np.array(a)).to(dev) for a in (inc, s_co, s_cr, dsig, anc)]
    kinds = dict(co=torch.complex64, cr=torch.complex64, idx=torch.int32, cc=torch.int32, ccr=torch.int32)
    o, ptr = {}, {}
    for k in ("co", "idx", "cc") + (("cr", "ccr") if dual else ()):
        o[k] = torch.full((lines + 2, samples) + ((3,) if k == "idx" else ()), SENT, dtype=kinds[k], device=dev)
        ptr[k] = o[k][1:].data_ptr()
    torch.cuda.synchronize()
    p = lambda x: None if x is None else x.data_ptr()
    ctx.timing_enable(True)
    if stats:
        ctx.stats_enable(True)
    try:
        ctx.invert_raw(lines, samples, _lib.XSW_F32, _lib.XSW_F32, _lib.MEM_DEVICE, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), ptr["co"], ptr.get("cr"),
                       out_idx=ptr["idx"], algo=_lib.ALGOS[algo], out_code_co=ptr["cc"], out_code_cr=ptr.get("ccr"))
        ctx.synchronize()
        tm, st = ctx.timing(), (ctx.stats() if stats else None)
    finally:
        ctx.timing_enable(False)
        if stats:
            ctx.stats_enable(False)
    return {k: v.cpu().numpy() for k, v in o.items()}, tm, st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.complex64 else a.view(np.float32).view(np.uint32)


def _check_outputs(got, want, what):
    for k, v in got.items():
        sent = np.asarray(SENT).astype(v.dtype)
        assert np.all(v[0] == sent) and np.all(v[-1] == sent), (what, k, "a store outside the raster")
        body = v[1:-1]
        if k in ("co", "cr"):
            assert not np.any(body.real == SENT), (what, k, "a pixel was not stored")
        elif k == "idx":
            assert not np.any(body == int(SENT)), (what, k, "a pixel was not stored")
        assert np.array_equal(_bits(v), _bits(want[k])), (what, k, int(np.sum(_bits(v) != _bits(want[k]))))


_EXACT = {}


def _exact(ctx, torch, key, arrs, dual):
    if key not in _EXACT:
        want, tm, _ = _invert(ctx, torch, arrs, dual, "exact")
        assert tm["launches"] == 0, "algo=exact is the general kernel alone"
        for v in want.values():
            v.setflags(write=False)
        _EXACT[key] = want
    return _EXACT[key]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("table", TABLES)
def test_scene_holds_every_condition_among_the_kept_pixels(tables, table, shape):
    """CPU only: what the rasters are built for, counted by the model of stage 1 among the pixels k_invert_band keeps."""
    lco, _, _ = tables[table]
    n_inc, n_w, n_phi = len(lco.incidence), len(lco.wspd), len(lco.phi)
    (inc, s_vv, _, _, anc), kept, n_search = _scene(tables, table, shape)
    classes = collections.Counter(bc.window_class(m["ncols"]) for m in kept)
    seen = dict(over_128=sum(m["ncols"] > 128 for m in kept), chunked=sum(m["ncols"] > bc.CHUNK for m in kept),
                bin0_below_grid=sum(m["below"] and m["b_lo"] == 0 for m in kept), none_above=sum(m["b_hi"] < 0 for m in kept),
                first_slice=sum(m["i_inc"] == 0 for m in kept), last_slice=sum(m["i_inc"] == n_inc - 1 for m in kept),
                last_direction=sum(m["ip_lo"] + m["ncols"] == n_phi for m in kept), first_row=sum(m["w_lo"] == 0 for m in kept),
                last_row=sum(m["w_hi"] == n_w - 1 for m in kept), nan_holes=int(inc.size - n_search))
    print(table, shape, "searchable", n_search, "kept by the model", len(kept), "classes", sorted(classes.items()), seen)
    widest = bc.window_class(n_phi)  # (73 directions: class 9 is the widest a window can be)
    assert set(classes) == set(range(widest + 1)), sorted(classes)
    need = set(seen) - ({"over_128", "chunked"} if n_phi <= 128 else {"chunked"} if n_phi <= bc.CHUNK else set())
    assert all(seen[k] > 0 for k in need), seen
    assert 2 * len(kept) >= n_search
    # a part-filled last pass: some workgroup (four lines x one strip) keeps a number of pixels that no class's pixels per pass
    # (32, 16, 8, 4, 2, 1) divides into whole passes -- not a multiple of 32, while narrow classes are present
    per_wg = collections.Counter((m["at"][0] // 4, m["at"][1] // 64) for m in kept)
    assert any(n % 32 for n in per_wg.values()), per_wg


@pytest.mark.parametrize("dual", [False, True], ids=["mono", "dual"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("table", TABLES)
def test_band_kernel_equals_exact(ctx_tables, tables, torch, table, shape, dual):
    lco, lcr, _ = tables[table]
    ctx = ctx_tables(table, (lco, lcr))
    arrs, kept, n_search = _scene(tables, table, shape)
    want = _exact(ctx, torch, (table, shape, dual), arrs, dual)
    got, tm, _ = _invert(ctx, torch, arrs, dual, "pruned")
    handed = int(tm["last_band2_pixels"]) + int(tm["last_blocks_pixels"]) + int(tm["last_list_pixels"])
    print(f"{table} {shape} {'dual' if dual else 'mono'}: searchable {n_search}, handed on by k_invert_band: band2 {tm['last_band2_pixels']}, "
          f"blocks {tm['last_blocks_pixels']}, list {tm['last_list_pixels']}; its own share {1.0 - handed / n_search:.3f}; kept by the model {len(kept)}")
    assert tm["launches"] == 1, "the chain ran"
    _check_outputs(got, want, (table, shape, dual))
    # the winning directions include the table's last one (a pixel the model says k_invert_band keeps)
    won = {int(got["idx"][1 + m["at"][0], m["at"][1], 1]) for m in kept}
    assert len(lco.phi) - 1 in won, max(won)
    # (the pixels with an infinite sigma0 are searchable and k_invert_list's: the counters count)
    assert int(tm["last_list_pixels"]) >= int(np.sum(np.isinf(arrs[1]) & ~np.isnan(arrs[0]) & ~np.isnan(np.abs(arrs[4])))) > 0
    assert 2 * handed <= n_search, ("k_invert_band decided fewer than half of the searchable pixels", handed, n_search)


def test_statistics_instantiation(ctx_tables, tables, torch):
    """The statistics instantiation (COUNT, ROLE 0: every window swept in k_invert_band, nothing handed to k_invert_band2) fills
    and reads the same slots: same outputs, and it searched exactly the searchable pixels."""
    table, shape = "default", "9x200"
    lco, lcr, _ = tables[table]
    ctx = ctx_tables(table, (lco, lcr))
    arrs, _, n_search = _scene(tables, table, shape)
    want = _exact(ctx, torch, (table, shape, False), arrs, False)
    got, _, st = _invert(ctx, torch, arrs, False, "pruned", stats=True)
    _check_outputs(got, want, "statistics")
    assert st["pixels_co"] == n_search and st["cand_co"] > 0, (st, n_search)
