"""GPU: every table a co-pol LUT install derives on the device (k_pad_co, k_transpose_slices, k_mono_rows, k_tail_min,
k_inv_range, k_inv_rows, k_block_minmax, k_band_minmax), read back whole with xsw_lut_table_read and compared BIT FOR BIT, pad
columns and slack included, with the numpy restatement (tests/lut_tables_ref.py) of the dense table that went in.  The tables
are comparisons, minima and maxima, one fused multiply-add and one directed cast: no tolerance anywhere.  Nothing here launches a
search; each test is an install plus copies.  Every comparison prints, per table, the number of elements that differ."""
import ctypes
import time

import numpy as np
import pytest

import lut_table_shapes as ls
import lut_tables_ref as ref

pytestmark = pytest.mark.gpu

CR = dict(db=np.array([[-30.0, -25.0, -20.0], [-29.0, -24.0, -19.0]]), inc=np.array([20.0, 40.0]), wspd=np.array([1.0, 10.0, 19.0]))


@pytest.fixture(scope="module")
def ctx():
    """One context of this module's own: its tables change with every install below."""
    from xsarsea_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need the MI355X box")
    c = _lib.Context(0)
    yield c
    c.close()


def read_all(ctx, shape):
    return {name: ctx.read_lut_table(name, shape) for name in ref.TABLES}


def report(what, diff, extra=""):
    print(f"\n{what}: " + ", ".join(f"{k} {n}" for k, n in diff.items()) + extra)


def check(ctx, what, dense, inv_slices=None):
    """Holds the context's current install to the restatement of `dense`; returns the names of the tables that differ."""
    got = read_all(ctx, dense.shape)
    want = ref.all_tables(dense, inv_slices)
    if inv_slices is not None and got["inv_rows"] is not None:
        got["inv_rows"] = got["inv_rows"][list(inv_slices)]
    diff = ref.compare(got, want)
    finite, absmax, prunable = ctx.read_lut_table("scalars", dense.shape)
    report(what, diff, f"; scalars {finite:g} {absmax!r} {prunable:g}")
    assert (finite, absmax) == ref.scalars(dense) and prunable == 1.0, what
    return [k for k, n in diff.items() if n]


def test_every_shape_on_one_context(ctx):
    """The tables of lut_table_shapes.SHAPES in INSTALL_ORDER on one context (a smaller table after a larger one and back: a
    pointer or a size left from the previous install would show), each through upload_luts with a trivial cross-pol table.
    no_inverse: inv_rows and inv_grid read back ABSENT, every other table present and right."""
    wrong = {}
    for n, key in enumerate(ls.INSTALL_ORDER):
        dense = ls.table(key)
        inc, wspd, phi = ls.axes(key)
        ctx.upload_luts(co=dict(db=dense, inc=inc, wspd=wspd, phi=phi), cr=CR)
        assert np.array_equal(ctx.read_lut(dense.shape), dense)
        bad = check(ctx, f"install {n} {key} {dense.shape}", dense)
        if bad:
            wrong[(n, key)] = bad
        absent = [k for k in ref.TABLES if ctx.read_lut_table(k, dense.shape) is None]
        assert absent == (["inv_grid", "inv_rows"] if key == "no_inverse" else []), key
    assert not wrong


@pytest.mark.parametrize("route", ["host", "device"])
def test_default_cmod5n(ctx, default_luts, route):
    """The default CMOD5.N table (501 x 499 x 181), uploaded from the host or built by xsw_lut_build; the restatement is evaluated
    on xsw_lut_read's table of the same context.  All tables in full but inv_rows, which is compared on every 25th slice and the
    first and last (a correctly rounded threshold for all 10^6 bins is slow on the CPU: 21 slices take 0.8 s of the restatement).
    Measured on an MI355X host, the line this test prints (host route): "read-back of inv_rows alone (378 MB) 0.042 s, of all
    tables (1328 MB) 0.089 s, restatement 1.14 s, comparison 0.07 s"; device route: 0.043 s, 0.089 s, 0.95 s, 0.07 s.  The whole
    test takes 1.6 s.  (The read-back is no empty copy: the comparison that follows finds every element of those buffers equal.)"""
    from xsarsea_amd.windspeed import _engine, get_model
    lco, _ = default_luts
    if route == "host":
        ctx.upload_luts(co=_engine._co_dict(lco), cr=CR)
    else:
        plan = get_model("gmf_cmod5n").device_lut_plan()
        _engine.DeviceLut("gmf_cmod5n", plan[0], plan[1], plan[2], key=None).build(ctx)
    shape = lco.values.shape
    assert shape == (501, 499, 181)
    dense = ctx.read_lut(shape)
    if route == "host":
        assert np.array_equal(dense, lco.values)
    slices = sorted(set(range(0, shape[0], 25)) | {0, shape[0] - 1})
    ta = time.perf_counter()
    inv_bytes = ctx.read_lut_table("inv_rows", shape).nbytes  # the largest table, once on its own for its time
    t0 = time.perf_counter()
    got = read_all(ctx, shape)
    t1 = time.perf_counter()
    all_bytes = sum(a.nbytes for a in got.values())
    want = ref.all_tables(dense, slices)
    t2 = time.perf_counter()
    got["inv_rows"] = got["inv_rows"][slices]
    diff = ref.compare(got, want)
    finite, absmax, prunable = ctx.read_lut_table("scalars", shape)
    report(f"default CMOD5.N, {route} route", diff, f"; scalars {finite:g} {absmax!r} {prunable:g}; read-back of inv_rows alone ({inv_bytes / 1e6:.0f} MB) "
           f"{t0 - ta:.3f} s, of all tables ({all_bytes / 1e6:.0f} MB) {t1 - t0:.3f} s, "
           f"restatement {t2 - t1:.2f} s, comparison {time.perf_counter() - t2:.2f} s")
    assert (finite, absmax) == ref.scalars(dense) and prunable == 1.0
    assert not any(diff.values()), diff
    assert (want["mono_rows"] < shape[1]).any() and (want["mono_rows"] == shape[1]).any()  # CMOD5.N saturates at the low incidences only


def test_lowres_cmod5n_built_on_the_device(ctx, lowres_luts):
    """The low-resolution CMOD5.N table built by xsw_lut_build, all tables in full."""
    from xsarsea_amd.windspeed import _engine, get_model
    plan = get_model("gmf_cmod5n").device_lut_plan(resolution="low")
    dl = _engine.DeviceLut("gmf_cmod5n", plan[0], plan[1], plan[2], key=None)
    dl.build(ctx)
    assert dl.shape == lowres_luts[0].values.shape
    assert not check(ctx, f"low-resolution CMOD5.N, device route {dl.shape}", ctx.read_lut(dl.shape))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_table_that_is_not_finite(ctx, bad):
    """One NaN / one +inf in the (3, 9, 5) table: the flag reads not finite, prunable is 0, co / co32 / coT hold the value in
    place, co_absmax is the largest FINITE magnitude.  (The derived bounds are not compared: fmin / fmax skip a NaN where numpy
    does not, and no kernel reads them on a table that is not prunable.)"""
    dense = ls.table("one_block").copy()
    dense[1, 4, 2] = bad
    inc, wspd, phi = ls.axes("one_block")
    ctx.upload_luts(co=dict(db=dense, inc=inc, wspd=wspd, phi=phi), cr=CR)
    got = {k: ctx.read_lut_table(k, dense.shape) for k in ("co", "co32", "coT")}
    diff = ref.compare(got, ref.all_tables(dense, bounds=False))
    finite, absmax, prunable = ctx.read_lut_table("scalars", dense.shape)
    report(f"one_block with one {bad}", diff, f"; scalars {finite:g} {absmax!r} {prunable:g}")
    assert not any(diff.values()), diff
    g = ref.geometry(*dense.shape)
    assert np.array_equal(got["co"][(1 * 9 + 4) * g.ppad + 2], bad, equal_nan=True)
    assert (finite, prunable) == (0.0, 0.0) and absmax == ref.scalars(dense)[1] and np.isfinite(absmax)


def test_error_paths_leave_the_buffer_alone():
    """xsw_lut_table_read on a fresh context: no LUT -> XSW_ENOLUT; a wrong size or an unknown id -> XSW_EINVAL with a message; an
    optional table that was not built -> XSW_TAB_ABSENT.  In each the output buffer keeps its fill."""
    from xsarsea_amd import _lib
    c = _lib.Context(0)
    try:
        lib, h = c._lib, c._h
        buf = np.full(4096, 0xA5, np.uint8)

        def call(which, nbytes):
            rc = lib.xsw_lut_table_read(h, which, ctypes.c_void_p(buf.ctypes.data), nbytes)
            assert (buf == 0xA5).all(), (which, nbytes)
            return rc, lib.xsw_last_error(h).decode()

        lay = _lib.co_table_layouts(*ls.SHAPES["no_inverse"])
        assert call(lay["mono_rows"][0], 2048 * 4)[0] == -3  # XSW_ENOLUT
        with pytest.raises(_lib.XswError, match="no co-pol LUT"):
            c.read_lut_table("mono_rows", ls.SHAPES["no_inverse"])
        inc, wspd, phi = ls.axes("no_inverse")
        c.upload_luts(co=dict(db=ls.table("no_inverse"), inc=inc, wspd=wspd, phi=phi), cr=CR)
        for nbytes in (2048 * 4 - 4, 2048 * 4 + 4, 0):
            rc, msg = call(lay["mono_rows"][0], nbytes)
            assert rc == -1 and "8192 bytes" in msg, (rc, msg)  # XSW_EINVAL
        rc, msg = call(lay["scalars"][0], 16)
        assert rc == -1 and "24 bytes" in msg
        for which in (-1, 12, 1000):
            rc, msg = call(which, 8)
            assert rc == -1 and "unknown table" in msg
        for name in ("inv_rows", "inv_grid"):
            assert call(lay[name][0], 4096)[0] == _lib.TAB_ABSENT == 1
            assert c.read_lut_table(name, ls.SHAPES["no_inverse"]) is None
        assert lib.xsw_lut_table_read(h, lay["mono_rows"][0], None, 8192) == -1
        assert np.array_equal(c.read_lut_table("mono_rows", ls.SHAPES["no_inverse"]), ref.mono_rows(ls.table("no_inverse")))
    finally:
        c.close()
