"""xsarsea_amd.calibrate on the MI355X against its CPU restatement (tests/calibrate_ref.py).  Every comparison is bit for bit
(`calibrate_ref.same_bits`: NaN where and only where the restatement has NaN, every other value equal as an unsigned integer).
The scenes are tests/calibrate_cases.py's, which asserts what each is there for on the restatement before anything runs here:
the vector path and the element-wise one (a ragged last quad; a base aligned to 2 bytes only), uint16 and float32 digital numbers,
three workgroup columns and three strips of lines, the last a tail; each with every combination of present tables, to float32
and float64, through device tensors and through numpy arrays."""
import warnings

import numpy as np
import pytest

import calibrate_cases as cc
import calibrate_ref as cref
from ancillary_model_ref import bracket
from test_gpu_kernel import synthetic_scene
from test_gpu_streams import _held_back, _in_flight, _read_back
from test_gpu_streams import delay_cycles, torch  # noqa: F401  (fixtures)
from util import bits_equal
from xsarsea_amd import AnnotationGrid, _lib, calibrate_dn, raster_from_grid, windspeed

pytestmark = pytest.mark.gpu

FIELDS = ("sigma0", "nesz", "incidence", "valid")


def host(t):
    return None if t is None else t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def device(torch):
    return torch.device("cuda", 0)


def place(torch, name, route):
    """The scene's digital numbers as the route hands them in.  Device: `vec` as torch.uint16, `elem` as torch.int16 (the same
    bits), `offset` as an int16 view from element 1 of a flat buffer, so that its base is aligned to 2 bytes only."""
    dn = np.array(cc.digital_numbers(name))
    if name == "offset":
        flat = np.zeros(dn.size + 1, dn.dtype)
        flat[1:] = dn.ravel()
        if route == "numpy":
            return flat[1:].reshape(dn.shape)
        t = torch.from_numpy(flat.view(np.int16)).to(device(torch))[1:].view(dn.shape)
        assert t.data_ptr() % 8 == 2 and t.is_contiguous()
        return t
    if route == "numpy":
        return dn
    if dn.dtype == np.uint16 and (name == "elem" or not hasattr(torch, "uint16")):
        dn = dn.view(np.int16)
    return torch.from_numpy(dn).to(device(torch))


def package_tables(samples, combo):
    g = cc.grids(samples)
    return AnnotationGrid(*g["lut"]), {k: None if v is None else AnnotationGrid(*v) for k, v in cc.tables(samples, combo).items()}


def assert_same(got, want, what, fields=FIELDS):
    for f in fields:
        g, w = host(got[f]), want[f]
        if w is None:
            assert g is None, f"{what}: {f} was not asked for"
        else:
            assert g is not None and g.dtype == w.dtype and cref.same_bits(g, w), \
                f"{what} {f}: {int((g != w).sum()) if g is not None and g.shape == w.shape else '?'} pixels differ (NaN counted)"


# ----------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("route", ["device", "numpy"])
@pytest.mark.parametrize("name", cc.SCENES)
def test_calibrate_dn(torch, name, route):
    dn = place(torch, name, route)
    samples = cc.SAMPLES[name]
    for dtype in ("float32", "float64"):
        for combo in cc.COMBOS:
            lut, kw = package_tables(samples, combo)
            got = calibrate_dn(dn, lut, dtype=dtype, valid=True, **kw)
            for f in FIELDS:
                if got[f] is not None:
                    assert (isinstance(got[f], torch.Tensor) and got[f].is_cuda) == (route == "device") and tuple(got[f].shape) == (cc.L, samples)
            assert_same(got, cc.case(name, combo, dtype), f"{name} {route} {dtype} {'+'.join(combo) or 'no table'}")


@pytest.mark.parametrize("route", ["device", "numpy"])
def test_device_argument_and_other_fill_values(torch, route):
    """A numpy `dn` with device= goes up as its own 2 bytes per pixel and gives device tensors; fill=None and another fill value."""
    dn = np.array(cc.digital_numbers("vec"))
    lut, kw = package_tables(2100, cc.TABLES)
    if route == "device":
        got = calibrate_dn(dn, lut, device="cuda:0", valid=True, **kw)
        assert got.sigma0.is_cuda and got.valid.dtype == torch.uint8
        assert_same(got, cc.case("vec"), "device=")
        dn = torch.from_numpy(dn.view(np.int16)).to(device(torch))
    for fill in (None, 65535, 17):
        assert_same(calibrate_dn(dn, lut, fill=fill, valid=True, **kw), cc.case("vec", cc.TABLES, "float32", fill), f"fill={fill} {route}")
    f32 = np.array(cc.digital_numbers("f32"))
    f32[3, 5], f32[70, 2099] = np.nan, 0.5
    want = cref.calibrate(f32, cc.grids(2100)["lut"], fill=0.5, **cc.tables(2100, cc.TABLES))
    assert np.isnan(want["sigma0"][70, 2099]) and np.isnan(want["sigma0"][3, 5]) and want["sigma0"][0, 0] == cc.case("f32")["sigma0"][0, 0]
    got = calibrate_dn(torch.from_numpy(f32).to(device(torch)) if route == "device" else f32, lut, fill=0.5, valid=True, **kw)
    assert_same(got, want, f"float32 fill {route}")


@pytest.mark.parametrize("route", ["device", "numpy"])
def test_raster_from_grid(torch, route):
    dev = "cuda:0" if route == "device" else None
    for samples in (2100, 2099):
        g = cc.grids(samples)
        for key in ("incidence", "lut", "azimuth"):
            for dtype in (np.float32, np.float64):
                got = raster_from_grid(AnnotationGrid(*g[key]), shape=(cc.L, samples), dtype=dtype, device=dev)
                assert (hasattr(got, "is_cuda") and got.is_cuda) == (route == "device")
                want = cref.raster_from_grid(g[key], np.arange(cc.L), np.arange(samples), dtype)
                assert cref.same_bits(host(got), want), (samples, key, dtype)
    # coordinates of the caller's: fractional, descending, a single line
    g = cc.grids(2100)["lut"]
    line, sample = np.array([-2.5, 79.75, 20.0, 33.3]), 2099.0 - 0.7 * np.arange(2999)
    got = raster_from_grid(AnnotationGrid(*g), line=line, sample=sample, dtype="float64", device=dev)
    assert cref.same_bits(host(got), cref.raster_from_grid(g, line, sample, np.float64))
    assert tuple(raster_from_grid(AnnotationGrid(*g), shape=(0, 7), device=dev).shape) == (0, 7)


def test_outputs_left_out_leave_the_rest_unchanged(torch):
    for name in ("vec", "elem"):
        samples = cc.SAMPLES[name]
        lut, kw = package_tables(samples, cc.TABLES)
        want = cc.case(name)
        for put in (lambda a: torch.from_numpy(a.view(np.int16)).to(device(torch)), lambda a: a):
            dn = put(np.array(cc.digital_numbers(name)))
            lean = calibrate_dn(dn, lut, nesz=False, valid=True, **kw)
            assert lean.nesz is None
            assert_same(lean, want, f"{name} nesz=False", ("sigma0", "incidence", "valid"))
            default = calibrate_dn(dn, lut, **kw)
            assert default.valid is None
            assert_same(default, want, f"{name} defaults", ("sigma0", "nesz", "incidence"))
            kw_no_inc = dict(kw, incidence=None)
            bare = calibrate_dn(dn, lut, nesz=False, **kw_no_inc)
            assert bare.nesz is None and bare.incidence is None and bare.valid is None
            assert_same(bare, want, f"{name} sigma0 alone", ("sigma0",))


# ------------------------------------------------------------------------------------------------------------------------ chain
def test_calibrated_rasters_feed_the_inversion(torch):
    """60 x 260: calibrate_dn on the device, its float32 tensors straight into invert_from_model; the restatement's float32
    rasters through the numpy route give the same bits."""
    import xsarsea_amd
    L, S = 60, 260
    _, s_vv, _, _, anc = synthetic_scene(L, S, np.float32, 53)
    lut = (np.array([0.0, L - 1.0]), np.array([0.0, 100.0, S - 1.0]), np.array([[480.0, 510.0, 560.0], [470.0, 505.0, 555.0]]))
    inc = (np.array([0.0, L - 1.0]), np.array([0.0, S - 1.0]), np.array([[30.0, 46.0], [30.2, 46.1]]))
    A = cref.blend(lut, np.arange(float(L)), np.arange(float(S)))
    dn = np.nan_to_num(np.rint(np.sqrt(s_vv.astype(np.float64)) * A), nan=0.0).clip(0, 65535).astype(np.uint16)
    want = cref.calibrate(dn, lut, incidence=inc)
    assert (dn == 0).sum() > 20 and np.isnan(want["sigma0"]).sum() == (dn == 0).sum() and 0.001 < np.nanmedian(want["sigma0"]) < 1.0
    cal = calibrate_dn(torch.from_numpy(dn.view(np.int16)).to(device(torch)), AnnotationGrid(*lut), incidence=AnnotationGrid(*inc))
    assert cal.sigma0.dtype == torch.float32 and cal.incidence.dtype == torch.float32
    old = (xsarsea_amd.options.device_out_dtype, xsarsea_amd.options.db_on_device)
    try:
        xsarsea_amd.options.device_out_dtype = "complex64"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            co = windspeed.invert_from_model(cal.incidence, cal.sigma0, ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
            xsarsea_amd.options.db_on_device = True
            ref = windspeed.invert_from_model(want["incidence"], want["sigma0"], ancillary_wind=anc, model="gmf_cmod5n", resolution="low")
    finally:
        xsarsea_amd.options.device_out_dtype, xsarsea_amd.options.db_on_device = old
    assert co.is_cuda and co.dtype == torch.complex64 and tuple(co.shape) == (L, S)
    assert (~np.isnan(ref.real)).mean() > 0.9 and bits_equal(co.cpu().numpy(), ref.astype(np.complex64))


# ----------------------------------------------------------------------------------------------------------------------- stream
def test_call_is_ordered_on_the_callers_stream(torch, delay_cycles):  # noqa: F811
    """`dn` is filled on a non-default stream behind a held-back producer; the call, issued on that stream, returns while the
    producer is still in flight and its outputs are those of the filled values."""
    dn = np.array(cc.digital_numbers("vec"))
    decoy = (dn // 2 + 1).astype(np.uint16)
    lut, kw = package_tables(2100, cc.TABLES)
    want = cc.case("vec")
    assert not cref.same_bits(cref.calibrate(decoy, cc.grids(2100)["lut"], **cc.tables(2100, cc.TABLES))["sigma0"], want["sigma0"])
    up = lambda a: torch.from_numpy(a.view(np.int16)).to(device(torch))
    buf, src = up(decoy), up(dn)
    calibrate_dn(src, lut, valid=True, **kw)   # once on landed values: the code object is loaded
    torch.cuda.synchronize()
    P = torch.cuda.Stream(device=device(torch))
    with torch.cuda.stream(P):
        done = _held_back(torch, P, delay_cycles, [(buf, src)])
        out = calibrate_dn(buf, lut, valid=True, **kw)
        _in_flight(done)
        got = _read_back(torch, P, out.sigma0, out.nesz, out.incidence, out.valid)
    assert_same(dict(zip(FIELDS, got)), want, "behind a held-back producer")


# -------------------------------------------------------------------------------------------------------------------- raw entry
def test_raw_entry_refusals_leave_the_outputs_alone():
    """xsw_calibrate itself on host buffers: dn == NULL with anything but the incidence table and the incidence output, dn
    without the sigma0 LUT, a bad mem, dtype or fill, a table without a bracket: XSW_EINVAL each, and no output is written."""
    ctx = _lib.default_context(0)
    L, S = 9, 21
    rng = np.random.default_rng(5)
    dn = rng.integers(0, 300, (L, S)).astype(np.uint16)
    grids = {"lut": (np.array([0.0, 8.0]), np.array([0.0, 20.0]), np.array([[400.0, 500.0], [450.0, 550.0]])),
             "range": (np.array([0.0, 8.0]), np.array([0.0, 7.0, 20.0]), np.array([[900.0, 700.0, 800.0], [950.0, 750.0, 850.0]])),
             "incidence": (np.array([0.0, 8.0]), np.array([0.0, 20.0]), np.array([[20.0, 40.0], [21.0, 41.0]]))}
    keep = []

    def table(key, **o):
        gl, gs, v = grids[key]
        lf, lt = bracket(gl, np.arange(float(L)))
        sf, st = bracket(gs, np.arange(float(S)))
        arrays = [np.ascontiguousarray(v, np.float64), np.ascontiguousarray(lf, np.int32), np.ascontiguousarray(lt, np.float64),
                  np.ascontiguousarray(sf, np.int32), np.ascontiguousarray(st, np.float64)]
        keep.append(arrays)
        ptrs = [a.ctypes.data for a in arrays]
        if "drop" in o:
            ptrs[o["drop"]] = None
        return (o.get("n_lines", len(gl)), len(gs), *ptrs)

    outs = {k: np.full((L, S), 7, np.float32) for k in ("sigma0", "nesz", "incidence")}
    outs["valid"] = np.full((L, S), 7, np.uint8)
    untouched = lambda: all((a == 7).all() for a in outs.values())

    def call(dn_=dn, lut="lut", rng_="range", azi=None, inc="incidence", mem=_lib.MEM_HOST, dn_dtype=_lib.DN_U16, out_dtype=_lib.XSW_F32, fill=0,
             want=("sigma0", "nesz", "incidence", "valid"), tabs=None):
        t = tabs or [None if k is None else table(k) for k in (lut, rng_, azi, inc)]
        ctx.calibrate_raw(L, S, mem, dn_dtype, out_dtype, None if dn_ is None else dn_.ctypes.data, *t, fill,
                          *[outs[k].ctypes.data if k in want else None for k in ("sigma0", "nesz", "incidence", "valid")])

    bad = [dict(dn_=None),                                                   # dn == NULL with the calibration tables and outputs
           dict(dn_=None, lut=None, rng_=None),                              # ... with outputs that need dn
           dict(dn_=None, lut=None, rng_=None, inc=None, want=("incidence",)),  # ... without the incidence table
           dict(dn_=None, rng_=None, want=("incidence",)),                   # ... with the sigma0 LUT
           dict(dn_=None, lut=None, rng_=None, want=()),                     # ... without the incidence output
           dict(lut=None),                                                   # dn without the sigma0 LUT
           dict(inc=None),                                                   # the incidence output without its table
           dict(want=()),                                                    # no output
           dict(mem=7), dict(mem=_lib.MEM_HOST_PINNED), dict(dn_dtype=2), dict(out_dtype=5), dict(fill=65536.0), dict(fill=0.5), dict(fill=-1.0),
           dict(tabs=[table("lut", drop=3), None, None, table("incidence")]),   # a table without a bracket
           dict(tabs=[table("lut", n_lines=0), None, None, table("incidence")])]
    for kw in bad:
        with pytest.raises(_lib.XswError):
            call(**kw)
        assert untouched(), kw
    call()
    want = cref.calibrate(dn, grids["lut"], noise_range=grids["range"], incidence=grids["incidence"])
    for k in FIELDS:
        assert cref.same_bits(outs[k], want[k]), k
    only = np.full((L, S), 7, np.float64)     # dn == NULL, the incidence table and output alone: raster_from_grid
    ctx.calibrate_raw(L, S, _lib.MEM_HOST, _lib.DN_U16, _lib.XSW_F64, None, None, None, None, table("incidence"), None, None, None, only.ctypes.data, None)
    assert cref.same_bits(only, cref.raster_from_grid(grids["incidence"], np.arange(L), np.arange(S), np.float64))
