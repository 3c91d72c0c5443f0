"""Benchmark of xsarsea_amd.calibrate (k_calibrate, csrc/xsw_calibrate.hip) on a 20000 x 20000 raster of uint16 digital numbers
made from the flagship scene.  HIP events, median of warm repetitions, the variants taking turns inside every repetition.  Prints
one JSON line and writes it to profiles/calibrate_bench.json:

  - k_calibrate uint16 -> float32: sigma0 alone (2 B read + 4 B written per pixel), with nesz and incidence (2 + 12, all four
    tables), with valid as well (2 + 13); the incidence table alone (4 B written: raster_from_grid)
  - beside them, in the same run: k_detrend (4 B read + 8 B written: the yardstick of the streaming kernels) and
    k_ancillary_model (16 B written, division-bound); each as a fraction of the 8 TB/s peak by its streamed bytes, and
    k_calibrate's times against what their bytes would take at k_detrend's measured rate
  - end to end on the first --e2e-lines lines, VV + VH: (a) calibrate_dn(numpy uint16, tables) -> dsig_from_nesz -> the dual-pol
    invert_from_model on the resulting device tensors; (b) the same rasters expanded on the host by the numpy restatement
    (tests/calibrate_ref.py; untimed, and compared with (a)'s bit for bit) and passed as numpy float32 through the same two calls;
    wall time of both and the bytes that crossed the link in each

    python profiles/bench_calibrate.py [--size 20000] [--steps 7] [--warmup 2] [--e2e-lines 5000] [--out profiles/calibrate_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

sys.path.insert(0, os.path.join(REPO, "tests"))

import calibrate_ref as cref  # noqa: E402  (tests/: the numpy restatement, route (b)'s host expansion)
from bench_ancillary_model import scene  # noqa: E402  (same folder)

HBM_PEAK = 8.0e12
NESZ_CR = 10 ** -3.5  # the cross-pol noise floor of bench.make_crosspol


def annotation(n):
    """name -> (line, sample, values): tables of a product's sizes -- calibration and range-noise vectors every 1000 lines and 40
    samples, an azimuth-noise table of four swath blocks whose boundaries are neighbouring nodes, an 11 x 21 geolocation grid."""
    line = np.unique(np.append(np.arange(-500.0, n, 1000.0), n - 1.0))
    sample = np.unique(np.append(np.arange(0.0, n, 40.0), n - 1.0))
    x = sample / max(n - 1, 1)
    lut = (line, sample, 520.0 + 90.0 * x[None, :] - 0.0005 * line[:, None])
    rng = (line, sample, 1.0 + 0.35 * np.cos(6.0 * x)[None, :] + 0.00001 * line[:, None])
    cuts = [int(n * f) for f in (0.3, 0.55, 0.8)]
    az_s = np.array([0.0] + [c + d for c in cuts for d in (0, 1)] + [n - 1.0])
    az_l = np.unique(np.append(np.arange(0.0, n, 500.0), n - 1.0))
    level = NESZ_CR * 560.0 ** 2 * np.repeat([0.9, 1.1, 0.95, 1.2], 2)
    az = (az_l, az_s, level[None, :] * (1.0 + 0.02 * np.sin(az_l / 700.0))[:, None])
    il, isamp = np.linspace(0.0, n - 1.0, 11), np.linspace(0.0, n - 1.0, 21)
    inc = (il, isamp, 30.0 + 16.0 * (isamp / max(n - 1, 1))[None, :] + 0.01 * np.sin(il / max(n, 1))[:, None])
    return {"lut": lut, "range": rng, "azimuth": az, "incidence": inc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e-lines", type=int, default=5000)
    ap.add_argument("--e2e-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "calibrate_bench.json"))
    a = ap.parse_args()

    import torch
    import bench  # the scene generator of the flagship benchmark (repository root)
    from xsarsea_amd import AnnotationGrid, TiePoints, _build, _lib, calibrate_dn, streaks as S, windspeed

    n = a.size
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    inc, s_vv, anc = bench.make_scene(n, n, n, 0, 20260320 + 2, dev)
    s_vh, _ = bench.make_crosspol(inc, anc, 7, dev)
    tabs = annotation(n)
    grids = {k: AnnotationGrid(*v) for k, v in tabs.items()}
    put = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)

    def table(key):
        gl, gs, v = tabs[key]
        lf, lt = S.bracket(gl, np.arange(n))
        sf, st = S.bracket(gs, np.arange(n))
        return [len(gl), len(gs), put(v, np.float64), put(lf, np.int32), put(lt, np.float64), put(sf, np.int32), put(st, np.float64)]

    t_lut, t_rng, t_az, t_inc = (table(k) for k in ("lut", "range", "azimuth", "incidence"))
    raw = lambda t: None if t is None else (t[0], t[1], *[x.data_ptr() for x in t[2:]])

    def digital_numbers(sigma0, rows):
        """uint16 DN (as int16 bits) whose calibration gives sigma0 back within the quantisation: DN = rint(sqrt(sigma0 + nesz) * A)."""
        out = torch.empty(sigma0.shape, dtype=torch.int16, device=dev)
        A = torch.empty((rows, n), dtype=torch.float64, device=dev)
        nz = torch.empty((rows, n), dtype=torch.float64, device=dev)
        for r0 in range(0, sigma0.shape[0], rows):
            r1 = min(r0 + rows, sigma0.shape[0])
            m = r1 - r0
            # A and nesz of these lines from the kernel under test itself (untimed scene synthesis): DN = 1 gives g and N * g
            one = torch.ones((m, n), dtype=torch.int16, device=dev)
            tl = lambda t: None if t is None else (t[0], t[1], t[2].data_ptr(), t[3][r0:r1].contiguous().data_ptr(), t[4][r0:r1].contiguous().data_ptr(),
                                                   t[5].data_ptr(), t[6].data_ptr())
            ctx.calibrate_raw(m, n, _lib.MEM_DEVICE, _lib.DN_U16, _lib.XSW_F64, one.data_ptr(), tl(t_lut), tl(t_rng), tl(t_az), None, None,
                              A[:m].data_ptr(), nz[:m].data_ptr(), None, None)
            ctx.synchronize()
            g = A[:m] + nz[:m]                      # (1 - N) g + N g = g = 1 / A**2
            dn = torch.sqrt((sigma0[r0:r1].double().nan_to_num(0.0) + nz[:m]) / g).round().clamp(0, 65535)
            out[r0:r1] = dn.to(torch.int32).to(torch.int16)
        return out

    dn_vv, dn_vh = digital_numbers(s_vv, 2000), digital_numbers(s_vh, 2000)
    del s_vh
    f32 = lambda: torch.empty((n, n), dtype=torch.float32, device=dev)
    o_s0, o_nz, o_inc, o_valid = f32(), f32(), f32(), torch.empty((n, n), dtype=torch.uint8, device=dev)
    DEV, p = _lib.MEM_DEVICE, lambda t: None if t is None else t.data_ptr()

    def cal(tables, outs):
        return lambda: ctx.calibrate_raw(n, n, DEV, _lib.DN_U16, _lib.XSW_F32, p(dn_vh), *[raw(t) for t in tables], 0, *[p(o) for o in outs])

    variants = {
        "k_calibrate sigma0": cal([t_lut, None, None, None], [o_s0, None, None, None]),
        "k_calibrate sigma0+nesz+incidence": cal([t_lut, t_rng, t_az, t_inc], [o_s0, o_nz, o_inc, None]),
        "k_calibrate sigma0+nesz+incidence+valid": cal([t_lut, t_rng, t_az, t_inc], [o_s0, o_nz, o_inc, o_valid]),
        "k_calibrate incidence table alone": lambda: ctx.calibrate_raw(n, n, DEV, _lib.DN_U16, _lib.XSW_F32, None, None, None, None, raw(t_inc), None,
                                                                       None, None, p(o_inc), None),
    }
    bytes_px = {"k_calibrate sigma0": 6, "k_calibrate sigma0+nesz+incidence": 14, "k_calibrate sigma0+nesz+incidence+valid": 15,
                "k_calibrate incidence table alone": 4, "k_detrend": 12, "k_ancillary_model": 16}
    det = torch.empty((n, n), dtype=torch.float64, device=dev)
    ratio = np.random.default_rng(0).uniform(0.5, 2.0, n)
    variants["k_detrend"] = lambda: ctx.detrend_raw(n, n, _lib.XSW_F32, _lib.XSW_F64, DEV, s_vv.data_ptr(), ratio, det.data_ptr())
    tie_line, tie_sample, lon, lat, heading, mlon, mlat, mu, mv = scene(n)
    tp = TiePoints(tie_line, tie_sample, lon, lat, heading)
    lf, lt = S.bracket(tp.line, np.arange(n))
    sf, st = S.bracket(tp.sample, np.arange(n))
    ties = [put(x, np.float64) for x in (tp.longitude, tp.latitude, tp.cos_heading, tp.sin_heading)]
    ties += [put(lf, np.int32), put(lt, np.float64), put(sf, np.int32), put(st, np.float64)]
    tu, tv = put(mu[::-1], np.float64), put(mv[::-1], np.float64)
    wind = torch.empty((n, n), dtype=torch.complex128, device=dev)
    dlon, dlat = float(mlon[-1] - mlon[0]) / (len(mlon) - 1), float(mlat[0] - mlat[-1]) / (len(mlat) - 1)
    variants["k_ancillary_model"] = lambda: ctx.ancillary_model_raw(n, n, DEV, _lib.XSW_F64, p(tu), p(tv), len(mlat), len(mlon), float(mlon[0]), dlon, 0,
                                                                    float(mlat[-1]), dlat, len(tp.line), len(tp.sample), *(p(x) for x in ties), p(wind))

    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.steps):  # alternating: one repetition of every variant per round
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    px = n * n
    frac = {k: bytes_px[k] * px / (med[k] * 1e-3) / HBM_PEAK for k in med}
    detrend_rate = bytes_px["k_detrend"] * px / (med["k_detrend"] * 1e-3)
    at_detrend = {k: med[k] / (bytes_px[k] * px / detrend_rate * 1e3) for k in med if k.startswith("k_calibrate")}
    valid_frac = float(o_valid.float().mean().item())
    del det, wind, o_s0, o_nz, o_inc, o_valid

    # ---- end to end, VV + VH, on the first lines of the raster
    m = min(a.e2e_lines, n)
    e2e_px = m * n
    line = np.arange(m)
    h_vv, h_vh = (t[:m].contiguous().cpu().numpy().view(np.uint16) for t in (dn_vv, dn_vh))
    d_anc, h_anc = anc[:m].contiguous(), anc[:m].contiguous().cpu().numpy()
    del dn_vv, dn_vh, s_vv, inc
    kw = dict(line=line, sample=np.arange(n), device=dev)
    models = ("gmf_cmod5n", "gmf_s1_v2")

    def route_a():
        co = calibrate_dn(h_vv, grids["lut"], incidence=grids["incidence"], nesz=False, **kw)
        cr = calibrate_dn(h_vh, grids["lut"], noise_range=grids["range"], noise_azimuth=grids["azimuth"], **kw)
        dsig = windspeed.dsig_from_nesz("gmf_s1_v2", co.incidence, cr.sigma0, cr.nesz, out_dtype=np.float32)
        out = windspeed.invert_from_model(co.incidence, co.sigma0, cr.sigma0, ancillary_wind=d_anc, dsig_cr=dsig, model=models)
        torch.cuda.synchronize()
        return co, cr, out

    b_parts = {"dsig_from_nesz": [], "invert_from_model": []}

    def route_b(h_inc, h_s_vv, h_s_vh, h_nesz):
        t0 = time.perf_counter()
        dsig = windspeed.dsig_from_nesz("gmf_s1_v2", h_inc, h_s_vh, h_nesz, out_dtype=np.float32)
        t1 = time.perf_counter()
        out = windspeed.invert_from_model(h_inc, h_s_vv, h_s_vh, ancillary_wind=h_anc, dsig_cr=dsig, model=models)
        b_parts["dsig_from_nesz"].append((t1 - t0) * 1e3)
        b_parts["invert_from_model"].append((time.perf_counter() - t1) * 1e3)
        return out

    def timed(fn, steps):
        out = []
        for _ in range(steps):
            t0 = time.perf_counter()
            res = fn()
            out.append((time.perf_counter() - t0) * 1e3)
            del res
        return out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        co, cr, _ = route_a()   # untimed: the first call installs the LUTs
        x_vv = cref.calibrate(h_vv, tabs["lut"], incidence=tabs["incidence"])   # untimed: the host expansion, route (b)'s inputs
        x_vh = cref.calibrate(h_vh, tabs["lut"], noise_range=tabs["range"], noise_azimuth=tabs["azimuth"])
        host = [x_vv["incidence"], x_vv["sigma0"], x_vh["sigma0"], x_vh["nesz"]]
        same = bool(all(cref.same_bits(t.cpu().numpy(), h) for t, h in zip((co.incidence, co.sigma0, cr.sigma0, cr.nesz), host)))
        del co, cr, x_vv, x_vh
        route_b(*host)          # untimed: the host route's staging is set up
        t_a = timed(route_a, a.e2e_steps)
        t_b = timed(lambda: route_b(*host), a.e2e_steps)

    rows = [r for r in _build.kernel_resources() if "k_calibrate" in r["kernel"] and ("unsigned short, float, true" in r["kernel"] or "ItfLb1E" in r["kernel"])]
    res = {"workload": "calibrate", "raster": [n, n], "steps": a.steps, "warmup": a.warmup,
           "tables": {k: list(v[2].shape) for k, v in tabs.items()},
           "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "bytes_per_pixel": bytes_px, "fraction_of_8_TB_per_s": {k: round(v, 4) for k, v in frac.items()},
           "time_over_time_at_k_detrend_rate": {k: round(v, 3) for k, v in at_detrend.items()},
           "more_than_twice_the_time_at_k_detrend_rate": {k: bool(v > 2.0) for k, v in at_detrend.items()},
           "valid_fraction": round(valid_frac, 4),
           "vgpr_uint16_float32_vector": {r["kernel"]: [r["vgpr"], r["sgpr"], r["scratch_bytes"], r["waves_per_simd_by_vgpr"]] for r in rows},
           "end_to_end": {"raster": [m, n], "steps": a.e2e_steps,
                          "a_calibrate_on_device_ms": round(float(np.median(t_a)), 1), "a_ms_all": [round(x, 1) for x in t_a],
                          "b_host_float32_rasters_ms": round(float(np.median(t_b)), 1), "b_ms_all": [round(x, 1) for x in t_b],
                          "b_parts_ms": {k: round(float(np.median(v[-a.e2e_steps:])), 1) for k, v in b_parts.items()},
                          "host_expansion_equals_device_rasters_bit_for_bit": same,
                          "a_bytes_up": 4 * e2e_px, "a_bytes_down": 0,
                          "b_bytes_up_at_least": (16 + 4 + 8) * e2e_px,
                          "note": "(a) numpy uint16 VV + VH in (2 B per pixel each), a-priori wind resident, device tensors out; (b) numpy float32 "
                                  "incidence, sigma0 VV, sigma0 VH, nesz (16 B per pixel), float32 dsig_cr (4 B) and the complex64 a-priori wind "
                                  "(8 B) in, numpy out; dsig_from_nesz on host arrays chooses its own route, its traffic is not counted.  (b)'s "
                                  "rasters are the numpy restatement's (tests/calibrate_ref.py), untimed"},
           "device": torch.cuda.get_device_name(0)}
    out_line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out_line + "\n")
    print(out_line)


if __name__ == "__main__":
    main()
