"""The scenes that tests/test_calibrate_cpu.py and tests/test_gpu_calibrate.py share, and the restatement's results on them
(tests/calibrate_ref.py), computed once and read-only.  `digital_numbers(name)` asserts on the restatement what each scene is
there for, before anything runs on a device; `launch(lines, samples)` states the launch k_calibrate is expected to get, from the
kernel's own constants read from its source.

    vec     75 x 2100 uint16: 525 quads of samples make three workgroup columns, the last ragged; with strips of at least 32
            lines three strips, the last of 11 lines: two groups of four lines in flight and a tail of three
    elem    75 x 2099: the row's last quad is partial, every access element-wise
    offset  the vec raster, which the GPU test views out of a flat device buffer from element 1 on: a base aligned to 2 bytes only
    f32     vec with float32 digital numbers
"""
import functools

import numpy as np

import calibrate_ref as cref
from test_host_plan import source_define

L = 75
SAMPLES = {"vec": 2100, "elem": 2099, "offset": 2100, "f32": 2100}
SCENES = tuple(SAMPLES)
TABLES = ("range", "azimuth", "incidence")
# every combination of present tables: none, range only, azimuth only, both, each with and without incidence
COMBOS = tuple(tuple(t for t, on in zip(TABLES, (r, a, i)) if on) for i in (0, 1) for a in (0, 1) for r in (0, 1))


def launch(lines, samples):
    """(workgroup columns, line strips, lines per strip, lines of the last strip) of k_calibrate's launch: strip_grid over
    (lines, quads of samples) (tests/test_host_plan.py restates it) with strips of XSW_CAL_MIN_LINES lines or more."""
    quads = -(-samples // 4)
    gx = -(-quads // 256)
    gy = max(1, min(-(-256 * 16 // gx), lines, 65535))
    lpb = max(-(-lines // gy), source_define("XSW_CAL_MIN_LINES"))
    gy = -(-lines // lpb)
    return gx, gy, lpb, lines - (gy - 1) * lpb


@functools.lru_cache(maxsize=None)
def grids(samples):
    """name -> (line, sample, values).  The sigma0 LUT has a jump inside the quad 1000..1003 (nodes at the neighbouring samples
    1001 and 1002) and a node at a column that is no multiple of 4, its first line node lies before the raster; the azimuth
    noise jumps between lines 10 and 11, inside one group of four lines; the last sample node is the raster's last sample."""
    last = float(samples - 1)
    lut_s = np.array([0.0, 500.0, 1001.0, 1002.0, 1600.0, last])
    lut = np.array([320.0, 450.0, 520.0, 640.0, 610.0, 700.0])[None, :] - 5.0 * np.arange(4.0)[:, None]
    rng_s = np.array([0.0, 3.0, 700.0, last])
    rng_v = np.array([[5200.0, 4100.0, 2600.0, 3900.0], [4700.0, 3800.0, 2500.0, 3500.0], [5600.0, 4300.0, 2900.0, 4400.0]])
    azi_v = np.array([[0.8, 0.85], [0.9, 0.95], [1.3, 1.25], [1.2, 1.15], [1.0, 1.1]])
    inc_s = np.array([0.0, 700.0, 1400.0, last])
    inc_v = np.array([[17.0, 27.1, 36.3, 44.6], [17.2, 27.3, 36.5, 44.8], [17.4, 27.5, 36.7, 45.0]])
    out = {"lut": (np.array([-3.0, 20.0, 41.0, 80.0]), lut_s, lut), "range": (np.array([0.0, 37.0, 74.0]), rng_s, rng_v),
           "azimuth": (np.array([0.0, 10.0, 11.0, 50.0, 74.0]), np.array([0.0, last]), azi_v),
           "incidence": (np.array([0.0, 30.0, 74.0]), inc_s, inc_v)}
    assert lut.min() >= 300.0 and lut.max() <= 700.0 and inc_v.min() == 17.0 and inc_v.max() == 45.0
    for g in out.values():
        for a in g:
            a.setflags(write=False)
    return out


def tables(samples, combo):
    """Keyword arguments of cref.calibrate for the combination `combo` of TABLES."""
    g = grids(samples)
    return dict(noise_range=g["range"] if "range" in combo else None, noise_azimuth=g["azimuth"] if "azimuth" in combo else None,
                incidence=g["incidence"] if "incidence" in combo else None)


@functools.lru_cache(maxsize=None)
def digital_numbers(name):
    """The scene's digital numbers: most below 400, so that a good part lies under the noise; 2 % fill (0); 65535 in the second
    and in the last strip.  Asserts each property on the restatement with every table present."""
    samples = SAMPLES[name]
    gx, gy, lpb, last = launch(L, samples)
    assert (gx, gy, lpb, last) == (3, 3, 32, 11) and -(-samples // 4) == 525 and 525 % 256 and last % source_define("XSW_CAL_LINES") == 3
    assert (samples % 4 == 0) == (name != "elem")
    rng = np.random.default_rng(2410)
    dn = rng.integers(1, 400, (L, 2100)).astype(np.uint16)
    dn[rng.uniform(size=dn.shape) < 0.02] = 0
    dn[40, 1001], dn[40, 1002], dn[70, 7], dn[74, 2098] = 65535, 65535, 65535, 65535
    dn = np.ascontiguousarray(dn[:, :samples])
    g = grids(samples)
    want = cref.calibrate(dn, g["lut"], **tables(samples, TABLES))
    A = cref.blend(g["lut"], np.arange(float(L)), np.arange(float(samples)))
    assert 1001 % 4 and (np.abs(A[:, 1002] - A[:, 1001]) > 100.0).all() and (np.abs(A[:, 1001] - A[:, 1000]) < 0.2).all()
    Na = cref.blend(g["azimuth"], np.arange(float(L)), np.arange(float(samples)))
    assert 10 // 4 == 11 // 4 and (Na[11] - Na[10] > 0.25).all()
    fill, neg, top = dn == 0, want["sigma0"] < 0, dn == 65535
    assert fill.mean() >= 0.01 and neg.mean() >= 0.01 and np.isnan(want["sigma0"][fill]).all() and not np.isnan(want["sigma0"][~fill]).any()
    for a, b in ((lpb, 2 * lpb), (L - last, L)):     # the second strip, the last strip
        assert fill[a:b].any() and neg[a:b].any() and top[a:b].any(), (a, b)
    assert 0.5 < want["valid"].mean() < 0.97 and not want["valid"][fill].any() and not want["valid"][neg].any()
    if name == "f32":
        dn = dn.astype(np.float32)
    dn.setflags(write=False)
    return dn


@functools.lru_cache(maxsize=None)
def case(name, combo=TABLES, dtype="float32", fill=0):
    """The restatement's dict(sigma0, nesz, incidence, valid) for scene `name` with the tables of `combo` present."""
    samples = SAMPLES[name]
    out = cref.calibrate(digital_numbers(name), grids(samples)["lut"], fill=fill, dtype=np.dtype(dtype).type, **tables(samples, combo))
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out
