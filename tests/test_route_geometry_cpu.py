"""CPU: the scene builder behind tests/test_gpu_route_geometry.py (tests/route_geometry.py).  The forced routes of the GPU test
have crowd rules that look at a whole wave -- 64 pixels of one line -- so the scenes must fill waves with wide windows, on every
table shape.  That is a property of the scenes and of the window geometry (tests/prune_model.py: search_window), checked here
without a GPU; the flags of the seven tables are pinned in tests/test_host_lutplan.py."""
import numpy as np
import pytest

import route_geometry as rg

# line % 4 of the lines whose waves must hold wide windows.  A window of the a-priori wind at 1.6 / 0.6 of the truth is about 45 / 85
# degrees wide whatever the table: 17 / 33 directions of a 2.5 degree axis, but 3 / 6 of the 15 and 16.4 degree axes of coarse_full
# and narrow, where only the lines at 0.3 of the truth (the disc holds the origin: every direction) can reach 8.
WIDE_LINES = {"pad4_half": (1, 2, 3), "pad4_full": (1, 2, 3), "open_half": (1, 2, 3), "tail": (1, 2, 3), "default_like": (1, 2, 3), "narrow": (3,), "coarse_full": (3,)}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(rg.GEOMETRIES))
def test_scene_is_deterministic_and_as_specified(name):
    geo = rg.GEOMETRIES[name]
    lco, lcr = rg.build_luts(name)
    assert lco.values.shape == (geo["n_inc"], geo["n_w"], geo["n_phi"]) and lcr.values.shape == (geo["n_inc"], geo["n_wcr"])
    assert np.all(np.isfinite(lco.values)) and np.all(np.diff(lcr.values, axis=1) >= 0)  # (cr_monotone: dual-pol stays on the chain)
    for dt in (np.float64, np.float32):
        a, b = rg.build_scene(name, dt), rg.build_scene(name, dt)
        assert all(_same(a[k], b[k]) for k in a), "the scene differs between two builds"
        assert a["inc"].shape == (rg.LINES, rg.SAMPLES) and a["inc"].dtype == dt and a["sco"].dtype == dt
        n = a["inc"].size
        for k in ("inc", "sco", "scr", "dsig"):
            bad = int(np.sum(~np.isfinite(a[k]) | (a[k] == 0) | (a[k] < -140)))  # (sigma0 = 0 is -150 dB)
            assert 0.02 * n < bad < 0.035 * n, (k, bad)
        bad = int(np.sum(np.isnan(a["anc"]) | (a["anc"] == 0)))
        assert 0.02 * n < bad < 0.035 * n, ("anc", bad)
        inc = a["inc"][np.isfinite(a["inc"])]
        assert inc.min() < lco.incidence[0] - 2.9 and inc.max() > lco.incidence[-1] + 2.9  # beyond both ends: first and last slice
        # every strip of 64 samples reaches below the first slice and above the last one
        for s0 in range(0, rg.SAMPLES - 63, 64):
            strip = a["inc"][0, s0:s0 + 64]
            assert np.nanmin(strip) < lco.incidence[0] and np.nanmax(strip) > lco.incidence[-1]
        # the pinned line: a-priori directions within 2 degrees of both ends of the direction axis
        z = a["anc"][rg.PINNED_LINE]
        z = z[np.isfinite(z) & (z != 0)]
        ang = np.degrees(np.angle(z)) % 360.0
        d0 = np.minimum(ang, 360.0 - ang)                                               # from phi[0] = 0
        d1 = np.abs((ang - geo["phi_last"] + 180.0) % 360.0 - 180.0)                    # from phi[-1]
        assert np.all(np.minimum(d0, d1) <= 2.0 + 1e-3)
        assert np.sum(d0 <= 2.001) > 64 and np.sum(d1 <= 2.001) > 64


@pytest.mark.parametrize("name", list(rg.GEOMETRIES))
def test_scene_fills_waves_with_wide_windows(name):
    """In the lines named by WIDE_LINES, 48 or more of the 64 pixels of every whole strip have a window of 8 directions or more
    (what XSW_ARC_MIN=8 looks at; 48 is XSW_ARC_CROWD's default, and far above XSW_B2_REFINE_MIN = 16 and XSW_B2_CROWD = 24).
    The window is prune_model's: the bound of the whole ray at the a-priori direction (at most the bisection's), then
    search_window; a pixel without a finite co-pol problem counts as narrow."""
    lco, _ = rg.build_luts(name)
    nc = rg.window_columns(lco, rg.build_scene(name, np.float64))
    strips = nc[:, :(rg.SAMPLES // 64) * 64].reshape(rg.LINES, -1, 64)
    wide = (strips >= 8).sum(axis=-1)
    print(name, "pixels of 64 with a window of >= 8 directions, by line and strip:\n", wide)
    for ln in range(rg.LINES):
        if ln % 4 in WIDE_LINES[name]:
            assert wide[ln].min() >= 48, (name, ln, wide[ln].tolist())
    # and a workgroup's four waves differ in class: the lines at the truth hold the narrowest windows, those at 0.3 of it the widest
    med = [float(np.median(nc[k::4][nc[k::4] > 0])) for k in range(4)]
    assert med[0] <= min(med[1:]) and med[0] < med[3] == max(med), med
