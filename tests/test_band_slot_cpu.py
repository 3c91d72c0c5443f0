"""The table offsets a pixel's slot carries through k_invert_band's passes (csrc/xsw_bandslot.hpp) on the host: a stand-alone
program built from the header with the host compiler (tests/band_slot_c/band_slot_main.cpp; nothing is added to libxsw.so)
against the plain formulas in Python's unbounded integers:

    slice0 = phi_pad * 8 * n_w * i_inc                         bytes into the co-pol table   [n_inc][n_w][phi_pad] doubles
    inv0   = 2 * phi_pad * (i_inc * 2048 + bin)                bytes into the inverse table  [n_inc][2048][phi_pad] uint16
    inv1   = 2 * phi_pad * (i_inc * 2048 + bin_hi), or the reserved value when bin_hi == 2048 (no threshold above s + d)

on the seven LUT shapes of the forced-route tests, the default 501 x 499 x 181 and shapes at the limits the band kernels are
gated by (csrc/xsw_lutplan.hpp: band_mul24, co_off32, inv_ok), restated in `gates` below."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lut_tables_ref as ltr
import route_geometry as rg
from conftest import REPO

BINS = ltr.INV_BINS
NONE = 0xFFFFFFFF

# (n_inc, n_w, n_phi)
SHAPES = {name: (g["n_inc"], g["n_w"], g["n_phi"]) for name, g in rg.GEOMETRIES.items()}
SHAPES["default"] = (501, 499, 181)
# at the gates: the most slices the 24-bit bin number allows, on the widest table that keeps the inverse table below 4 GB;
# the most table rows (n_inc * n_w) 24 bits hold, on the widest table that keeps the co-pol table below 4 GB; the most directions
SHAPES["most_slices"] = (8190, 512, 128)
SHAPES["most_rows"] = (512, 32767, 32)
SHAPES["most_directions"] = (2, 64, 65535)


def gates(n_inc, n_w, n_phi):
    """What a table must meet for the band kernels to run on it (xsw_lutplan.hpp / xsw_plan.hpp), as far as these offsets go."""
    g = ltr.geometry(n_inc, n_w, n_phi)
    mul24 = n_inc * n_w <= 0xFFFFFF and (n_inc + 1) * BINS <= 0xFFFFFF and g.ppad * 8 <= 0xFFFFFF
    co_off32 = (n_inc * n_w + 260) * g.ppad * 8 < 1 << 32
    return mul24 and co_off32 and g.inv_ok and n_w < 32768 and n_phi < 65536


def probes(n_inc):
    """(i_inc, bin, bin_hi): first, second, middle and last slice x bin 0, 1, the middle, the last x a bin above, the last one,
    none (2048)."""
    out = []
    for i in sorted({0, min(1, n_inc - 1), n_inc // 2, n_inc - 1}):
        for b in (0, 1, BINS // 2, BINS - 1):
            for bh in sorted({min(b + 1, BINS - 1), BINS - 1, BINS}):
                out.append((i, b, bh))
    return out


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """{shape name: uint32 [probes][6]} as the compiled header gives them: one build, one run."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("band_slot") / "band_slot"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "xsarsea_amd", "csrc"), "-o", str(exe),
                    os.path.join(REPO, "tests", "band_slot_c", "band_slot_main.cpp")], check=True)
    args = []
    for name, (n_inc, n_w, n_phi) in SHAPES.items():
        ppad = ltr.geometry(n_inc, n_w, n_phi).ppad
        for i, b, bh in probes(n_inc):
            args += [ppad, n_w, i, b, bh]
    r = subprocess.run([str(exe)] + [str(v) for v in args], check=True, capture_output=True)
    flat = np.frombuffer(r.stdout, dtype=np.uint32).reshape(-1, 6)
    out, k = {}, 0
    for name, (n_inc, _, _) in SHAPES.items():
        n = len(probes(n_inc))
        out[name] = flat[k:k + n]
        k += n
    assert k == len(flat)
    return out


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_pass_the_gates_and_limit_shapes_sit_on_them(name):
    n_inc, n_w, n_phi = SHAPES[name]
    assert gates(n_inc, n_w, n_phi)
    if name == "most_slices":
        assert not gates(n_inc + 1, n_w, n_phi) and not gates(n_inc, n_w + 1, n_phi) and not gates(n_inc, n_w, n_phi + 1)
    if name == "most_rows":
        assert not gates(n_inc, n_w + 1, n_phi) and not gates(n_inc + 1, n_w, n_phi) and not gates(n_inc, n_w, n_phi + 4)
    if name == "most_directions":
        assert not gates(n_inc, n_w, n_phi + 1)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_packed_offsets_against_the_plain_formulas(packed, name):
    n_inc, n_w, n_phi = SHAPES[name]
    g = ltr.geometry(n_inc, n_w, n_phi)
    pr = probes(n_inc)
    assert {p[0] for p in pr} >= {0, n_inc - 1} and {p[1] for p in pr} >= {0, BINS - 1} and {p[2] for p in pr} >= {BINS - 1, BINS}
    for (i, b, bh), got in zip(pr, packed[name].tolist()):
        slice0, inv0, inv1, capped, row1, none = got
        assert none == NONE
        want_slice0 = g.ppad * 8 * n_w * i
        want_inv0 = 2 * g.ppad * (i * BINS + b)
        want_inv1 = 2 * g.ppad * (i * BINS + bh) if bh < BINS else NONE
        # the plain values fit 32 bits and stay inside their tables (a whole row of directions still follows the offset)
        assert want_slice0 + g.ppad * 8 * n_w <= g.n_body * 8 < 1 << 32
        assert want_inv0 + 2 * g.ppad <= g.inv_n * 2 < 1 << 32
        assert (slice0, inv0, inv1) == (want_slice0, want_inv0, want_inv1), (name, i, b, bh)
        # the reserved value is no offset: every real one is even and below the table's size
        assert inv0 != NONE and inv0 % 2 == 0
        if bh < BINS:
            assert inv1 != NONE and inv1 % 2 == 0 and inv1 + 2 * g.ppad <= g.inv_n * 2
        # the pass: a row above the band or not, and a readable offset either way
        assert capped == (1 if bh < BINS else 0)
        assert row1 == (want_inv1 if bh < BINS else want_inv0)
