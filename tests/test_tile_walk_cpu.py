"""The tile walk of the inversion kernels (csrc/xsw_tilewalk.hpp) on the host: a stand-alone program built from the header with
the host compiler (tests/tile_walk_c/tile_walk_main.cpp; nothing is added to libxsw.so) against the Python restatement
tests/tile_walk_ref.py, and the properties the kernels rely on: every tile exactly once, the leftover columns shared evenly,
every XCD's own columns contiguous, and today's walk unchanged where the strips divide by 8."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tile_walk_ref as ref
from conftest import REPO

STRIPS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 312, 313, 319)
LINE_GROUPS = (1, 2, 7, 8, 9, 63, 5000)
PAIRS = [(s, lg) for s in STRIPS for lg in LINE_GROUPS]


@pytest.fixture(scope="module")
def program_maps(tmp_path_factory):
    """{(strips, lg): (map by (xcd, y, g), map by linear slot number)} as the compiled header gives them: one build, one run."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("tile_walk") / "tile_walk"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "xsarsea_amd", "csrc"), "-o", str(exe),
                    os.path.join(REPO, "tests", "tile_walk_c", "tile_walk_main.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for p in PAIRS for v in p], check=True, capture_output=True)
    flat = np.frombuffer(r.stdout, dtype=np.int32)
    out, k = {}, 0
    for s, lg in PAIRS:
        n = 8 * ref.cols_per_xcd(s) * lg * 2
        out[(s, lg)] = (flat[k:k + n].reshape(8, ref.cols_per_xcd(s), lg, 2), flat[k + n:k + 2 * n].reshape(-1, 2))
        k += 2 * n
    assert k == flat.size
    return out


def test_restatement_scalar_and_vectorised_agree():
    for s, lg in ((1, 1), (7, 9), (9, 2), (17, 8), (23, 63)):
        m = ref.tile_map(s, lg)
        for xcd in range(8):
            for y in range(ref.cols_per_xcd(s)):
                for g in range(lg):
                    t = ref.tile_walk(s, lg, xcd, y, g)
                    assert tuple(m[xcd, y, g]) == (t if t is not None else (-1, -1)), (s, lg, xcd, y, g)


@pytest.mark.parametrize("strips", STRIPS)
def test_header_against_restatement(program_maps, strips):
    for lg in LINE_GROUPS:
        got, got_linear = program_maps[(strips, lg)]
        want = ref.tile_map(strips, lg)
        assert np.array_equal(got, want), (strips, lg)
        # linear slot number b: xcd = b % 8, then y outer, g inner
        assert np.array_equal(got_linear.reshape(ref.cols_per_xcd(strips), lg, 8, 2), want.transpose(1, 2, 0, 3)), (strips, lg)


@pytest.mark.parametrize("strips", STRIPS)
def test_walk_properties(program_maps, strips):
    base, rem = divmod(strips, 8)
    for lg in LINE_GROUPS:
        m = program_maps[(strips, lg)][0]
        has = m[..., 0] >= 0
        assert np.array_equal(has, m[..., 1] >= 0)
        # a bijection onto the strips x lg tiles
        tiles = m[has].astype(np.int64)
        assert tiles[:, 0].max() < strips and tiles[:, 1].max() < lg
        ids = tiles[:, 0] * lg + tiles[:, 1]
        assert ids.size == strips * lg and np.array_equal(np.sort(ids), np.arange(strips * lg)), (strips, lg)
        # no XCD takes more than its columns and its share of the leftover tiles
        per_xcd = has.reshape(8, -1).sum(axis=1)
        assert per_xcd.max() <= base * lg + ref.share(strips, lg), (strips, lg, per_xcd)
        # with nothing left over the walk is the one before the sharing
        if rem == 0:
            assert np.array_equal(m, ref.old_tile_map(strips, lg)), (strips, lg)
        # every XCD's own columns: contiguous, whole, line groups in order
        for xcd in range(8):
            own = m[xcd, :base]
            assert np.array_equal(own[..., 0], np.broadcast_to(xcd * base + np.arange(base)[:, None], (base, lg)))
            assert np.array_equal(own[..., 1], np.broadcast_to(np.arange(lg)[None, :], (base, lg)))
        # the leftover row: each XCD's share is one contiguous run of leftover tiles, in XCD order, at the front of its row
        if rem:
            left = m[:, base].astype(np.int64)
            t = np.where(left[..., 0] >= 0, (left[..., 0] - 8 * base) * lg + left[..., 1], -1)
            q, n_left = ref.share(strips, lg), rem * lg
            for xcd in range(8):
                lo, hi = min(xcd * q, n_left), min((xcd + 1) * q, n_left)
                assert np.array_equal(t[xcd, :hi - lo], np.arange(lo, hi)) and (t[xcd, hi - lo:] < 0).all(), (strips, lg, xcd)
