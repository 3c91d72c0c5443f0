"""CPU: the parts of bench.py's command line that run before any GPU call (--steps / --warmup checks, --dump-outputs)."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")


def test_dump_outputs_finite_pixels_whole_and_sampled(tmp_path):
    """Up to DUMP_MAX_PIXELS finite pixels are written whole, in raster order (complex64 -> float32 [..., 2]); a pixel that is
    not finite in ANY output is left out of all of them.  Above DUMP_MAX_PIXELS finite pixels: DUMP_MAX_PIXELS of them, the
    same in every call; float64 stays float64; every value written is finite."""
    re = torch.arange(12.0).reshape(3, 4)
    co = torch.complex(re, -re)
    co[0, 1] = complex(float("nan"), 0.0)
    dual = torch.complex(re + 100, re)
    dual[2, 3] = complex(0.0, float("inf"))
    bench.dump_outputs(str(tmp_path / "s"), {"co": co, "dual": dual})
    keep = np.ones(12, bool)
    keep[[1, 11]] = False
    s_co, s_dual = np.load(tmp_path / "s" / "co.npy"), np.load(tmp_path / "s" / "dual.npy")
    assert s_co.dtype == np.float32 and s_co.shape == s_dual.shape == (10, 2)
    assert np.array_equal(s_co[:, 0], np.arange(12.0)[keep]) and np.array_equal(s_co[:, 1], -np.arange(12.0)[keep])
    assert np.array_equal(s_dual[:, 0], np.arange(12.0)[keep] + 100)

    n = bench.DUMP_MAX_PIXELS + 4097
    big = torch.arange(n, dtype=torch.float64)
    big[::1000] = float("nan")
    bench.dump_outputs(str(tmp_path / "a"), {"big": big})
    bench.dump_outputs(str(tmp_path / "b"), {"big": big})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_MAX_PIXELS,) and np.array_equal(a, b)
    assert np.isfinite(a).all() and np.all(np.diff(a) > 0) and a[-1] < n  # distinct, raster order (values = flat index)
    assert not np.any(a.astype(np.int64) % 1000 == 0)


def test_bench_rejects_steps_below_one():
    """`ms_per_step` is the time of one of --steps timed steps: zero steps is refused before any GPU call."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""
