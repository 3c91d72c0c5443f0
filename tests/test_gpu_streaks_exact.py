"""k_streaks_peak on the MI355X, held to the bit on the hand-built histograms of tests/streak_cases.py: exact ties across lanes and
across a lane's strides, the unique maximum at every edge of the lanes' ownership, window counts around a workgroup, and the
values at which a comparison or a sum can go wrong.  What each case can catch is stated in streak_cases.py; its expected values
are the restatement's (tests/streaks_ref.py), whose own properties tests/test_streaks_cpu.py asserts without a GPU."""
import numpy as np
import pytest

import gradients_ref as ref
import streak_cases as sc
from test_gpu_streams import torch  # noqa: F401  (fixture)
from util import bits_equal
from xsarsea_amd import gradients, streaks

pytestmark = pytest.mark.gpu
DIMS = ("c", "line", "sample", "angles")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_peak_exact(s, want, table, what):
    """index equal at every window; weight, used_ratio bit-equal (NaN included); angle bit-equal to table[index]."""
    index = host(s.index)
    assert index.dtype == np.int32 and index.shape == want["index"].shape, what
    np.testing.assert_array_equal(index, want["index"], err_msg=what)
    assert bits_equal(host(s.weight), want["weight"]), f"{what}: weight {host(s.weight)} != {want['weight']}"
    assert bits_equal(host(s.used_ratio), want["used_ratio"]), f"{what}: used_ratio"
    assert bits_equal(host(s.angle), table[want["index"]]), f"{what}: angle"
    assert bits_equal(host(s.angle), want["angle"]), f"{what}: angle against the restatement's"


@pytest.mark.parametrize("name", sc.names())
def test_peak_of_hand_built_histograms_bit_for_bit(name, torch):
    c = sc.cases()[name]
    nl, ns = c.weight.shape[1:3]
    bins = ref.angles_bins(c.n)
    table = bins + np.pi / 2
    line, sample = np.arange(nl) * 10.0, np.arange(ns) * 10.0
    h = gradients.GradientsHistogram(c.weight, c.ratio, bins, line, sample, DIMS)
    assert_peak_exact(streaks.streaks_direction(h, smooth=c.smooth), c.want, table, name + " (numpy)")
    hd = gradients.GradientsHistogram(torch.from_numpy(c.weight.copy()).cuda(), torch.from_numpy(c.ratio.copy()).cuda(), bins, line, sample, DIMS)
    sd = streaks.streaks_direction(hd, smooth=c.smooth)
    assert sd.index.is_cuda and sd.weight.is_cuda
    assert_peak_exact(sd, c.want, table, name + " (device tensors)")
