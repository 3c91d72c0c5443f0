"""CPU: the exact reference and the adjudicator of tests/db_f32_ref.py, which tests/test_gpu_db_f32.py holds the kernels' to_db(float)
to on every float32 argument.  numpy's float64 log10 rounded to float32 stands in for the device here: over one binade it must
pass; with three arguments nudged to the neighbouring float32, and with numpy's own float32 log10, it must fail."""
import decimal

import numpy as np
import pytest

import db_f32_ref as ref


@pytest.fixture(scope="module")
def binade():
    """x over [2**-7, 2**-6) and the stand-in device value 10f * fl32(log10(float64(x + 1e-15f)))."""
    x = ref.as_f32(np.arange(ref.BINADE_2M7, ref.BINADE_2M7 + (1 << 23), dtype=np.uint32))
    got, _ = ref.predict_np(x)
    x.setflags(write=False)
    got.setflags(write=False)
    return x, got


def test_float64_log10_rounded_once_passes(binade):
    x, got = binade
    undecided = ref.near_boundary(ref.BINADE_2M7)
    rep = ref.check(x, got, "[2**-7, 2**-6)")
    print(ref.summary("[2**-7, 2**-6), numpy float64 log10", rep))
    assert 10 <= undecided.size <= 100 and rep.judged == undecided.size, "the filter's share of undecided arguments is ~25 per binade"
    assert not rep.wrong, rep.wrong[:5]
    closest = min(ref.exact_log10(float(v)).dist for v in ref.as_f32(undecided))
    print(f"closest to its boundary: {closest / 1e-15:.3g} x 1e-15 |L|")
    assert closest > 1e-17, "a logarithm of a float32 is no rounding boundary"


@pytest.mark.parametrize("where", [0, 12345, (1 << 23) - 1])
def test_a_value_off_by_one_float32_fails(binade, where):
    """One argument's value nudged to the next float32 (an ordinary argument, far from a boundary): not a double rounding."""
    x, got = binade
    for direction in (np.float32(np.inf), -np.float32(np.inf)):
        bad = got.copy()
        bad[where] = np.nextafter(bad[where], direction)
        rep = ref.check(x, bad)
        assert len(rep.wrong) == 1 and f"0x{int(ref.as_bits(x)[where]):08X}" in rep.wrong[0] and not rep.doubles


def test_three_nudged_arguments_fail(binade):
    x, got = binade
    bad = got.copy()
    for k in (7, 4_000_000, 8_000_000):
        bad[k] = np.nextafter(bad[k], np.float32(0))
    assert len(ref.check(x, bad).wrong) == 3


def test_the_other_neighbour_fails_away_from_the_boundary(binade):
    """10f * l for the other neighbour l of the logarithm is accepted only within ALLOW of the boundary: at the near-boundary
    arguments of the binade it is a double rounding for those within ALLOW, wrong for the others.  (Where |10 l| >= 16 the
    product's ulp is 16 ulp(l) and 10f * l can be the same float32 for both neighbours: those are equal to E.)"""
    hard = ref.as_f32(ref.near_boundary(ref.BINADE_2M7))
    ex = [ref.exact_log10(float(v)) for v in hard]
    other = np.array([ref.TEN32 * e.other for e in ex], dtype=np.float32)
    merged = np.array([ref.TEN32 * e.other == ref.TEN32 * e.rn for e in ex])
    dists = np.array([e.dist for e in ex])
    rep = ref.adjudicate(ref.as_bits(hard), other)
    assert len(rep.doubles) == int((~merged & (dists <= ref.ALLOW)).sum())
    assert len(rep.wrong) == int((~merged & (dists > ref.ALLOW)).sum()) > 10


def test_a_double_rounding_within_the_allowance_is_legitimate(monkeypatch):
    """The verdict's other branch, on a widened allowance: the argument of the binade nearest its boundary, given the other
    neighbour, is a double rounding when ALLOW covers its distance and wrong when it does not."""
    hard = ref.near_boundary(ref.BINADE_2M7)
    dist, p = min((ref.exact_log10(float(v)).dist, int(b)) for v, b in zip(ref.as_f32(hard), hard))
    got = ref.TEN32 * ref.exact_log10(float(ref.as_f32(p))).other
    monkeypatch.setattr(ref, "ALLOW", dist * 1.01)
    assert ref.judge(p, got).kind == "double"
    monkeypatch.setattr(ref, "ALLOW", dist * 0.99)
    assert ref.judge(p, got).kind == "wrong"
    assert ref.judge(p, ref.TEN32 * ref.exact_log10(float(ref.as_f32(p))).rn).kind == "equal"


def test_numpy_float32_log10_fails(binade):
    """numpy's own float32 log10 (faithful, not correctly rounded) as the device: the test catches it."""
    x, _ = binade
    with np.errstate(all="ignore"):
        got = ref.TEN32 * np.log10(ref.y_of(x))
    pred, ok = ref.predict_np(x)
    differ = ok & (got != pred)
    print(f"numpy float32 log10: {int(differ.sum())} of {x.size} arguments differ from the correctly rounded value")
    assert differ.any()
    some = np.flatnonzero(differ)[:50]
    rep = ref.adjudicate(ref.as_bits(x)[some], got[some])
    assert len(rep.wrong) == some.size and not rep.doubles


def test_expected_on_the_specials():
    f = lambda p: ref.expected(p)
    assert ref.as_f32(0xA6901D7D) == -ref.EPS32 and ref.as_f32(0x3F800000) == 1.0
    eps_db = ref.TEN32 * ref.exact_log10(float(ref.EPS32)).rn  # 10 log10(1e-15f): -150 and a bit
    assert abs(float(eps_db) + 150.0) < 1e-4
    for p in (0x00000000, 0x80000000, 0x00000001, 0x00800000):  # below half an ulp of 1e-15f: y == 1e-15f
        assert f(p) == eps_db
    assert f(0xA6901D7D) == -np.inf                         # y == 0
    assert f(0xA6901D7C) == ref.TEN32 * np.float32(-73 * np.log10(2.0))   # y == 2**-73, the smallest positive y
    assert float(ref.y_of(ref.as_f32(0xA6901D7C))) == 2.0 ** -73 and float(ref.y_of(ref.as_f32(0xA6901D7E))) == -(2.0 ** -73)
    assert np.isnan(f(0xA6901D7E)) and np.isnan(f(0xBF800000)) and np.isnan(f(0x7FC00000)) and np.isnan(f(0xFFFFFFFF))
    assert f(0x7F800000) == np.inf
    assert f(0x7F7FFFFF) == ref.TEN32 * np.float32(np.log10(float(np.finfo(np.float32).max)))
    assert f(0x3F800000) == 0.0 and not np.signbit(f(0x3F800000))   # y == 1: the logarithm is exact
    # RN32 itself, against a 100-digit logarithm of a value whose float64 log10 is unremarkable
    L = decimal.Context(prec=100).log10(decimal.Decimal(0.02))
    e = ref.exact_log10(0.02)
    assert e.rn == np.float32(float(L)) and decimal.Decimal(float(e.lo)) < L < decimal.Decimal(float(e.hi)) and e.hi == np.nextafter(e.lo, np.float32(0))


def test_hard_arguments():
    h = ref.hard_arguments()
    bits = ref.as_bits(h)
    assert set(ref.SPECIAL_PATTERNS) <= set(bits.tolist())
    for e in (-74, -1, 0, 127):
        for d in (-1, 0, 1):
            assert ((e + 127) << 23) + d in bits
    n = [ref.near_boundary(b).size for b in (ref.BINADE_2M7, ref.BINADE_HALF, ref.BINADE_ONE)]
    print(f"hard arguments: {h.size}; near-boundary arguments per binade {n}")
    assert all(5 <= k <= 100 for k in n) and h.size == len(ref.SPECIAL_PATTERNS) + 3 * 202 + sum(n)
    rep = ref.check(h, ref.predict_np(h)[0])
    assert not rep.wrong, rep.wrong[:5]
