"""CPU: the exact reference and the bounds of tests/nesz_ref.py, which tests/test_gpu_nesz_pair.py holds the noise flattening's
log10 / exp10 pair to.  The plain float64 restatement and the oracle's polyfit lie within a few units of 2**-52 * max(1, |y|) of
the exact value; the header's series, ported to numpy, lies within the float64 bound, and with one coefficient off, or with the
library's float32 functions in the pair's place, it does not."""
import decimal

import numpy as np
import pytest

import nesz_ref as ref

from oracle import crosspol

UNIT = 2.0 ** -52


def _units(err, dtype):
    """An error raster in units of 2**-52 * max(1, |y|), over the compared outputs."""
    with np.errstate(all="ignore"):
        u = err / (UNIT * np.maximum(1.0, np.abs(ref.exact(dtype).y)))
    return u[ref.compared(dtype)]


def test_arguments():
    for dtype, kmax in ((np.float64, 1023), (np.float32, 120)):
        v, kinds = ref.arguments(dtype)
        fi = np.finfo(dtype)
        normal = np.array([k == "normal" for k in kinds])
        assert v.dtype == dtype and v.size % 4 == 3 and v.size == len(kinds)
        assert np.all((v[normal] >= fi.tiny) & np.isfinite(v[normal])) and np.unique(v[normal]).size == normal.sum()
        assert [k for k in kinds if k != "normal"][:5] == list(ref.SPECIALS)
        rest = v[~normal]
        assert rest[0] == 0 and rest[1] < 0 and np.isposinf(rest[2]) and np.isnan(rest[3]) and np.all((rest[4:] > 0) & (rest[4:] < fi.tiny))
        m, e = np.frexp(v[normal].astype(np.float64))
        assert (m < np.sqrt(0.5)).any() and (m >= np.sqrt(0.5)).any(), "both sides of the mantissa fold"
        assert e.min() <= -kmax + 2 and e.max() >= kmax
        print(f"{np.dtype(dtype).name}: {int(normal.sum())} finite normal arguments, {v.size} lines")
    t = ref.exact(np.float64).t
    assert (np.abs(t) < 300).any() and (np.abs(t) >= 300).any(), "both sides of nesz_exp10's hand-over to the library"


def test_exact_is_v_to_a_power():
    """out = 10**-0.1 * v ** (x / 70 + 1 / 2), evaluated another way (at x = 35 it is v / 10**0.1), compared through the float64 pair."""
    c = decimal.Context(prec=120)
    v, kinds = ref.arguments(np.float64)
    ex = ref.exact(np.float64)
    for i in list(range(0, v.size, 97)) + [kinds.index("denormal")]:
        if kinds[i] not in ("normal", "denormal"):
            continue
        for s, x in enumerate(ref.INC):
            want = c.multiply(c.power(decimal.Decimal(float(v[i])), c.divide(decimal.Decimal(int(x) + 35), decimal.Decimal(70))),
                              c.power(decimal.Decimal(10), decimal.Decimal("-0.1")))
            if not np.isfinite(ex.hi[i, s]) or ex.hi[i, s] < np.finfo(np.float64).tiny:
                continue
            got = c.add(decimal.Decimal(float(ex.hi[i, s])), decimal.Decimal(float(ex.lo[i, s])))
            # hi + lo is a pair of float64: lo is a denormal, resolved to 4.9e-324, where hi < 1e-292 (the bounds there are ~1e-12)
            assert abs(c.divide(c.subtract(got, want), want)) < decimal.Decimal(1e-25 + 1e-323 / ex.hi[i, s]), (i, s)


def test_restatement_and_oracle_lie_within_a_few_units():
    r = _units(ref.restatement_error(np.float64), np.float64)
    noise, inc = ref.rasters(np.float64)
    with np.errstate(all="ignore"):
        flat = crosspol.nesz_flattening(noise, inc)
    ref.check_lines(flat, np.float64, "oracle")
    o = _units(ref.rel_error(flat, ref.exact(np.float64)), np.float64)
    print(f"float64, in units of 2**-52 max(1, |y|): restatement at worst {r.max():.3f}, the oracle's polyfit at worst {o.max():.3f}")
    assert r.max() < 2 and o.max() < 4


def test_outputs_outside_the_normal_range_exist_and_are_not_nan():
    ex, out = ref.exact(np.float64), ref.restate(ref.arguments(np.float64)[0])
    beyond = np.isinf(ex.hi) | (ex.hi < np.finfo(np.float64).tiny)
    assert np.isinf(ex.hi).any() and (ex.hi < np.finfo(np.float64).tiny).any()
    assert not np.isnan(out[beyond]).any()


def _series(log_coef=ref.LOG_COEF, exp_coef=ref.EXP_COEF):
    v = ref.arguments(np.float64)[0]
    return ref.restate(v, log10=lambda a: ref.series_log10(a, log_coef), exp10=lambda t: ref.series_exp10(t, exp_coef))


def test_the_series_lies_within_the_float64_bound():
    got = _series()
    ref.check_lines(got, np.float64, "series")
    ratio, at, n = ref.worst_ratio(got, np.float64)
    print(f"the header's series in numpy: worst error / bound {ratio:.3f} at line {at[0]} sample {at[1]} of {n} outputs")
    assert ratio <= 1.0


@pytest.mark.parametrize("which", ["log 1/9 -> 1/8", "log cut after 1/15", "exp 1/9! -> 1/8!", "exp degree 10"])
def test_a_subtly_wrong_series_exceeds_the_bound(which):
    """(The series has slack: without its 1/21 and 1/19 terms, or at degree 11 of the exponential, it still lies within the bound
    at these arguments -- 0.40 and 0.47 of it.)"""
    lc, ec = list(ref.LOG_COEF), list(ref.EXP_COEF)
    if which == "log 1/9 -> 1/8":
        lc[lc.index(1.0 / 9.0)] = 1.0 / 8.0
    elif which == "log cut after 1/15":
        lc = lc[3:]
    elif which == "exp 1/9! -> 1/8!":
        ec[ec.index(1.0 / 362880.0)] = 1.0 / 40320.0
    else:
        ec = ec[3:]
    ratio, at, _ = ref.worst_ratio(_series(tuple(lc), tuple(ec)), np.float64)
    print(f"{which}: worst error / bound {ratio:.3g} at line {at[0]}")
    assert ratio > 1.0


def test_float32_bound_holds_a_faithful_pair_and_catches_a_wrong_constant():
    """numpy's float32 log2 / exp2 (within an ulp) in the place of v_log_f32 / v_exp_f32, in the kernel's float32 steps: within
    the float32 bound.  With 3.0104f for 3.01029995...f (3e-5 relative) it is not."""
    v, _ = ref.arguments(np.float32)

    def pair(c):
        log10 = lambda a: (np.float32(c) * np.log2(a.astype(np.float32))).astype(np.float64) / 10.0
        exp10 = lambda t: np.exp2((t * 3.321928094887362).astype(np.float32)).astype(np.float64)
        with np.errstate(all="ignore"):
            return ref.restate(v.astype(np.float64), log10=log10, exp10=exp10)

    got = pair(3.0102999566398120)
    ref.check_lines(got, np.float32, "float32 pair")
    ratio, at, n = ref.worst_ratio(got, np.float32)
    print(f"numpy's float32 log2 / exp2 as the pair: worst error / bound {ratio:.3f} at line {at[0]} sample {at[1]} of {n} outputs")
    assert ratio <= 1.0
    assert ref.worst_ratio(pair(3.0104), np.float32)[0] > 1.0
