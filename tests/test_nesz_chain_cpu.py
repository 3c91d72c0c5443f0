"""CPU: the cases, the reference, the restatement and the bound that tests/test_gpu_nesz_chain.py holds the noise flattening to
(tests/nesz_cases.py, tests/nesz_chain_ref.py).  Every case is built, which runs the assertions of what it is for; the plain
float64 restatement of the kernels lies within the bound with its R term left out; the oracle's polyfit route agrees with the
longdouble reference where numpy does not raise; and each of the seven wrong variants of the restatement moves the result by more
than 100 times the bound at the cases meant to catch it, for float32 rasters as well as float64 ones."""
import numpy as np
import pytest

import nesz_cases as nc
import nesz_chain_ref as ref

from oracle import crosspol

DTYPES = [np.float64, np.float32]
FAMILIES = {"samples": [f"samples_{s}" for s in nc.SAMPLES], "lines": [f"lines_{l}x{s}" for s in nc.LINES_S for l in nc.LINES],
            "branch": list(nc.BRANCH), "tall": ["tall_blocks"]}


def _names(family, dtype):
    return FAMILIES[family] + (list(nc.F32_ONLY) if family == "branch" and dtype == np.float32 else [])


def test_the_restated_launch_reads_the_kernels_constants():
    assert ref.constants() == (4, 256, 2, 2)  # XSW_NESZ_LINES, XSW_NESZ_THREADS, XSW_NESZ_F32_GROUP, XSW_NESZ_EV: the case tables assume them
    assert [ref.nesz_blocks(l, 130) for l in (9, 15, 17, 33)] == [(2, 5, 4), (2, 8, 7), (3, 6, 5), (5, 7, 5)]
    assert ref.nesz_blocks(*nc.TALL) == (15, 10, 7) and ref.nesz_blocks(11, 2049) == (2, 6, 5)
    assert ref.nesz_blocks(20000, 20000)[1] == 385 and ref.nesz_blocks(1537, 4101)[1] == 8  # the workload; the older tests' raster
    assert set(nc.EXPECT_SAMPLES) == set(nc.SAMPLES) and set(nc.EXPECT_LINES) == set(nc.LINES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_cases_build_and_the_restatement_lies_within_the_bound_without_r(family, dtype):
    """Building a case asserts its property (tests/nesz_cases.py).  Then: the restatement against the reference within the bound
    WITHOUT its R term -- the float64 row for both raster types, the restatement's pair being numpy's float64 one -- so the
    other terms are seen to be honest: an error of the restatement is not simply handed to the device as allowance."""
    worst = (0.0, "")
    for name in _names(family, dtype):
        c = nc.case(name, dtype)
        ratio, at, n, _err = ref.worst_ratio(c.rst.out, c.ref, ref.bound(c.ref, np.float64))
        worst = max(worst, (ratio, name))
        print(f"{name} {np.dtype(dtype).name}: {n} of {c.noise.size} pixels finite, R at worst {c.R.max():.2e}; restatement error / bound without R "
              f"{ratio:.3f} at {at}")
        assert ratio <= 1.0, (name, ratio, at)
        if family == "tall":  # (built once per raster type: its oracle check rides along)
            err = _oracle_error(c)
            print(f"{name} {np.dtype(dtype).name}: oracle against the reference {err:.2e}")
            assert err <= ORACLE_TOL[np.dtype(dtype)], (name, err)
    print(f"{family} {np.dtype(dtype).name}: worst {worst[0]:.3f} ({worst[1]})")


def _oracle_error(c):
    """The largest relative error of oracle.crosspol.nesz_flattening against the reference (None where numpy raises; 0.0 on an
    all-NaN result); NaN positions equal."""
    try:
        with np.errstate(all="ignore"):
            got = np.asarray(crosspol.nesz_flattening(c.noise, c.inc), dtype=np.float64)
    except np.linalg.LinAlgError:
        return None
    assert np.array_equal(np.isnan(got), np.isnan(c.ref.out)), c.name
    finite = np.isfinite(c.ref.out)
    if not finite.any():
        return 0.0
    # two_samples: the oracle's rounding of y (float32 for float32 rasters) reaches a column through sum |h_i| <= kappa, up to
    # 600 on the lines that extrapolate 25 degrees from two adjacent samples: the tolerance is per unit of kappa there
    scale = ref.kappa(c.ref) if c.name == "two_samples" else 1.0
    return float((ref.rel_error(got, c.ref) / scale)[finite].max())


ORACLE_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 2e-6}


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_oracle_agrees_with_the_reference_where_numpy_does_not_raise(dtype):
    """oracle.crosspol.nesz_flattening (numpy's SVD polyfit; float32 rasters in float32) against the longdouble reference: 1e-12 for
    float64 rasters, 2e-6 for float32 ones -- loose on purpose (measured 9.6e-15 and 1.1e-6): a check of the reference's
    branches, not of the kernel.  numpy raises on a NaN abscissa among the fitted samples (nan_inc_column).  (tall_blocks: with
    its build, in test_cases_build_...)"""
    raised, worst = [], (0.0, "")
    for name in nc.names(dtype):
        c = nc.case(name, dtype)
        err = _oracle_error(c)
        if err is None:
            raised.append(name)
            continue
        worst = max(worst, (err, name))
        print(f"{name} {np.dtype(dtype).name}: oracle against the reference {err:.2e}")
        assert err <= ORACLE_TOL[np.dtype(dtype)], (name, err)
    print(f"{np.dtype(dtype).name}: worst {worst[0]:.2e} ({worst[1]})")
    assert raised == ["nan_inc_column"]


# variant: the cases meant to catch it
CATCHES = {1: ["samples_129", "samples_512", "lines_5x130", "lines_7x131", "lines_9x130", "lines_15x131", "lines_17x130", "lines_33x131"],
           2: ["samples_3", "samples_257", "lines_2x130", "lines_8x131", "nan_noise_line"],
           3: ["samples_3", "samples_63", "samples_65", "samples_513", "lines_4x131", "two_samples"],
           4: ["samples_1023", "samples_1025", "samples_2049"],
           5: ["samples_3", "samples_64", "samples_1025", "lines_16x130", "nan_noise_pair"],
           6: ["samples_511", "samples_512", "samples_513", "samples_2049"],
           7: ["samples_3", "samples_65", "samples_257", "lines_2x131", "lines_33x131", "two_samples"]}


@pytest.mark.parametrize("variant", sorted(ref.MUTANTS))
def test_a_wrong_variant_is_caught(variant):
    """restate(mutate=variant) against the plain restatement, in units of the bound the device is held to (R term included): more
    than 100 on at least one pixel of EVERY case named for the variant, float64 and float32 rasters."""
    assert set(CATCHES) == set(ref.MUTANTS)
    for dtype in DTYPES:
        for name in CATCHES[variant]:
            c = nc.case(name, dtype)
            wrong = ref.restate(c.noise, c.inc, mutate=variant).out
            both = np.isfinite(wrong) & np.isfinite(c.ref.out)
            assert both.any(), (variant, name)
            with np.errstate(all="ignore"):
                moved = np.where(both, np.abs(wrong - c.rst.out) / np.abs(c.ref.out.astype(np.float64)) / c.bound, 0.0)
            at = np.unravel_index(int(np.argmax(moved)), moved.shape)
            rel = float(abs(wrong[at] - c.rst.out[at]) / abs(c.rst.out[at]))
            print(f"variant {variant} ({ref.MUTANTS[variant]}), {name} {np.dtype(dtype).name}: moves the result by {rel:.2e} relative = "
                  f"{moved[at]:.3g} bounds at {tuple(int(k) for k in at)}; {int((moved > 100).sum())} of {int(both.sum())} pixels beyond 100 bounds")
            assert moved[at] > 100.0, (variant, name, np.dtype(dtype).name, moved[at])
