"""CPU: the one statement of the 4-byte grid codes (csrc/xsw_codes.hpp), compiled alone with a host C++ compiler.

What the decoder must say comes from the numpy restatements of the kernels that read the codes, never from the header:
tests/crosspol_codes_ref.py (cross_from_codes: which co-pol codes are grid codes, which entry of `sol` they name, which are
"no search ran", which are handled as XSW_CODE_NAN_RE) and tests/cost_codes_ref.py (_co_grid: grid code and flat index; cost_cr:
which cross-pol codes hold an index, and which).  The strict cross-pol rule of the expansion to winds has no numpy statement of
its own: it is the lenient one and bit 31 clear (include/xsw.h: no producer sets bit 31 of a cross-pol code but in
XSW_CODE_NAN_RE), restated here.

The two rules differ on 0x80000003 and on nothing else of the list -- at n_wcr = 40; at n_wcr = 3 index 3 is out of range for
both, so there they agree on every code."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import cost_codes_ref
import crosspol_codes_ref as cross_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE_NAN_RE, CODE_NAN, PICK_CO, NO_INDEX = cross_ref.CODE_NAN_RE, cross_ref.CODE_NAN, cross_ref.CODE_PICK_CO, cross_ref.CODE_NO_INDEX
PLANES = ((7, 5), (80, 73))  # (n_wspd, n_phi)
N_WCR = (3, 40)

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "xsw_codes.hpp"
using namespace xsw;
int main()
{
    char cmd[16];
    unsigned long long a, b, c;
    while (scanf("%15s %llu %llu %llu", cmd, &a, &b, &c) == 4) {
        if (!strcmp(cmd, "co")) {  // code, plane
            const CoCode d = co_decode((unsigned)a, (long long)b);
            printf("%d %d %d %u %u %lld\n", (int)d.nan_re(), (int)d.nan(), (int)d.grid(), d.flat(), d.sign(), d.k());
        } else if (!strcmp(cmd, "cr")) {  // code, n_wcr
            const CrCode d = cr_decode((unsigned)a);
            printf("%d %d %d %u %d %d\n", (int)d.nan_re(), (int)d.foreign(), (int)d.pick_co(), d.index(), (int)cr_index_strict(d, (long long)b),
                   (int)cr_index_lenient(d, (long long)b));
        } else if (!strcmp(cmd, "co_enc")) printf("%u\n", co_encode((unsigned)a, (unsigned)b));
        else if (!strcmp(cmd, "cr_enc")) printf("%u\n", cr_encode((unsigned)a, (unsigned)b));
        else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("g++", "clang++", "c++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, clang++, c++) on PATH")
    td = tmp_path_factory.mktemp("host_codes")
    src, exe = td / "driver.cpp", td / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "xsarsea_amd", "csrc"),
                           "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)])

    def run(lines):
        """One output line per command (cmd, a, b), as lists of ints."""
        text = "".join(f"{cmd} {a} {b} 0\n" for cmd, a, b in lines)
        out = subprocess.run([str(exe)], input=text, text=True, capture_output=True, check=True).stdout
        rows = [[int(v) for v in ln.split()] for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return rows

    return run


def co_codes(plane):
    return [0, plane - 1, plane, 0x3FFFFFFF, 0x40000000 | (plane - 1), 0x40000000 | plane, 0x80000000, 0x80000005, 0xC0000001, CODE_NAN, CODE_NAN_RE]


def cr_codes(n_wcr):
    return [0, n_wcr - 1, n_wcr, 0x3FFFFFFE, 0x40000000 | 1, 0x40000000 | n_wcr, 0x7FFFFFFE, 0x80000003, 0xBFFFFFFF, CODE_NAN_RE]


@pytest.mark.parametrize("n_w,n_phi", PLANES)
def test_copol_decode_is_what_the_numpy_readers_state(driver, n_w, n_phi):
    plane = n_w * n_phi
    codes = co_codes(plane)
    got = driver([("co", c, plane) for c in codes])
    arr = np.array(codes, np.uint32)

    # cost_codes_ref._co_grid: (grid code of this LUT, its flat index)
    p = types.SimpleNamespace(wspd_dim=np.zeros(n_w), phi_dim=np.zeros(n_phi))
    grid, flat = cost_codes_ref._co_grid(arr, p)

    # crosspol_codes_ref.cross_from_codes on tables whose entry k of `sol` ([sign][i_wspd][i_phi], flattened) is (k + 1) * 1e-6:
    # with no cross-pol search (sigma0_cr NaN) and the dual select on, a grid code returns its own `sol` entry (|wind_co| < 5),
    # XSW_CODE_NAN returns (nan, nan) with XSW_CODE_NO_INDEX, everything else is XSW_CODE_NAN_RE / (nan, 0)
    tab = dict(wspd_cr=np.arange(4.0), inc_cr_dim=np.array([30.0]), cr_lut=np.zeros((4, 1)), n_wspd=n_w, n_phi=n_phi,
               sol=((np.arange(2 * plane) + 1) * 1e-6).astype(np.complex128).reshape(2, n_w, n_phi))
    code_cr, wind = cross_ref.cross_from_codes(arr, np.full(len(codes), 30.0), np.nan, 0.1, tab, dual_select=True)

    assert list(grid) == [True, True, False, False, True, False, False, False, False, False, False]  # (the list holds both kinds)
    for c, g, ok, fl, ccr, w in zip(codes, got, grid, flat, code_cr, wind):
        nan_re, nan, is_grid, g_flat, g_sign, g_k = g
        what = f"code {c:#x} plane {plane}"
        assert nan_re == (c == CODE_NAN_RE) and nan == (c == CODE_NAN), what
        assert bool(is_grid) == bool(ok), what
        assert bool(is_grid) == bool(np.isfinite(w.real)), what
        if ok:
            assert g_flat == fl, what
            assert g_k == round(w.real * 1e6) - 1, what                  # the entry of `sol` the reference read
            assert g_k == g_flat + g_sign * plane and g_sign in (0, 1), what
            assert ccr == (NO_INDEX | PICK_CO), what
        elif c == CODE_NAN:
            assert ccr == NO_INDEX and np.isnan(w.real) and np.isnan(w.imag), what  # no search ran: not an early exit
        else:
            assert ccr == CODE_NAN_RE and np.isnan(w.real) and w.imag == 0.0, what  # handled as XSW_CODE_NAN_RE
        assert g_flat == c & 0x3FFFFFFF and g_sign == (c >> 30) & 1, what


@pytest.mark.parametrize("n_wcr", N_WCR)
def test_crosspol_decode_and_both_index_rules(driver, n_wcr):
    codes = cr_codes(n_wcr)
    got = driver([("cr", c, n_wcr) for c in codes])
    arr = np.array(codes, np.uint32)

    # cost_codes_ref.cost_cr on a table with cr_lut[icr] = icr, sigma0 = 0: the residual is finite where the code holds an index
    # by the cost pass's rule, and is that index
    p = types.SimpleNamespace(wspd_cr=np.arange(float(n_wcr)), inc_cr_dim=np.array([30.0]), cr_lut=np.arange(float(n_wcr))[:, None],
                              wspd_dim=np.zeros(0), phi_dim=np.zeros(0), dwspd_fg=2.0)
    res = cost_codes_ref.cost_cr(None, arr, np.full(len(codes), 30.0), 0.0, 0.1, p)["residual"]

    differ = []
    for c, g, r in zip(codes, got, res):
        nan_re, foreign, pick_co, index, strict, lenient = g
        what = f"code {c:#x} n_wcr {n_wcr}"
        assert nan_re == (c == CODE_NAN_RE), what
        assert foreign == (c >= 0x80000000 and c != CODE_NAN_RE), what
        assert pick_co == bool(c & PICK_CO) and index == c & NO_INDEX, what
        assert bool(lenient) == bool(np.isfinite(r)), what
        if lenient:
            assert index == r, what
        assert bool(strict) == bool(lenient and c < 0x80000000), what
        if strict != lenient:
            differ.append(c)
    assert differ == ([0x80000003] if n_wcr > 3 else []), differ
    by_code = dict(zip(codes, got))
    assert by_code[0x80000003][4] == 0 and by_code[0x80000003][1] == 1  # the strict rule never reads a foreign code


def test_encode_then_decode_is_the_identity(driver):
    n_w, n_phi = PLANES[0]
    plane = n_w * n_phi
    pairs = [(flat, sign) for flat in range(plane) for sign in (0, 1)]
    enc = [r[0] for r in driver([("co_enc", f, s) for f, s in pairs])]
    dec = driver([("co", e, plane) for e in enc])
    for (flat, sign), e, d in zip(pairs, enc, dec):
        assert d == [0, 0, 1, flat, sign, flat + sign * plane], (flat, sign, hex(e))
    for n_wcr in N_WCR:
        cases = [(index, pick) for index in list(range(n_wcr)) + [NO_INDEX] for pick in (0, 1)]
        enc = [r[0] for r in driver([("cr_enc", i, p) for i, p in cases])]
        dec = driver([("cr", e, n_wcr) for e in enc])
        for (index, pick), e, d in zip(cases, enc, dec):
            has = int(index != NO_INDEX)
            assert d == [0, 0, pick, index, has, has], (index, pick, hex(e))
