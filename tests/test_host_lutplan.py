"""CPU: the LUT side's pure arithmetic (csrc/xsw_lutplan.hpp: axis predicates, co-pol geometry and gates, the scalars and
capability flags of DevTables, the host-built tables, the cross-pol plan, detrend's row and the nesz block rule), compiled with
a host C++ compiler and compared with the expressions install_co / upload_cr / xsw_detrend / xsw_nesz_flatten carried inline
before.  The expected values are those expressions restated here in Python / numpy (line of csrc/xsw.hip at commit 3c1e37a
beside each), never the header's own output.  Doubles travel as C99 hex floats, so every comparison is bit for bit."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xsarsea_amd", "csrc")
INCLUDE = os.path.join(os.path.dirname(CSRC), "..", "include")
BLK_R, BLK_C, BLK_C4, CELL_R, CELL_C, INV_BINS, TAIL_LEVELS = 4, 16, 4, 8, 2, 2048, 7  # xsw_device.hpp:28-29, :86-87, :735-747

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include "xsw_lutplan.hpp"
struct Tab {  // the non-pointer members of DevTables an install sets
    int n_inc, n_w, n_phi, phi_pad, w_pad, phi_180, prunable, co_off32, band_mul24, nbc4, ncr, ncc, cell_span_ok, nbr, nbc, blk_g, nbands,
        blk_span_ok, inc_uniform;
    double w0, inv_wstep, phi0, phi_last, inv_dphi, wstep_half, inv_nphi, inc0, inv_incstep;
    int n_inc_cr, n_wcr, wcr_pad, cr_finite, cr_monotone, inc_cr_uniform;
    double wcr0, inv_wcrstep, wcrstep_half, inc_cr0, inv_inccrstep;
};
static bool rd_vec(std::vector<double> &v)  // "hex n v..." (C99 hex floats), "ramp n a0 step" (a0 + i * step: exact values only), "none"
{
    char kind[8];
    long long n;
    if (scanf("%7s", kind) != 1) return false;
    if (!strcmp(kind, "none")) { v.clear(); return true; }
    if (scanf("%lld", &n) != 1) return false;
    v.resize((size_t)n);
    if (!strcmp(kind, "ramp")) {
        double a0, step;
        if (scanf("%la %la", &a0, &step) != 2) return false;
        for (long long i = 0; i < n; ++i) v[(size_t)i] = a0 + (double)i * step;
        return true;
    }
    for (auto &x : v) if (scanf("%la", &x) != 1) return false;
    return true;
}
template <class V> static void pr(const V &v) { printf(" %zu", v.size()); for (auto x : v) printf(" %a", (double)x); }
int main()
{
    char cmd[16];
    long long a[4];
    std::vector<double> x, y, z, t[6];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "geom")) {  // nI nW nP
            if (scanf("%lld %lld %lld", &a[0], &a[1], &a[2]) != 3) return 2;
            const CoGeometry g{(int)a[0], (int)a[1], (int)a[2]};
            printf("%d %d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %lld %lld %lld %lld %lld %d %d %d %u %u %zu %u", g.ppad, g.wpad,
                   g.nbr, g.nbc, g.nbc4, g.ncr, g.ncc, g.blk_g, g.nbands, g.n_dense, g.n_body, g.n_slack, g.n_pad, g.tail_n, g.inv_n, g.inv_grid_n, g.coT_n,
                   g.rows, g.nblk, g.nband, g.ncell, g.nblk4, (int)g.inv_ok, (int)g.blk_ok, (int)g.blk4_ok, g.pad_grid, g.col_grid,
                   g.n_pad * 8 + XSW_OWNED_SLACK, blocks_of_256(g.nblk));
        } else if (!strcmp(cmd, "axis")) {  // one axis: strictly_ascending uniform_axis all_finite
            if (!rd_vec(x)) return 2;
            printf("%d %d %d", (int)strictly_ascending(x.data(), (int)x.size()), (int)uniform_axis(x.data(), (int)x.size()), (int)all_finite(x.data(), x.size()));
        } else if (!strcmp(cmd, "same")) {
            if (!rd_vec(x) || !rd_vec(y)) return 2;
            printf("%d", (int)same_axis(x.data(), (int)x.size(), y.data(), (int)y.size()));
        } else if (!strcmp(cmd, "left")) {  // x_old x_new
            if (!rd_vec(x) || !rd_vec(y)) return 2;
            std::vector<int> lo;
            const bool ok = left_neighbours(x.data(), (int)x.size(), y.data(), (int)y.size(), lo);
            printf("%d", (int)ok);
            if (ok) for (int v : lo) printf(" %d", v);
        } else if (!strcmp(cmd, "coscal")) {  // lut_finite trig_ok inc wspd phi
            if (scanf("%lld %lld", &a[0], &a[1]) != 2 || !rd_vec(x) || !rd_vec(y) || !rd_vec(z)) return 2;
            xsw_lut l{};
            l.inc = x.data(); l.wspd = y.data(); l.phi = z.data();
            l.n_inc = (int)x.size(); l.n_wspd = (int)y.size(); l.n_phi = (int)z.size();
            Tab T{};
            co_scalars(T, &l, CoGeometry{l.n_inc, l.n_wspd, l.n_phi}, a[0] != 0, a[1] != 0);
            printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %a %a %a %a %a %a %a %a %a", T.n_inc, T.n_w, T.n_phi, T.phi_pad, T.w_pad, T.phi_180,
                   T.prunable, T.co_off32, T.band_mul24, T.nbc4, T.ncr, T.ncc, T.cell_span_ok, T.nbr, T.nbc, T.blk_g, T.nbands, T.blk_span_ok, T.inc_uniform,
                   T.w0, T.inv_wstep, T.phi0, T.phi_last, T.inv_dphi, T.wstep_half, T.inv_nphi, T.inc0, T.inv_incstep);
        } else if (!strcmp(cmd, "cotab")) {  // wspd phi cos_phi sin_phi out_dir abs_co dual_dir ("none": the library's libm)
            if (!rd_vec(y) || !rd_vec(z)) return 2;
            for (auto &v : t) if (!rd_vec(v)) return 2;
            xsw_lut l{};
            l.wspd = y.data(); l.phi = z.data(); l.n_inc = 1; l.n_wspd = (int)y.size(); l.n_phi = (int)z.size();
            auto opt = [](const std::vector<double> &v) { return v.empty() ? nullptr : v.data(); };
            l.cos_phi = opt(t[0]); l.sin_phi = opt(t[1]); l.out_dir = opt(t[2]); l.abs_co = opt(t[3]); l.dual_dir = opt(t[4]);
            const CoHostTables H(&l);
            printf("%d", (int)H.trig_ok);
            pr(H.wh); pr(H.wh32); pr(H.cphi); pr(H.sphi); pr(H.csphi); pr(H.csphi32); pr(H.out_dir); pr(H.abs_co); pr(H.dual_dir); pr(H.sol); pr(H.sol32);
        } else if (!strcmp(cmd, "cr")) {  // inc wspd db[n_inc][n_wspd]
            if (!rd_vec(x) || !rd_vec(y) || !rd_vec(z)) return 2;
            xsw_lut l{};
            l.inc = x.data(); l.wspd = y.data(); l.db = z.data(); l.n_inc = (int)x.size(); l.n_wspd = (int)y.size();
            const CrPlan p(&l);
            Tab T{};
            cr_scalars(T, &l, p);
            printf("%d %d %d %d %d %d %a %a %a %a %a", T.n_inc_cr, T.n_wcr, T.wcr_pad, T.cr_finite, T.cr_monotone, T.inc_cr_uniform, T.wcr0, T.inv_wcrstep,
                   T.wcrstep_half, T.inc_cr0, T.inv_inccrstep);
            pr(p.pad); pr(p.wh); pr(p.inv); pr(p.grid);
        } else if (!strcmp(cmd, "detrend")) {
            if (!rd_vec(x)) return 2;
            std::vector<double> both;
            printf("%d", (int)detrend_row(x.data(), x.size(), both));
            pr(both);
        } else if (!strcmp(cmd, "nesz")) {  // lines samples partial_bytes
            if (scanf("%lld %lld %lld", &a[0], &a[1], &a[2]) != 3) return 2;
            const NeszBlocks b = nesz_blocks(a[0], a[1], (size_t)a[2]);
            printf("%lld %lld %zu", b.nb, b.lpb, b.scratch_bytes);
        } else return 2;
        printf("\n");
    }
    return 0;
}
"""


def hexv(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    return "hex %d %s" % (v.size, " ".join(float(x).hex() for x in v)) if v.size else "hex 0"


def ramp(n, a0=0.0, step=1.0):
    """An axis the driver makes itself (a0 + i * step, exact for these values): the long axes of the gate shapes."""
    return "ramp %d %s %s" % (n, float(a0).hex(), float(step).hex()), a0 + np.arange(n, dtype=np.float64) * step


def num(tok):
    return float.fromhex(tok) if ("x" in tok or "nan" in tok or "inf" in tok) else int(tok)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = next((c for c in ("g++", "clang++", "c++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, clang++, c++) on PATH")
    td = tmp_path_factory.mktemp("host_lutplan")
    src, exe = td / "driver.cpp", td / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-I" + INCLUDE, str(src), "-o", str(exe)])

    def ask_(*queries):
        """queries: strings (one command each); returns the tokens of each answer, numbers parsed (hex floats exactly)."""
        out = subprocess.run([str(exe)], input="\n".join(queries) + "\n", text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[num(t) for t in ln.split()] for ln in out]

    return ask_


def vectors(tokens):
    """The answer's trailing ' n v...' groups."""
    out, k = [], 0
    while k < len(tokens):
        n = tokens[k]
        out.append(np.array(tokens[k + 1:k + 1 + n], dtype=np.float64))
        k += 1 + n
    return out


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ceil_div(a, b):
    return -(-a // b)


# ---- the parent's expressions
def p_uniform(a):  # xsw.hip:301-310
    n = len(a)
    if n < 2:
        return False
    step = (a[n - 1] - a[0]) / (n - 1)
    if not (step > 0) or not math.isfinite(step):
        return False
    tol = 1e-12 * max(max(abs(a[0]), abs(a[n - 1])), step)
    return bool(np.all(np.abs(a - (a[0] + np.arange(n) * step)) <= tol))


def p_geometry(nI, nW, nP):
    ppad, wpad = (nP + 3) & ~3, (nW + 3) & ~3  # :349
    nbr, nbc, nbc4 = ceil_div(nW, BLK_R), ceil_div(nP, BLK_C), ceil_div(nP, BLK_C4)  # :421
    ncr, ncc = ceil_div(nbr, CELL_R), ceil_div(nbc, CELL_C)  # :422
    blk_g = max(1, 64 // nbc)  # :423
    nbands = ceil_div(nbr, blk_g)  # :424
    n_dense = nI * nW * nP  # :351
    n_body, n_slack = nI * nW * ppad, 260 * ppad  # :352, :369-370
    inv_n = nI * INV_BINS * ppad  # :402
    rows = nI * nW  # :372
    nblk, nband, ncell, nblk4 = nI * nbr * nbc, nI * nbands, nI * ncr * ncc, nI * nbr * nbc4  # :428, :440, :456
    return [ppad, wpad, nbr, nbc, nbc4, ncr, ncc, blk_g, nbands, n_dense, n_body, n_slack, n_body + n_slack,
            nI * (TAIL_LEVELS + 1) * ppad,  # :394
            inv_n, 3 * nI,  # :407
            nI * nP * wpad + 512,  # :568
            rows, nblk, nband, ncell, nblk4,
            int(nW < 65536 and nI < 65536 and inv_n * 2 < (1 << 32)),  # :403
            int(nblk < (1 << 31)), int(nblk4 < (1 << 31)),  # :426, :454
            min((rows + 3) // 4, 256 * 32), (nI * nP + 255) // 256,  # :373, :386 / :411
            (n_body + n_slack) * 8 + 64,  # :365
            ((nblk + 255) // 256) & 0xffffffff]  # :433


def p_co_scalars(inc, w, phi, lut_finite, trig_ok):  # xsw.hip:546-565
    nI, nW, nP = len(inc), len(w), len(phi)
    g = p_geometry(nI, nW, nP)
    ppad, wpad, nbr, nbc, nbc4, ncr, ncc, blk_g, nbands = g[:9]
    span = phi[nP - 1] - phi[0]
    with np.errstate(divide="ignore"):
        inv_wstep = (nW - 1) / (w[nW - 1] - w[0]) if nW > 1 else 0.0  # :551
        wstep_half = np.float64(0.5) / np.float64(inv_wstep)  # :553
    prunable = (nW >= 2 and nP >= 2 and nW < 32768 and nP < 65536 and nW * ppad < (1 << 30) and p_uniform(w) and p_uniform(phi) and trig_ok
                and span <= 360.0 + 1e-9 and lut_finite)  # :558-559
    band_mul24 = (nI * nW <= 0xFFFFFF and (nI + 1) * INV_BINS <= 0xFFFFFF and ppad * 8 <= 0xFFFFFF and (nI + 1) * nP <= 0xFFFFFF
                  and wpad * 8 <= 0xFFFFFF and nI * nP * wpad * 8 < (1 << 32))  # :562-563
    return [nI, nW, nP, ppad, wpad, int((180.0 - span) < 2.0),  # :546-547
            int(prunable), int((nI * nW + 260) * ppad * 8 < (1 << 32)),  # :561
            int(band_mul24), nbc4, ncr, ncc,
            int(nP > 1 and (CELL_C * BLK_C - 1) * span / (nP - 1) < 170.0),  # :565
            nbr, nbc, blk_g, nbands,
            int(nP > 1 and (BLK_C - 1) * span / (nP - 1) < 170.0),  # :564
            int(p_uniform(inc) and nI >= 2),  # :555
            w[0], inv_wstep, phi[0], phi[nP - 1],  # :548-551
            (nP - 1) / span if nP > 1 else 0.0, float(wstep_half), 1.0 / nP,  # :552-554
            inc[0], (nI - 1) / (inc[nI - 1] - inc[0]) if nI > 1 else 0.0]  # :556-557


def check_scalars(ask, cases):
    """cases: (inc, wspd, phi, lut_finite, trig_ok), an axis either an array or a ramp() pair."""
    def spec(ax):
        return ax if isinstance(ax, tuple) else (hexv(ax), np.asarray(ax, dtype=np.float64))
    cases = [tuple(spec(ax) for ax in c[:3]) + tuple(c[3:]) for c in cases]
    got = ask(*["coscal %d %d %s %s %s" % (lf, tr, i[0], w[0], p[0]) for i, w, p, lf, tr in cases])
    for (i, w, p, lf, tr), g in zip(cases, got):
        want = p_co_scalars(i[1], w[1], p[1], lf, tr)
        print(len(i[1]), len(w[1]), len(p[1]), "->", g[:19])
        assert g[:19] == want[:19], (len(i[1]), len(w[1]), len(p[1]))
        assert same_bits(g[19:], want[19:]), (len(i[1]), len(w[1]), len(p[1]), g[19:], want[19:])
    return got


def model_axes():
    """(inc, wspd, phi) of the default CMOD5.N LUT, of its resolution="low" LUT and of a 0..360 phi axis, read from the model."""
    from xsarsea_amd.windspeed import models
    m = models.get_model("gmf_cmod5n")
    high, low = ([np.asarray(ax, dtype=np.float64) for ax in m._target_axes(res, {})] for res in ("high", "low"))
    return [high, low, [high[0], high[1], np.linspace(0.0, 360.0, 2 * (len(high[2]) - 1) + 1)]]


def test_geometry_and_gates(ask):
    shapes = [tuple(len(ax) for ax in axes) for axes in model_axes()]
    shapes += [(1, 1, 1), (2, 2, 2), (1, 2, 1), (3, 5, 7), (60, 1000, 361)]
    shapes += [(65535, 4, 4), (65536, 4, 4), (4, 65535, 4), (4, 65536, 4)]  # unsigned short rows / slices of the inverse
    shapes += [(1023, 8, 1024), (1024, 8, 1024), (1025, 8, 1024), (1024, 8, 1020), (1024, 8, 1025)]  # inv_n * 2 < 2^32
    shapes += [(2047, 4096, 16384), (2048, 4096, 16384), (2048, 4093, 16384), (2048, 4097, 16384), (2048, 4096, 16368)]  # blocks < 2^31
    shapes += [(2047, 4096, 4096), (2048, 4096, 4096), (2048, 4096, 4092), (2048, 4096, 4097)]  # sub-blocks < 2^31
    for shape, got in zip(shapes, ask(*["geom %d %d %d" % s for s in shapes])):
        print(shape, "->", got)
        assert got == p_geometry(*shape), shape
    gates = {s: p_geometry(*s)[22:25] for s in shapes}
    assert gates[(65535, 4, 4)][0] == 1 and gates[(65536, 4, 4)][0] == 0 and gates[(4, 65536, 4)][0] == 0
    assert gates[(1023, 8, 1024)][0] == 1 and gates[(1024, 8, 1024)][0] == 0 and gates[(1024, 8, 1020)][0] == 1
    assert gates[(2047, 4096, 16384)][1] == 1 and gates[(2048, 4096, 16384)][1] == 0 and gates[(2048, 4096, 16368)][1] == 1
    assert gates[(2047, 4096, 4096)][2] == 1 and gates[(2048, 4096, 4096)][2] == 0 and gates[(2048, 4096, 4092)][2] == 1


def test_axis_predicates(ask):
    lin = np.linspace(0.2, 50.0, 250)
    step = lin[1] - lin[0]
    bumped = lin.copy()
    bumped[100] += 1e-7 * step
    axes = [lin, np.linspace(17.0, 50.0, 166), np.linspace(0.0, 180.0, 181), np.linspace(-180.0, 180.0, 721),  # np.linspace: uniform
            np.array([1.0, 2.0, 4.0, 8.0]), lin.astype(np.float32).astype(np.float64), bumped,  # none of these is
            np.array([3.0]), np.array([1.0, 2.0]), np.array([2.0, 1.0]), np.array([1.0, 1.0]), np.array([0.0, np.inf]), np.array([0.0, np.nan, 2.0])]
    want = [[1, 1, 1]] * 4 + [[1, 0, 1]] * 3 + [[1, 0, 1], [1, 1, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 0]]
    got = ask(*["axis " + hexv(a) for a in axes])
    for a, g, w in zip(axes, got, want):
        assert g == w, a
        assert g[0] == int(np.all(np.diff(a) > 0)) and g[1] == int(p_uniform(a)) and g[2] == int(np.all(np.isfinite(a)))  # xsw.hip:291-316
    same = ask("same %s %s" % (hexv(lin), hexv(lin.copy())), "same %s %s" % (hexv(lin), hexv(bumped)), "same %s %s" % (hexv(lin), hexv(lin[:-1])))
    assert same == [[1], [0], [0]]  # xsw.hip:1166-1172


def test_left_neighbours_is_searchsorted_clipped(ask):
    rng = np.random.default_rng(5)
    x_old = np.sort(rng.uniform(0.0, 10.0, 37))
    x_new = np.concatenate([[x_old[0], x_old[-1], x_old[5], x_old[5], x_old[6]], rng.uniform(x_old[0], x_old[-1], 50)])
    (got,) = ask("left %s %s" % (hexv(x_old), hexv(x_new)))
    want = np.clip(np.searchsorted(x_old, x_new, side="left"), 1, len(x_old) - 1) - 1  # scipy interp1d; xsw.hip:1068-1076
    assert got[0] == 1 and got[1:] == want.tolist()
    two = ask("left %s %s" % (hexv([1.0, 2.0]), hexv([1.0, 1.5, 2.0])))
    assert two == [[1, 0, 0, 0]]
    for bad in (x_old[0] - 1e-9, x_old[-1] + 1e-9, np.nan):  # bounds_error=True: refused (xsw.hip:1072)
        assert ask("left %s %s" % (hexv(x_old), hexv([x_old[3], bad]))) == [[0]]


def test_scalars_and_flags_of_the_model_luts_and_small_axes(ask):
    cases = [(inc, w, phi, 1, 1) for inc, w, phi in model_axes()]
    inc, w, phi = cases[0][:3]
    cases += [(inc, w, phi, 0, 1), (inc, w, phi, 1, 0)]  # a NaN in the table, a caller's cos / sin off this libm's
    cases += [([30.0], [5.0], [0.0], 1, 1), ([30.0, 31.0], [5.0, 6.0], [0.0, 1.0], 1, 1), ([30.0], [5.0, 6.0], [10.0], 1, 1)]  # lengths 1 and 2
    w32 = w.astype(np.float32).astype(np.float64)
    bumped = w.copy()
    bumped[7] += 1e-7 * (w[1] - w[0])
    cases += [(inc, np.cumsum(np.linspace(0.1, 1.0, 40)), phi, 1, 1), (inc, w32, phi, 1, 1), (inc, bumped, phi, 1, 1),  # not uniform: not prunable
              (np.array([20.0, 21.0, 23.0]), w, phi, 1, 1), (inc, w, np.linspace(0.0, 361.0, 362), 1, 1)]
    got = check_scalars(ask, cases)
    assert [g[6] for g in got] == [1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]  # prunable
    assert [g[5] for g in got[:3]] == [1, 1, 1] and got[11][18] == 0  # phi_180: a span of 178 degrees or more; inc_uniform


def test_scalars_and_flags_at_the_gates(ask):
    one, two = np.array([30.0]), np.array([30.0, 31.0])
    P = lambda n, span: ramp(n, 0.0, span / (n - 1))  # exact: spans and counts below are chosen so
    cases = []
    for nW in (32767, 32768, 32769):  # prunable: n_wspd < 32768
        cases.append((two, ramp(nW), ramp(4, 0.0, 64.0), 1, 1))
    for nP in (65535, 65536, 65537):  # prunable: n_phi < 65536 (step 2^-8 degree: span <= 360)
        cases.append((two, ramp(8), ramp(nP, 0.0, 2.0 ** -8), 1, 1))
    cases += [(two, ramp(16385), ramp(65532, 0.0, 2.0 ** -8), 1, 1), (two, ramp(16385), ramp(65535, 0.0, 2.0 ** -8), 1, 1)]  # n_wspd * phi_pad < 2^30
    # band_mul24: each 24-bit product (and the 4 GB of the transposed slices) at the last shape that passes and the first that does not
    cases += [(ramp(94), ramp(178481), ramp(4), 1, 1), (ramp(4095), ramp(4097), ramp(4), 1, 1), (ramp(4096), ramp(4096), ramp(4), 1, 1)]  # n_inc * n_wspd
    cases += [(ramp(n), ramp(8), ramp(4), 1, 1) for n in (8189, 8190, 8191)]  # (n_inc + 1) * XSW_INV_BINS
    cases += [(two, ramp(8), ramp(n), 1, 1) for n in (2097148, 2097151, 2097152, 2097153)]  # phi_pad * 8
    cases += [(ramp(4094), ramp(8), ramp(4097), 1, 1), (ramp(4095), ramp(8), ramp(4096), 1, 1), (ramp(4095), ramp(8), ramp(4097), 1, 1)]  # (n_inc + 1) * n_phi
    cases += [(two, ramp(n), ramp(4), 1, 1) for n in (2097148, 2097151, 2097152, 2097153)]  # w_pad * 8
    cases += [(ramp(511), ramp(1024), ramp(1024), 1, 1), (ramp(512), ramp(1024), ramp(1024), 1, 1), (ramp(512), ramp(1020), ramp(1024), 1, 1),
              (ramp(512), ramp(1025), ramp(1024), 1, 1)]  # n_inc * n_phi * w_pad * 8 < 2^32
    # co_off32: (n_inc * n_wspd + 260) * phi_pad * 8 against 4 GB: one row below, at, one row above (phi_pad = 2^16: 2^13 - 260 rows)
    cases += [(one, ramp(n), ramp(65536, 0.0, 2.0 ** -8), 1, 1) for n in ((1 << 13) - 261, (1 << 13) - 260, (1 << 13) - 259)]
    # the 170 degree span rules (15 / 31 direction steps) and phi_180 (a span of more than 178 degrees)
    cases += [(two, ramp(8), P(16, s), 1, 1) for s in (169.0, 170.0, 171.0)] + [(two, ramp(8), P(32, s), 1, 1) for s in (169.0, 170.0, 171.0)]
    cases += [(two, ramp(8), ramp(2, 0.0, s), 1, 1) for s in (177.0, 178.0, 178.5, 180.0, 182.5)]
    got = check_scalars(ask, cases)
    flag = lambda k: [g[k] for g in got]
    assert flag(6)[:8] == [1, 0, 0, 1, 0, 0, 1, 0]  # prunable
    assert flag(8)[8:29] == [1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0]  # band_mul24 (the pads round up to a multiple of 4)
    assert flag(7)[29:32] == [1, 0, 0]  # co_off32
    assert flag(17)[32:35] == [1, 0, 0] and flag(12)[35:38] == [1, 0, 0]  # blk_span_ok, cell_span_ok
    assert flag(5)[38:] == [0, 0, 1, 1, 1]  # phi_180: 180 - span < 2


def test_flags_of_the_route_geometries(ask):
    """The seven LUT shapes of tests/route_geometry.py are there for the flags below (tests/test_gpu_route_geometry.py forces every
    inversion route on each of them): a later change of the pads or of the block sizes must fail here instead of quietly leaving
    the GPU test with seven controls.  All of them run the chain (prunable, band_mul24, co_off32)."""
    import route_geometry as rg
    #                 phi_pad % 8, phi_180, blk_span_ok, cell_span_ok, block columns
    want = {"pad4_half": (4, 1, 1, 1, 5),      # misaligned odd rows of inv_rows
            "pad4_full": (4, 1, 1, 1, 10),     # ... on a full circle: phi_180 all the same (180 - span < 2, the reference's rule)
            "open_half": (4, 0, 1, 1, 5),      # 0..175 degrees: phi_180 == 0 needs a span below 178
            "narrow": (4, 1, 0, 0, 1),         # 12 directions 16.4 degrees apart: one block column, and 15 steps span 245 degrees
            "coarse_full": (4, 1, 0, 0, 2),    # 15 degree steps: no k_invert_blocks
            "tail": (4, 1, 1, 1, 5),
            "default_like": (0, 1, 1, 1, 12)}  # the control
    assert list(want) == list(rg.GEOMETRIES)
    axes = {}
    for name in want:
        lco, _ = rg.build_luts(name)
        axes[name] = (lco.incidence, lco.wspd, lco.phi)
    got = check_scalars(ask, [axes[name] + (1, 1) for name in want])
    for (name, w), g in zip(want.items(), got):
        geo = rg.GEOMETRIES[name]
        assert g[:3] == [geo["n_inc"], geo["n_w"], geo["n_phi"]], name
        assert (g[3] % 8, g[5], g[17], g[12], g[14]) == w, (name, g[:19])
        assert g[6] == 1 and g[8] == 1 and g[7] == 1, (name, "prunable, band_mul24, co_off32", g[:19])
    assert got[1][4] != got[1][1]  # pad4_full: w_pad != n_w
    assert rg.GEOMETRIES["pad4_full"]["n_wcr"] % 4 != 0


def p_host_tables(w, phi, cos_phi=None, sin_phi=None, out_dir=None, abs_co=None, dual_dir=None):
    """xsw.hip:478-542 restated; math.cos / sin / atan2 are the C library's, as the defaults are; hypot is taken from libm itself
    (CPython's math.hypot has been its own algorithm since 3.8 and differs from libm's in the last bit)."""
    import ctypes
    import ctypes.util
    c_hypot = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").hypot
    c_hypot.restype, c_hypot.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]
    nW, nP = len(w), len(phi)
    wh = 0.5 * w  # :479
    rad = [p * (math.pi / 180.0) for p in phi]  # :482
    cp = np.array([math.cos(r) for r in rad]) if cos_phi is None else cos_phi  # :483
    sp = np.array([math.sin(r) for r in rad]) if sin_phi is None else sin_phi  # :484
    trig_ok = all(abs(c - math.cos(r)) <= 1e-12 and abs(s - math.sin(r)) <= 1e-12 for c, s, r in zip(cp, sp, rad))  # :485
    cs = np.stack([cp, sp], axis=1)  # :500
    if out_dir is None:  # :510-512
        od = np.array([[[math.cos(sg * p * (math.pi / 180.0)), math.sin(sg * p * (math.pi / 180.0))] for p in phi] for sg in (1.0, -1.0)])
    else:
        od = np.asarray(out_dir).reshape(2, nP, 2)
    re = w[None, :, None] * od[:, None, :, 0]  # :519 / :537
    im = w[None, :, None] * od[:, None, :, 1] + 0.0 * od[:, None, :, 0]  # :519 / :538
    if dual_dir is None:  # :522
        ph = np.array([math.atan2(i, r) for i, r in zip(im.ravel(), re.ravel())])
        dd = np.stack([[math.cos(v) for v in ph], [math.sin(v) for v in ph]], axis=1)
    else:
        dd = dual_dir
    ab = np.array([c_hypot(r, i) for r, i in zip(re[0].ravel(), im[0].ravel())]) if abs_co is None else abs_co  # :523
    sol = np.stack([re, im], axis=3)
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)  # :492, :502, :542
    return int(trig_ok), [wh, f32(wh), cp, sp, cs, f32(cs), od, ab, dd, sol, f32(sol)]


def cotab(ask, w, phi, *opt):
    (got,) = ask("cotab %s %s %s" % (hexv(w), hexv(phi), " ".join("none" if o is None else hexv(o) for o in opt)))
    return got[0], vectors(got[1:])


NAMES = ["wh", "wh32", "cphi", "sphi", "csphi", "csphi32", "out_dir", "abs_co", "dual_dir", "sol", "sol32"]


def test_host_tables_pass_the_callers_values_through(ask):
    """The route the Python layer uses: numpy's values for every optional table."""
    _, (_, w, phi) = model_axes()[0], model_axes()[1]
    w, phi = w[::3], phi[::2]
    cos_phi, sin_phi = np.cos(np.radians(phi)), np.sin(np.radians(phi))
    od = np.stack([np.exp(1j * np.deg2rad(phi)), np.exp(1j * np.deg2rad(-phi))])
    out_dir = np.stack([od.real, od.imag], axis=2)
    sol = w[None, :, None] * od[:, None, :]
    abs_co = np.abs(sol[0])
    dual = np.exp(1j * np.angle(sol))
    dual_dir = np.stack([dual.real, dual.imag], axis=3)
    trig_ok, got = cotab(ask, w, phi, cos_phi, sin_phi, out_dir, abs_co, dual_dir, None)
    want_ok, want = p_host_tables(w, phi, cos_phi, sin_phi, out_dir.ravel(), abs_co.ravel(), dual_dir.ravel())
    assert trig_ok == want_ok == 1
    for name, g, v in zip(NAMES, got, want):
        assert same_bits(g, v), name
    for k, passed in ((2, cos_phi), (3, sin_phi), (6, out_dir), (7, abs_co), (8, dual_dir)):
        assert same_bits(got[k], passed), NAMES[k]
    off = cos_phi.copy()
    off[3] += 2e-12
    assert cotab(ask, w, phi, off, sin_phi, out_dir, abs_co, dual_dir, None)[0] == 0  # trig_ok: 1e-12 (xsw.hip:485)


def test_host_tables_default_to_the_c_librarys(ask):
    w, phi = np.linspace(0.2, 50.0, 9), np.linspace(0.0, 180.0, 37)
    trig_ok, got = cotab(ask, w, phi, None, None, None, None, None, None)
    want_ok, want = p_host_tables(w, phi)
    assert trig_ok == want_ok == 1
    for name, g, v in zip(NAMES, got, want):
        assert same_bits(g, v), name


def p_cr(inc, w, db):  # xsw.hip:590-627
    nI, nW = db.shape
    wpad = (nW + 3) & ~3
    pad = np.zeros((nI, wpad))
    pad[:, :nW] = db  # :592
    finite = bool(np.all(np.isfinite(db)))  # :601
    mono = finite and nW >= 2 and p_uniform(w) and bool(np.all(db[:, 1:] >= db[:, :-1]))  # :602-605
    inv, grid = np.zeros(0), np.zeros(0)
    if mono and nW < 65536:  # :611
        inv, grid = np.zeros((nI, INV_BINS)), np.zeros((nI, 3))
        for r in range(nI):
            t0, width = db[r, 0], (db[r, -1] - db[r, 0]) / float(INV_BINS)  # :616
            if width > 0.0 and width < 1e300:  # :617
                grid[r] = [t0, width, 1.0 / width]  # :618
                thr = [t0 + b * width for b in range(INV_BINS)]  # fma(b, width, t0) :620 -- see below
                inv[r] = np.searchsorted(db[r], thr, side="left")
                inv[r, 0] = 0
    with np.errstate(divide="ignore"):
        inv_wstep = np.float64(nW - 1) / np.float64(w[-1] - w[0]) if nW > 1 else np.float64(0.0)  # :608
        half = np.float64(0.5) / inv_wstep  # :609
    return ([nI, nW, wpad, int(finite), int(mono), int(p_uniform(inc) and nI >= 2)],  # :599-606, :625
            [w[0], float(inv_wstep), float(half), inc[0], (nI - 1) / (inc[-1] - inc[0]) if nI > 1 else 0.0],  # :607-609, :626-627
            [pad, 0.5 * w, inv, grid])


def ask_cr(ask, inc, w, db):
    (got,) = ask("cr %s %s %s" % (hexv(inc), hexv(w), hexv(db)))
    return got[:6], got[6:11], vectors(got[11:])


def test_cross_pol_plan(ask):
    """Rows on a dyadic grid (multiples of 2^-10 dB, width a multiple of 2^-21): fma(b, width, t0) is then exact, so numpy's
    t0 + b * width is the same threshold and np.searchsorted the same first index."""
    rng = np.random.default_rng(11)
    inc, w = np.linspace(17.0, 50.0, 5), np.linspace(0.2, 50.0, 250)
    db = np.cumsum(rng.integers(0, 200, (5, 250)), axis=1) / 1024.0 - 40.0
    db[2] = -12.5  # a constant row: width 0, all zeros
    db[3, 100:140] = db[3, 100]  # a plateau: the FIRST index at or above a threshold
    for case, (i_, w_, d_) in {"monotone": (inc, w, db), "short": (inc[:1], w[:2], db[:1, :2])}.items():
        flags, scal, vecs = ask_cr(ask, i_, w_, d_)
        w_flags, w_scal, w_vecs = p_cr(i_, w_, d_)
        assert flags == w_flags and flags[3:5] == [1, 1], case
        assert same_bits(scal, w_scal), case
        for g, v in zip(vecs, w_vecs):
            assert same_bits(g, v), case
    assert not np.any(ask_cr(ask, inc, w, db)[2][2].reshape(5, INV_BINS)[2]) and not np.any(ask_cr(ask, inc, w, db)[2][3].reshape(5, 3)[2])
    down = db.copy()
    down[1, 60] = down[1, 59] - 1.0 / 1024.0
    nan = db.copy()
    nan[4, 17] = np.nan
    w32 = w.astype(np.float32).astype(np.float64)
    for case, (w_, d_, finite) in {"not monotone": (w, down, 1), "nan": (w, nan, 0), "speed axis not uniform": (w32, db, 1)}.items():
        flags, scal, vecs = ask_cr(ask, inc, w_, d_)
        w_flags, w_scal, w_vecs = p_cr(inc, w_, d_)
        assert flags == w_flags and flags[3:5] == [finite, 0], case
        assert vecs[2].size == 0 and vecs[3].size == 0, case  # no inverse
        assert same_bits(scal, w_scal) and same_bits(vecs[0], w_vecs[0]) and same_bits(vecs[1], w_vecs[1]), case


def test_detrend_row_and_its_fast_predicate(ask):
    ones = np.frombuffer(np.uint64(0x3FEFFFFFFFFFFFFF).tobytes(), dtype=np.float64)[0]  # mantissa all ones
    ordinary = [1.0, 0.731, -3.5, 2.0 ** 499, 2.0 ** -499, 1e-150]
    odd = [0.0, np.inf, -np.inf, np.nan, 5e-324, 2.0 ** 500, 2.0 ** -500, 2.0 ** 600, ones, -ones]
    rows = [ordinary] + [[1.0, v, 2.0] for v in odd] + [[v] for v in ordinary]
    got = ask(*["detrend " + hexv(r) for r in rows])
    for r, g in zip(rows, got):
        r = np.asarray(r, dtype=np.float64)
        with np.errstate(divide="ignore", over="ignore"):
            both = np.concatenate([r, 1.0 / r])  # xsw.hip:1321-1322
        a = np.abs(r)
        fast = np.all((a > 2.0 ** -500) & (a < 2.0 ** 500) & ((r.view(np.uint64) & np.uint64(0xFFFFFFFFFFFFF)) != np.uint64(0xFFFFFFFFFFFFF)))  # :1326
        assert g[0] == int(fast), r
        assert same_bits(vectors(g[1:])[0], both), r
    assert [g[0] for g in got] == [1] + [0] * len(odd) + [1] * len(ordinary)


def test_nesz_block_rule(ask):
    shapes = [(l, s) for l in (1, 7, 8, 20000) for s in (1, 256, 20000)]
    for partial in (16, 24):
        for (lines, samples), got in zip(shapes, ask(*["nesz %d %d %d" % (l, s, partial) for l, s in shapes])):
            gx = (samples + 255) // 256  # xsw.hip:1428
            nb = (256 * 16 + gx - 1) // gx  # :1429
            nb = max(1, min(min(nb, (lines + 7) // 8), 65535))  # :1430
            lpb = ceil_div(lines, nb)  # :1431
            nb = ceil_div(lines, lpb)  # :1432
            assert got == [nb, lpb, nb * samples * partial + (2 * samples + 8 + 2 * lines) * 8], (lines, samples)  # :1434
            assert nb * lpb >= lines and (nb - 1) * lpb < lines
