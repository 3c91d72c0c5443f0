"""CPU: the host side's pure arithmetic (csrc/xsw_plan.hpp: work-list layout, chunk plan, chunk staging, strip grid), compiled
with a host C++ compiler and compared with the expressions the four host paths carried before they shared it.  The expected
values are those expressions restated here (file:line of csrc/xsw.hip / xsw_invert_tu.hip at commit b383975 beside each), never
the header's own output.  The one allowed difference: the context's buffer now pads its lists to 256 B as the workers' buffers
always did, so its masks, records and total move up by at most 255 B."""
import itertools
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xsarsea_amd", "csrc")
B_SHARE, C_SHARE, REC_BYTES, NESZ_EV = 4, 4, 48, 2  # xsw_host.hpp:91-98, xsw_nesz.hpp:280
TOTAL = 1 + B_SHARE + C_SHARE

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "xsw_plan.hpp"
int main()
{
    char cmd[16];
    long long a[9];
    auto rd = [&](int n) { for (int i = 0; i < n; ++i) if (scanf("%lld", &a[i]) != 1) return false; return true; };
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "plan") && rd(5)) {  // lines samples cap_px tile_rows recut_flat
            const ChunkPlan p(a[0], a[1], a[2], a[3], a[4] != 0);
            printf("%lld %lld %lld %lld %lld %lld %zu", p.lines, p.samples, p.lines_per_chunk, p.nmain, p.tail_px, p.nchunks, p.max_px);
            for (long long k = 0; k < p.nchunks; ++k) {
                const ChunkPlan::Chunk c = p.chunk(k);
                printf(" %zu %zu %lld %lld", c.px0, c.npx, c.lines, c.samples);
            }
        } else if (!strcmp(cmd, "caps") && rd(4)) {  // n test_cap max_px lines_per_chunk
            printf("%zu %zu %zu", context_list_cap(a[0], a[1]), worker_list_cap((size_t)a[2]), strips_for(a[2], a[3]));
        } else if (!strcmp(cmd, "lists") && rd(2)) {  // list_cap mask_strips: byte offsets from the base, capacities, total
            WorkLists w;
            w.base = (unsigned *)(uintptr_t)(1u << 20);
            w.list_cap = (size_t)a[0];
            w.mask_strips = (size_t)a[1];
            auto off = [&](const void *p) { return (size_t)((const char *)p - (const char *)w.base); };
            for (WorkLists::List l : {WorkLists::G, WorkLists::B, WorkLists::C}) printf("%zu %zu %u ", off(w.count(l)), off(w.entries(l)), w.cap(l));
            printf("%zu %zu %zu", off(w.masks()), off(w.records()), w.bytes());
        } else if (!strcmp(cmd, "stage") && rd(9)) {  // max_px es inc co cr dsig anc code_co code_cr
            const ChunkStaging s((size_t)a[0], (size_t)a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu", s.o_inc, s.o_co, s.o_cr, s.o_dsig, s.o_anc, s.o_cc, s.o_ccr, s.o_end);
        } else if (!strcmp(cmd, "grid") && rd(3)) {  // rows cols wg_per_cu
            const Strips g = a[2] ? strip_grid(a[0], a[1], a[2]) : strip_grid(a[0], a[1]);
            printf("%lld %lld %lld", g.gx, g.gy, g.rows_per_block);
        } else return 2;
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = next((c for c in ("g++", "clang++", "c++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, clang++, c++) on PATH")
    td = tmp_path_factory.mktemp("host_plan")
    src, exe = td / "driver.cpp", td / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])

    def ask_(*queries):
        """queries: tuples (command, int, ...); returns one list of ints per query."""
        text = "".join(q[0] + " " + " ".join(str(int(v)) for v in q[1:]) + "\n" for q in queries)
        out = subprocess.run([str(exe)], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [[int(v) for v in ln.split()] for ln in out]

    return ask_


def ceil_div(a, b):
    return -(-a // b)


def pad(b):
    return (b + 255) & ~255


def strips_for(n, lines):  # xsw.hip:689
    return n // 64 + max(lines, n // 4096) + 64


# ---- the parent's chunk plans: each returns (nchunks, max_px, lines_per_chunk, [(px0, npx, lines, samples), ...])
def target_px(n, cap):  # xsw.hip:1002 / :1068 / :1441
    return min(cap, max(1 << 16, n // 16))


def parent_device(lines, samples):  # xsw.hip:967-990: at most two launches, main + tail
    n = lines * samples
    if lines < 16 and n >= (1 << 16):  # :967
        S = 4096
        Lv = n // S
        tail = n - Lv * S  # :972
        chunks = [(0, Lv * S, Lv, S)]  # :975
        if tail:
            chunks.append((Lv * S, tail, 1, tail))  # :978-980
        return len(chunks), max(Lv * S, tail), Lv, chunks
    return 1, n, lines, [(0, n, lines, samples)]  # :989


def parent_sigma0_host(lines, samples):  # xsw.hip:1001-1005 and :1015-1016
    n = lines * samples
    lpc = (max(ceil_div(target_px(n, 4 << 20), samples), 4) + 3) & ~3  # :1003
    nchunks = ceil_div(lines, lpc)  # :1004
    max_px = min(lpc, lines) * samples  # :1005
    chunks = []
    for k in range(nchunks):
        l0 = k * lpc
        l1 = min(lines, l0 + lpc)  # :1015
        chunks.append((l0 * samples, (l1 - l0) * samples, l1 - l0, samples))  # :1016, :1032
    return nchunks, max_px, lpc, chunks


def parent_host(lines, samples):  # xsw.hip:1065-1072 and :1093-1095, :1116-1118
    n = lines * samples
    tail_px = 0
    if lines < 16 and n >= (1 << 16):  # :1066
        samples = 4096
        lines = n // samples
        tail_px = n - lines * samples
    lpc = ceil_div(target_px(n, 2 << 20), samples) if samples > 0 else lines  # :1069
    lpc = (max(lpc, 4) + 3) & ~3  # :1070
    nmain = ceil_div(lines, lpc)
    nchunks = nmain + (1 if tail_px else 0)  # :1071
    max_px = max(min(lpc, lines) * samples, tail_px)  # :1072
    chunks = []
    for k in range(nchunks):
        is_tail = k >= nmain  # :1093
        l0 = lines if is_tail else k * lpc
        l1 = lines + 1 if is_tail else min(lines, l0 + lpc)  # :1094
        npx = tail_px if is_tail else (l1 - l0) * samples  # :1095
        chunks.append((l0 * samples, npx, l1 - l0, tail_px if is_tail else samples))  # :1116-1118
    return nchunks, max_px, lpc, chunks


def parent_detrend(lines, samples):  # xsw.hip:1441-1445 and :1450-1451
    n = lines * samples
    lpc = ceil_div(target_px(n, 4 << 20), samples) if samples > 0 else lines  # :1442
    lpc = max(lpc, 1)  # :1443
    nchunks = ceil_div(lines, lpc)
    max_px = min(lpc, lines) * samples  # :1445
    chunks = []
    for k in range(nchunks):
        l0 = k * lpc
        l1 = min(lines, l0 + lpc)
        chunks.append((l0 * samples, (l1 - l0) * samples, l1 - l0, samples))
    return nchunks, max_px, lpc, chunks


# (the parent's plan, cap_px, tile_rows, recut_flat) of the four users
USERS = {"device": (parent_device, 0, 1, 1), "sigma0_host": (parent_sigma0_host, 4 << 20, 4, 0),
         "host": (parent_host, 2 << 20, 4, 1), "detrend": (parent_detrend, 4 << 20, 1, 0)}

RASTERS = [(20000, 20000), (5000, 20000), (1, 1 << 16), (1, 4096 * 37 + 5), (15, 70001), (16, 4096), (1, 65535),
           (4, 100), (5, 7), (3, 9), (1000, 1001), (777, 12345), (2, 1 << 24)]


@pytest.mark.parametrize("user", sorted(USERS))
def test_chunk_plan_is_the_parents(ask, user):
    parent, cap, tile, recut = USERS[user]
    for (lines, samples), got in zip(RASTERS, ask(*[("plan", l, s, cap, tile, recut) for l, s in RASTERS])):
        nchunks, max_px, lpc, chunks = parent(lines, samples)
        g_lines, g_samples, g_lpc, g_nmain, g_tail, g_nchunks, g_max_px = got[:7]
        g_chunks = [tuple(got[7 + 4 * k: 11 + 4 * k]) for k in range(g_nchunks)]
        print(user, lines, samples, "->", got[:7])
        assert len(got) == 7 + 4 * g_nchunks
        assert (g_nchunks, g_max_px, g_lpc) == (nchunks, max_px, lpc), (user, lines, samples)
        assert g_chunks == chunks, (user, lines, samples)
        assert g_nmain + (1 if g_tail else 0) == g_nchunks and g_lines * g_samples + g_tail == lines * samples
        # the chunks tile the raster exactly once, in order, and none is larger than max_px
        at = 0
        for px0, npx, cl, cs in g_chunks:
            assert px0 == at and npx == cl * cs and 0 < npx <= g_max_px
            at += npx
        assert at == lines * samples
        if user in ("sigma0_host", "host"):  # whole 4-line tile rows, but for the last chunk and the tail
            assert all(c[2] % 4 == 0 for c in g_chunks[:g_nmain - 1])
    # XSW_MEM_DEVICE_SIGMA0_HOST refuses fewer than 4 lines before it plans (xsw.hip:998); the plan itself still tiles 3 x 9
    assert parent_sigma0_host(3, 9)[3] == [(0, 27, 3, 9)]


def test_samples_not_a_multiple_of_64_and_the_recut_rule_edges(ask):
    (flat, edge_lines, edge_n) = ask(("plan", 1, 1 << 16, 2 << 20, 4, 1), ("plan", 16, 4096, 2 << 20, 4, 1), ("plan", 1, 65535, 2 << 20, 4, 1))
    assert flat[:2] == [16, 4096] and flat[4] == 0 and flat[5] == 1  # re-cut, no tail
    assert edge_lines[:2] == [16, 4096] and edge_lines[4] == 0  # 16 lines: not re-cut (and 4096 wide as given)
    assert edge_n[:2] == [1, 65535] and edge_n[4] == 0  # fewer than 1 << 16 pixels: not re-cut
    (t37, t15) = ask(("plan", 1, 4096 * 37 + 5, 0, 1, 1), ("plan", 15, 70001, 0, 1, 1))
    assert t37[:7] == [37, 4096, 37, 1, 5, 2, 37 * 4096]
    n15 = 15 * 70001
    assert t15[:7] == [n15 // 4096, 4096, n15 // 4096, 1, n15 % 4096, 2, n15 // 4096 * 4096]


def test_worker_buffer_is_the_parents(ask):
    """Per chunked user and raster: list_cap, mask_strips (xsw.hip:1008 / :1079), the staging offsets (:1007 / :1075-1078) and
    the device buffer's bytes (:1009 / :1080), for float32 / float64, mono / dual-pol, with and without dsig_cr / anc / codes."""
    queries, expect = [], []
    for user in ("sigma0_host", "host"):
        parent = USERS[user][0]
        for lines, samples in RASTERS:
            _, max_px, lpc, _ = parent(lines, samples)
            list_cap = max(max_px // 8, 1 << 14) & ~1  # :1008 / :1079
            mask_strips = strips_for(max_px, lpc)
            queries.append(("caps", lines * samples, 0, max_px, lpc))
            expect.append((1, [list_cap, mask_strips]))
            for es, (co, cr), dsig, anc, codes in itertools.product((4, 8), ((1, 0), (1, 1), (0, 1)), (0, 1), (0, 1), (0, 1)):
                if user == "sigma0_host":  # :1007: only the sigma0 rasters travel
                    inc = dsig = anc = cc = ccr = 0
                    o_inc = o_co = 0
                    o_cr = o_co + (pad(max_px * es) if co else 0)
                    o_dsig = o_anc = o_cc = o_ccr = o_end = o_cr + (pad(max_px * es) if cr else 0)
                else:  # :1075-1078
                    inc, cc, ccr = 1, co or codes, cr and codes
                    o_inc = 0
                    o_co = o_inc + pad(max_px * es)
                    o_cr = o_co + (pad(max_px * es) if co else 0)
                    o_dsig = o_cr + (pad(max_px * es) if cr else 0)
                    o_anc = o_dsig + (pad(max_px * es) if dsig else 0)
                    o_cc = o_anc + (pad(max_px * es * 2) if anc else 0)
                    o_ccr = o_cc + (pad(max_px * 4) if cc else 0)
                    o_end = o_ccr + (pad(max_px * 4) if ccr else 0)
                queries.append(("stage", max_px, es, inc, co, cr, dsig, anc, cc, ccr))
                expect.append((0, [o_inc, o_co, o_cr, o_dsig, o_anc, o_cc, o_ccr, o_end]))
            o_masks = pad((TOTAL * list_cap + 16) * 4)  # relative to o_end; :1009 / :1080
            o_rec = o_masks + 2 * mask_strips * 8
            queries.append(("lists", list_cap, mask_strips))
            expect.append((9, [o_masks, o_rec, o_rec + B_SHARE * list_cap * REC_BYTES]))  # exactly the parent's: it padded here
    for q, (skip, want), got in zip(queries, expect, ask(*queries)):
        assert got[skip:] == want, q


def parent_context_lists(n, lines, test_cap):  # xsw.hip:682-706
    entries = max(test_cap, 16) if test_cap else max(n // 8, 1 << 16)  # :684-686
    want = (entries + 1) & ~1  # :692
    strips = strips_for(n, lines)
    total = (TOTAL * want + 16) * 4 + 2 * strips * 8 + B_SHARE * want * REC_BYTES  # :702
    o_masks = (16 + TOTAL * want) * 4  # :704
    return want, strips, o_masks, o_masks + 2 * strips * 8, total  # :705


@pytest.mark.parametrize("test_cap", [0, 40, 16, 41])
def test_context_lists_are_the_parents_up_to_the_mask_padding(ask, test_cap):
    rasters = RASTERS + [(70000, 70000)]
    caps = ask(*[("caps", l * s, test_cap, l * s, l) for l, s in rasters])
    for (lines, samples), (cap, _, strips) in zip(rasters, caps):
        n = lines * samples
        want, want_strips, p_masks, p_rec, p_total = parent_context_lists(n, lines, test_cap)
        assert (cap, strips) == (want, want_strips), (lines, samples)
        (got,) = ask(("lists", cap, strips))
        # counters at words 0 / 1 / 2 (xsw_invert_tu.hip:63, :76, :84), entries after the 16 counters in the order G, B, C
        # (:64, :76, :84), capacities clamped to what an unsigned counter can address (:65, :76, :84)
        assert got[0:9] == [0, 64, min(cap, 0xfffffff0), 4, 64 + 4 * cap, min(B_SHARE * cap, 0xfffffff0),
                            8, 64 + 4 * (1 + B_SHARE) * cap, min(C_SHARE * cap, 0xfffffff0)], (lines, samples)
        o_masks, o_rec, total = got[9:]
        print(lines, samples, "masks +%d B, total +%d B" % (o_masks - p_masks, total - p_total))
        assert 0 <= o_masks - p_masks <= 255 and o_masks % 8 == 0
        assert o_rec - o_masks == p_rec - p_masks == 2 * strips * 8  # the records start right after the two masks
        assert o_rec - p_rec == total - p_total == o_masks - p_masks  # nothing moved but by the padding
        assert 64 + 4 * TOTAL * cap <= o_masks  # the masks start after list C's last entry


def test_capacity_clamp(ask):
    (got,) = ask(("lists", 1 << 31, 64))
    assert [got[2], got[5], got[8]] == [1 << 31, 0xfffffff0, 0xfffffff0]


def parent_detrend_grid(lines, samples, wg=16):  # xsw.hip:1374-1384
    quads = (samples + 3) // 4
    gx = (quads + 255) // 256
    gy = (256 * wg + gx - 1) // gx
    gy = min(gy, lines)
    gy = min(gy, 65535)
    gy = max(gy, 1)
    lpb = ceil_div(lines, gy)
    return [gx, ceil_div(lines, lpb), lpb]


def parent_nesz_write_grid(lines, samples):  # xsw.hip:1484-1487
    egx = (samples + 256 * NESZ_EV - 1) // (256 * NESZ_EV)
    enb = max(1, min((256 * 16 + egx - 1) // egx, min(lines, 65535)))
    elpb = ceil_div(lines, enb)
    return [egx, ceil_div(lines, elpb), elpb]


def test_strip_grid_is_the_grid_of_detrend_and_of_the_nesz_write_pass(ask):
    shapes = RASTERS + [(1, 1), (1, 300), (70000, 3), (300000, 2), (70000, 70000), (300000, 1025), (65535, 17), (65536, 17)]
    det = ask(*[("grid", l, (s + 3) // 4, 0) for l, s in shapes])
    det8 = ask(*[("grid", l, (s + 3) // 4, 8) for l, s in shapes])  # -DXSW_DETREND_WG_PER_CU=8
    nesz = ask(*[("grid", l, ceil_div(s, NESZ_EV), 0) for l, s in shapes])
    for (lines, samples), d, d8, e in zip(shapes, det, det8, nesz):
        assert d == parent_detrend_grid(lines, samples), (lines, samples)
        assert d8 == parent_detrend_grid(lines, samples, 8), (lines, samples)
        assert e == parent_nesz_write_grid(lines, samples), (lines, samples)
        assert d[1] <= 65535 and e[1] <= 65535 and d[1] * d[2] >= lines and e[1] * e[2] >= lines


def source_define(name):
    """The integer a kernel source #defines `name` as (the kernels' own constants are not in the header under test)."""
    import re
    found = []
    for fn in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, fn)) as f:
            found += re.findall(r"^\s*#\s*define\s+" + name + r"\s+(\d+)\s*(?://.*)?$", f.read(), re.M)
    assert len(set(found)) == 1, (name, found)
    return int(found[0])


def grid_cap(fn, kernel):
    """The largest grid, in workgroups of 256 threads, that `fn` of csrc launches the grid-stride `kernel` with: the second
    argument of the std::min<long long>((n + 255) / 256, CAP) in that function, a product of integers.  The GPU tests that run
    such a kernel beyond one pass per thread size themselves by it and fail when the launch no longer reads so."""
    import re
    hits = []
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for m in re.finditer(r"\b" + fn + r"\([^;{]*\)\s*\{", text):
            body = text[m.end():]
            body = body[:body.index("\n}\n")]
            if "k_" + kernel in body:
                hits += re.findall(r"std::min<long long>\(\([^;]*?\+ 255\) / 256, ([0-9* ]+)\)", body)
    assert len(hits) == 1, (fn, kernel, hits)
    cap = 1
    for v in hits[0].split("*"):
        cap *= int(v)
    return cap


def test_grid_stride_caps():
    assert grid_cap("expand_codes_on", "expand") == 256 * 16 and grid_cap("xsw_grad_area", "grad_area") == 65536


def keep_instantiation(dtype, block, samples, base=0):
    """(T, W, B) of the k_grad_keep<T, W, B> that grad_keep launches (xsw_gradients.hip, the loop over w and XSW_KEEP_LAUNCH):
    the widest W among 16, 8, 4 above the element size that divides the block's row bytes and the raster's row bytes and to
    which the base address is aligned, else the element size; B = 2 only for float64 at W = 16 and 2 x 2 blocks."""
    es = {"float64": 8, "uint8": 1}[dtype]
    W = next((w for w in (16, 8, 4) if w > es and (block * es) % w == 0 and (samples * es) % w == 0 and base % w == 0), es)
    return {"float64": "double", "uint8": "uint8_t"}[dtype], W, 2 if es == 8 and W == 16 and block == 2 else 0


KEEP_INSTANTIATIONS = {("double", 16, 2), ("double", 16, 0), ("double", 8, 0), ("uint8_t", 16, 0), ("uint8_t", 8, 0), ("uint8_t", 4, 0),
                       ("uint8_t", 1, 0)}  # XSW_KEEP_LAUNCH's seven


def test_strip_shapes_stay_multi_line(ask):
    """Every raster of tests/strip_shapes.py, through the compiled strip_grid with its kernel's column divisor and workgroups per
    CU: at least two column strips, more than four lines per workgroup and no whole number of four-line groups, a shorter last
    workgroup that is no whole number of groups either -- and the grid the GPU tests place their special values by.  A change of
    strip_grid, XSW_DETREND_WG_PER_CU or XSW_NESZ_EV that sends these rasters back to one line per workgroup fails here, on the
    CPU, instead of silently emptying the GPU tests.
    The keep entries (k_grad_keep: strip_grid on the OUTPUT grid, one column per thread) hold to the same rules, but that with
    blocks wider than 2 x 2 they take ONE column strip, which must end in a partial wave; each selects, by grad_keep's width
    rule restated above, the instantiation it claims, all seven are claimed, and one entry at least trims a remainder row and
    a remainder column."""
    import strip_shapes
    assert NESZ_EV == source_define("XSW_NESZ_EV")
    wg_per_cu = {"detrend": source_define("XSW_DETREND_WG_PER_CU"), "dsig_flat": 0, "streaks": 0, "keep": 0}  # 0: strip_grid's default
    col_div = {"detrend": 4, "dsig_flat": NESZ_EV, "streaks": 1, "keep": 1}
    assert len(strip_shapes.SHAPES) == 12 and {e.kernel for e in strip_shapes.SHAPES.values()} == set(col_div)
    for key, e in sorted(strip_shapes.SHAPES.items()):
        assert e.col_div == col_div[e.kernel], key
        assert e.reduce >= 1 and (e.reduce == 1 or e.kernel == "keep"), key
        rows, cols = e.lines // e.reduce, e.samples // e.reduce
        assert rows == strip_shapes.grid_rows(key), key
        ((gx, gy, rpb),) = ask(("grid", rows, ceil_div(cols, e.col_div), wg_per_cu[e.kernel]))
        last = rows - (gy - 1) * rpb
        print(key, (e.lines, e.samples), "->", (gx, gy, rpb, last))
        if e.kernel == "keep" and e.reduce > 2:
            assert gx == 1 and cols % 64 != 0, key
        else:
            assert gx >= 2, key
        assert rpb >= 5 and rpb % 4 != 0, key
        assert 0 < last < rpb and last % 4 != 0, key
        assert (gx, gy, rpb, last) == e.grid, key
        assert strip_shapes.block_lines(key, -1) == list(range(rows - last, rows)), key
        assert strip_shapes.block_lines(key, 1) == list(range(rpb, 2 * rpb)), key
        if e.kernel == "keep":
            inst = keep_instantiation(e.dtype, e.reduce, e.samples)  # a whole allocation: the base is aligned to 16 bytes and more
            print(key, "-> k_grad_keep<%s, %d, %d>" % inst)
            assert inst == e.inst, key
            assert e.lines * e.samples * {"float64": 8, "uint8": 1}[e.dtype] < 70e6, key
        else:
            assert e.dtype is None and e.inst is None, key
    keep = [e for e in strip_shapes.SHAPES.values() if e.kernel == "keep"]
    assert len(keep) == 7 and {e.inst for e in keep} == KEEP_INSTANTIATIONS
    assert any(e.lines % e.reduce and e.samples % e.reduce for e in keep)
    assert any(e.reduce <= 2 for e in keep) and any(e.reduce > 2 for e in keep)
    # the width rule at what the entries do not vary: a base 8 bytes off a 16-byte boundary, rows of 8 and 4 bytes, bytes alone
    assert keep_instantiation("float64", 2, 516, base=8) == ("double", 8, 0) and keep_instantiation("float64", 1, 516) == ("double", 8, 0)
    assert keep_instantiation("uint8", 16, 144, base=8) == ("uint8_t", 8, 0) and keep_instantiation("uint8", 16, 152) == ("uint8_t", 8, 0)
    assert keep_instantiation("uint8", 16, 148) == ("uint8_t", 4, 0) and keep_instantiation("uint8", 1, 144) == ("uint8_t", 1, 0)
    assert strip_shapes.SHAPES["streaks"].grid[2] > 8  # the streaks pass: a second unrolled group in every workgroup
    # the vector and the element-wise raster of a kernel differ in the sample count's divisibility alone
    for a, b, q in (("detrend_vec", "detrend_elem", 4), ("dsig_flat_vec", "dsig_flat_elem", 2)):
        assert strip_shapes.SHAPES[a].samples % q == 0 and strip_shapes.SHAPES[b].samples % q != 0
        assert strip_shapes.SHAPES[a].grid == strip_shapes.SHAPES[b].grid
