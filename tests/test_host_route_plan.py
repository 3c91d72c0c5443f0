"""CPU: the route plan of an inversion launch (csrc/xsw_plan.hpp: RouteKnobs, RouteFacts, ChainPlan), compiled with a host C++
compiler and compared with what `launch_invert` decided inline before the plan existed.  The expected values are those
expressions restated here (file:line of csrc/xsw_invert_tu.hip at commit dfe8531 beside each, other files named), never the
header's own output.

Cases (counted where they are built, the counts asserted): 429 plans -- 36 shape x polarisation x statistics combinations, 13
for the route gate (all on, each of its eleven facts off alone, cross-pol tables not monotone without a cross-pol raster), 8 algo x
polarisation, 2 strip-mask sizes, 8 table cases, 350 for the environment (25 environments x 14 calls), 12 around the launch
limits -- and 34 readings of the environment (the 25, and 9 more for the clamps, the defaults and the list knobs)."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xsarsea_amd", "csrc")
PRUNED, EXHAUSTIVE, EXACT, EXHAUSTIVE_F64 = 1, 2, 3, 4  # include/xsw.h:51-55
WAVES = dict(band_wg=4, band2=4, blocks=4)  # XSW_BAND_WG_WAVES, XSW_BAND2_WAVES (xsw_band.hpp:90, :110), XSW_BLOCKS_WAVES (xsw_blocks.hpp:36)
NEVER = 0x7fffffff

KNOBS = ("block_min", "no_band", "long_run", "no_records", "no_blocks_kernel", "b2_area", "b2_crowd", "b2_wide", "arc_min",
         "arc_crowd", "b2_refine_min", "b2_rows_max", "tail_sweep", "no_strip_masks", "list_cap_test", "fail_list_alloc")
FACTS = ("prunable", "co_off32", "band_mul24", "cr_monotone", "blk_span_ok", "mono_rows", "inv_rows", "blk", "csphi32", "tail_min",
         "n_w", "n_phi", "lines", "samples", "n", "algo", "s_co", "s_cr", "mono", "stats", "stats_chain", "lists", "mask_strips")
PLAN = ("route", "limit", "nblocks", "block_min", "count_inst", "band2", "records", "blocks3", "masks", "nstrips", "long_run",
        "area_max", "b2_crowd", "area_crowd_max", "wide_min", "arc_min", "arc_crowd", "b2_refine_min", "b2_rows_max", "tail_max",
        "band_grid_x", "band_grid_y", "band2_blocks", "blocks3_blocks", "list_blocks")
ROUTES = ("exhaustive", "chain", "one_pruned", "one_exact", "too_large")  # ChainPlan::Route
LIMITS = (None, "nblocks", "band_groups", "band_cols")                    # ChainPlan::Limit

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "xsw_plan.hpp"
static void print_knobs(const RouteKnobs &k)
{
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %d\n", k.block_min, (int)k.no_band, k.long_run, (int)k.no_records, (int)k.no_blocks_kernel,
           k.b2_area, k.b2_crowd, k.b2_wide, k.arc_min, k.arc_crowd, k.b2_refine_min, k.b2_rows_max, k.tail_sweep, (int)k.no_strip_masks,
           k.list_cap_test, (int)k.fail_list_alloc);
}
int main()
{
    char cmd[16];
    long long a[42];
    auto rd = [&](int n) { for (int i = 0; i < n; ++i) if (scanf("%lld", &a[i]) != 1) return false; return true; };
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "env")) print_knobs(RouteKnobs::from_env());
        else if (!strcmp(cmd, "defaults")) print_knobs(RouteKnobs{});
        else if (!strcmp(cmd, "plan") && rd(42)) {  // 16 knobs, 23 facts, 3 waves, in the order of KNOBS, FACTS, WAVES of the test
            RouteKnobs k;
            RouteFacts f;
            const long long *v = a;
            k.block_min = (int)*v++; k.no_band = *v++; k.long_run = (int)*v++; k.no_records = *v++; k.no_blocks_kernel = *v++;
            k.b2_area = (int)*v++; k.b2_crowd = (int)*v++; k.b2_wide = (int)*v++; k.arc_min = (int)*v++; k.arc_crowd = (int)*v++;
            k.b2_refine_min = (int)*v++; k.b2_rows_max = (int)*v++; k.tail_sweep = (int)*v++; k.no_strip_masks = *v++;
            k.list_cap_test = *v++; k.fail_list_alloc = *v++;
            f.prunable = *v++; f.co_off32 = *v++; f.band_mul24 = *v++; f.cr_monotone = *v++; f.blk_span_ok = *v++;
            f.mono_rows = *v++; f.inv_rows = *v++; f.blk = *v++; f.csphi32 = *v++; f.tail_min = *v++;
            f.n_w = (int)*v++; f.n_phi = (int)*v++; f.lines = *v++; f.samples = *v++; f.n = *v++; f.algo = (int)*v++;
            f.s_co = *v++; f.s_cr = *v++; f.mono = *v++; f.stats = *v++; f.stats_chain = *v++; f.lists = *v++; f.mask_strips = (size_t)*v++;
            const ChainWaves w{(int)v[0], (int)v[1], (int)v[2]};
            const ChainPlan p(k, f, w);
            printf("%d %d %lld %d %d %d %d %d %d %zu %d %d %d %d %d %d %d %d %d %d %u %u %u %u %u\n", (int)p.route, (int)p.limit, p.nblocks, p.block_min,
                   (int)p.count_inst, (int)p.band2, (int)p.records, (int)p.blocks3, (int)p.masks, p.nstrips, p.long_run, p.area_max, p.b2_crowd,
                   p.area_crowd_max, p.wide_min, p.arc_min, p.arc_crowd, p.b2_refine_min, p.b2_rows_max, p.tail_max, p.band_grid_x, p.band_grid_y,
                   p.band2_blocks, p.blocks3_blocks, p.list_blocks);
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("g++", "clang++", "c++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, clang++, c++) on PATH")
    td = tmp_path_factory.mktemp("host_route_plan")
    src, exe = td / "driver.cpp", td / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])

    def run(text, env=None):
        """One output line per command, as lists of ints.  env: the XSW_* variables the driver sees (none of the caller's)."""
        clean = {k: v for k, v in os.environ.items() if not k.startswith("XSW_")}
        out = subprocess.run([str(exe)], input=text, text=True, capture_output=True, check=True, env=dict(clean, **(env or {}))).stdout
        return [[int(v) for v in ln.split()] for ln in out.splitlines()]

    return run


# ---- the parent's knobs: env_int / env_flag of xsw_host.hpp:94-99 at dfe8531 and every call of them for these variables
def env_int(env, name, dflt, lo=None, hi=None):  # xsw_host.hpp:94-98: atoll, then clamped; unset: the default, unclamped
    if name not in env:
        return dflt
    v = int(env[name])
    if lo is not None:
        v = max(v, lo)
    if hi is not None:
        v = min(v, hi)
    return v


def parent_knobs(env):
    flag = lambda name: int(name in env)  # xsw_host.hpp:99
    return dict(
        block_min=env_int(env, "XSW_BLOCK_MIN", 1024, 0),          # :59, default :41
        no_band=flag("XSW_NO_BAND"),                               # :61
        long_run=env_int(env, "XSW_LONG_RUN", 5, 0),               # :74, default :23
        no_records=flag("XSW_NO_RECORDS"),                         # :78
        no_blocks_kernel=flag("XSW_NO_BLOCKS_KERNEL"),             # :83
        b2_area=env_int(env, "XSW_B2_AREA", 2048, 1),              # :87, default :20
        b2_crowd=env_int(env, "XSW_B2_CROWD", 24, 1),              # :89, default :32
        b2_wide=env_int(env, "XSW_B2_WIDE", 0, 0),                 # :92, default :35
        arc_min=env_int(env, "XSW_ARC_MIN", 32),                   # :94, default :26 (not clamped)
        arc_crowd=env_int(env, "XSW_ARC_CROWD", 48, 1),            # :95, default :29
        b2_refine_min=env_int(env, "XSW_B2_REFINE_MIN", 16, 0),    # :98, default :38
        b2_rows_max=env_int(env, "XSW_B2_ROWS_MAX", 4096, 1),      # :100, default xsw_band2.hpp:52
        tail_sweep=env_int(env, "XSW_TAIL_SWEEP", 256, 0, 30000),  # :102, default xsw_band.hpp:76
        no_strip_masks=flag("XSW_NO_STRIP_MASKS"),                 # :105
        list_cap_test=env_int(env, "XSW_LIST_CAP_TEST", 0, 16),    # xsw.hip:490
        fail_list_alloc=flag("XSW_FAIL_LIST_ALLOC"),               # xsw.hip:494
    )


# ---- the parent's launch_invert (xsw_invert_tu.hip:44-162), as far as it decides anything
def parent_launch(K, F, W):
    lines, samples, algo = F["lines"], F["samples"], F["algo"]
    strips_per_line, line_groups = (samples + 63) // 64, (lines + 3) // 4  # :49
    nblocks = 8 * ((strips_per_line + 7) // 8) * line_groups               # :50
    if nblocks > 0x7fffffff:                                               # :51
        return dict(route="too_large", limit="nblocks")
    if algo in (EXHAUSTIVE, EXHAUSTIVE_F64):                               # :53
        return dict(route="exhaustive", nblocks=nblocks)
    P = dict(nblocks=nblocks, block_min=K["block_min"])                    # :59-60
    if (algo == PRUNED and not K["no_band"] and F["lists"] and F["s_co"] and F["prunable"] and F["mono_rows"] and F["inv_rows"]
            and F["co_off32"] and F["band_mul24"] and (not F["s_cr"] or F["cr_monotone"]) and F["n"] < (1 << 32)):  # :62-63
        count_inst = bool(F["stats"] and not F["stats_chain"])             # :75
        band2 = K["long_run"] > 0 and not count_inst                       # :76
        P.update(count_inst=count_inst, band2=band2,
                 records=bool(band2 and not K["no_records"]),              # :80
                 blocks3=bool(F["blk"] and F["blk_span_ok"] and not K["no_blocks_kernel"] and F["n_w"] < 32768 and F["n_phi"] < 32768),  # :84
                 long_run=K["long_run"],                                   # :86
                 area_max=K["b2_area"] if F["blk"] else 0x7fffffff,        # :88
                 b2_crowd=K["b2_crowd"],                                   # :90
                 area_crowd_max=1 << 20,                                   # :91
                 wide_min=K["b2_wide"] if K["b2_wide"] > 0 else 0x7fffffff,  # :93
                 arc_min=K["arc_min"] if (K["arc_min"] > 0 and F["csphi32"]) else 0x7fffffff,  # :96
                 arc_crowd=K["arc_crowd"],                                 # :97
                 b2_refine_min=K["b2_refine_min"],                         # :99
                 b2_rows_max=K["b2_rows_max"],                             # :101
                 tail_max=K["tail_sweep"] if (band2 and F["tail_min"]) else 0)  # :103
        nstrips = strips_per_line * lines                                  # :106
        P.update(nstrips=nstrips, masks=bool(nstrips <= F["mask_strips"] and not K["no_strip_masks"]))  # :107
        P["list_blocks"] = min(nblocks, 256 * 8)                           # :112
        cols_per_xcd = (strips_per_line + 7) // 8                          # :114
        band_groups = (lines + W["band_wg"] - 1) // W["band_wg"]           # :115
        if 8 * band_groups > 0x7fffffff or cols_per_xcd > 65535:           # :116
            return dict(route="too_large", limit="band_groups" if 8 * band_groups > 0x7fffffff else "band_cols")
        P.update(route="chain", band_grid_x=8 * band_groups, band_grid_y=cols_per_xcd,  # :117
                 band2_blocks=min(nblocks, 256 * W["band2"]),              # :135
                 blocks3_blocks=min(nblocks, 256 * W["blocks"]))           # :141
        return P
    P["route"] = "one_pruned" if algo == PRUNED else "one_exact"           # :153-158 (k_invert<.., 1, ..> or k_invert<.., 3>)
    return P


def facts(lines=160, samples=900, **over):
    """Everything the gate asks for, a mono call without statistics, work lists whose masks fit exactly."""
    F = dict(prunable=1, co_off32=1, band_mul24=1, cr_monotone=1, blk_span_ok=1, mono_rows=1, inv_rows=1, blk=1, csphi32=1, tail_min=1,
             n_w=499, n_phi=181, lines=lines, samples=samples, n=lines * samples, algo=PRUNED, s_co=1, s_cr=0, mono=1, stats=0, stats_chain=0,
             lists=1, mask_strips=(samples + 63) // 64 * lines)
    F.update(over)
    return F


DUAL = dict(s_cr=1, mono=0)
SHAPES = [(1, 1), (1, 63), (3, 65), (5, 129), (160, 900), (20000, 20000)]
STATS = [dict(), dict(stats=1), dict(stats=1, stats_chain=1)]  # off, the statistics instantiation, chain statistics


def check(driver, cases):
    """cases: (what, knobs, facts, waves).  Every field the parent computed on the route it took must be the plan's."""
    text = "".join("plan " + " ".join(str(int(d[k])) for d, keys in ((K, KNOBS), (F, FACTS), (W, ("band_wg", "band2", "blocks"))) for k in keys) + "\n"
                   for _, K, F, W in cases)
    got = driver(text)
    assert len(got) == len(cases)
    routes = set()
    for (what, K, F, W), line in zip(cases, got):
        plan = dict(zip(PLAN, line))
        plan["route"], plan["limit"] = ROUTES[plan["route"]], LIMITS[plan["limit"]]
        want = parent_launch(K, F, W)
        for key, value in want.items():
            assert plan[key] == value, (what, key, plan[key], value)
        routes.add(want["route"])
    return routes


def test_defaults_are_the_parents(driver):
    (env, dflt) = driver("env\ndefaults\n")
    assert dict(zip(KNOBS, env)) == dict(zip(KNOBS, dflt)) == parent_knobs({})


# the defaults, what the GPU route tests set (tests/test_gpu_kernel.py: test_long_run_kernel, test_block_pyramid_routes,
# test_tail_cut_keeps_saturating_windows_in_the_band_kernels) and, last, the forced-refinement soak of profiles/README.md
ENVS = [{}, {"XSW_LONG_RUN": "0"}, {"XSW_LONG_RUN": "1"}, {"XSW_B2_WIDE": "16"}, {"XSW_ARC_MIN": "0"}, {"XSW_ARC_MIN": "8", "XSW_ARC_CROWD": "1"},
        {"XSW_B2_CROWD": "1"}, {"XSW_B2_CROWD": "65"}, {"XSW_B2_REFINE_MIN": "0"}, {"XSW_B2_REFINE_MIN": "65", "XSW_B2_CROWD": "65"},
        {"XSW_B2_REFINE_MIN": "65"}, {"XSW_B2_ROWS_MAX": "8"}, {"XSW_TAIL_SWEEP": "0"}, {"XSW_BLOCK_MIN": "0"}, {"XSW_NO_BAND": "1"},
        {"XSW_NO_RECORDS": "1"}, {"XSW_NO_BLOCKS_KERNEL": "1"}, {"XSW_NO_STRIP_MASKS": "1"}, {"XSW_BLOCK_MIN": "0", "XSW_NO_BAND": "1"},
        {"XSW_LONG_RUN": "1", "XSW_NO_RECORDS": "1"}, {"XSW_LONG_RUN": "1", "XSW_NO_STRIP_MASKS": "1", "XSW_LIST_CAP_TEST": "300"},
        {"XSW_LONG_RUN": "0", "XSW_NO_BLOCKS_KERNEL": "1"}, {"XSW_LIST_CAP_TEST": "300"}, {"XSW_FAIL_LIST_ALLOC": "1"},
        {"XSW_ARC_MIN": "4", "XSW_ARC_CROWD": "1", "XSW_B2_REFINE_MIN": "0", "XSW_B2_CROWD": "1"}]
# the clamps (and the one knob without: a negative XSW_ARC_MIN is "never", like 0), empty values, the list knobs
ENVS_READ_ONLY = [{"XSW_TAIL_SWEEP": "30001"}, {"XSW_TAIL_SWEEP": "-1"}, {"XSW_B2_AREA": "0", "XSW_B2_CROWD": "0", "XSW_ARC_CROWD": "0", "XSW_B2_ROWS_MAX": "0"},
                  {"XSW_ARC_MIN": "-3"}, {"XSW_BLOCK_MIN": "-1", "XSW_LONG_RUN": "-1", "XSW_B2_WIDE": "-1", "XSW_B2_REFINE_MIN": "-1"},
                  {"XSW_LIST_CAP_TEST": "5"}, {"XSW_LIST_CAP_TEST": "41"}, {"XSW_NO_BAND": "0", "XSW_NO_RECORDS": ""}, {"XSW_B2_AREA": "100000000"}]


def test_environment_is_read_as_the_parent_read_it(driver):
    envs = ENVS + ENVS_READ_ONLY
    assert len(envs) == 34
    for env in envs:
        (got,) = driver("env\n", env)
        assert dict(zip(KNOBS, got)) == parent_knobs(env), env


def test_plan_is_the_parents_launch(driver):
    cases = []
    add = lambda what, K, F, W=WAVES: cases.append((what, K, F, W))
    K0 = parent_knobs({})
    for shape in SHAPES:
        for pol in (dict(), DUAL):
            for st in STATS:
                add(("shape", shape, pol, st), K0, facts(*shape, **pol, **st))
    assert len(cases) == 36
    # the route gate (:62-63): all on (dual-pol, so that cr_monotone counts), each of the eleven off alone
    gate_off = [dict(algo=EXACT), dict(lists=0), dict(s_co=0), dict(prunable=0), dict(mono_rows=0), dict(inv_rows=0), dict(co_off32=0),
                dict(band_mul24=0), dict(cr_monotone=0), dict(lines=65536, samples=65536, n=1 << 32, mask_strips=1 << 30)]
    add("gate: all on", K0, facts(**DUAL))
    for off in gate_off:
        add(("gate", off), K0, facts(**dict(DUAL, **off)))
    add("gate: XSW_NO_BAND", parent_knobs({"XSW_NO_BAND": "1"}), facts(**DUAL))
    add("gate: no cross-pol raster, tables not monotone", K0, facts(cr_monotone=0))
    assert len(cases) == 36 + 13
    for algo in (PRUNED, EXACT, EXHAUSTIVE, EXHAUSTIVE_F64):
        for pol in (dict(), DUAL):
            add(("algo", algo, pol), K0, facts(5, 129, algo=algo, **pol))
    nstrips = 15 * 160  # (900 + 63) // 64 strips per line
    add("masks one word short", K0, facts(mask_strips=nstrips - 1))
    add("masks fit exactly", K0, facts(mask_strips=nstrips))
    for over in (dict(blk=0), dict(csphi32=0), dict(tail_min=0), dict(blk_span_ok=0), dict(n_w=32768), dict(n_phi=32768), dict(n_w=32767, n_phi=32767),
                 dict(blk=0, csphi32=0, tail_min=0)):
        add(("tables", over), K0, facts(**over))
    assert len(cases) == 36 + 13 + 8 + 2 + 8
    # every environment on calls that look at different knobs
    calls = [facts(), facts(**DUAL), facts(stats=1), facts(stats=1, stats_chain=1), facts(blk=0), facts(csphi32=0), facts(tail_min=0), facts(lists=0),
             facts(mask_strips=nstrips - 1), facts(3, 65), facts(1, 1), facts(algo=EXACT), facts(algo=EXHAUSTIVE), facts(n_w=32768)]
    for env in ENVS:
        for F in calls:
            add(("env", env), parent_knobs(env), F)
    assert len(cases) == 67 + 25 * 14
    # launch limits, both sides.  k_invert_band's y: cols_per_xcd = ceil(ceil(samples / 64) / 8) at 65535 / 65536 (:116)
    add("cols_per_xcd 65535", K0, facts(1, 65535 * 512))
    add("cols_per_xcd 65536", K0, facts(1, 65535 * 512 + 1))
    # nblocks (:51) is a multiple of 8: 0x7ffffff8 is the last that fits (16383 x 16385 = 2^28 - 1 tile columns x line groups), 2^31 the first that
    # does not; at these sizes n >= 2^32, so the one-kernel route asks
    for algo in (PRUNED, EXACT, EXHAUSTIVE):
        add("nblocks 0x7ffffff8", K0, facts(4 * 16385, 512 * 16383, algo=algo))
        add("nblocks 0x80000000", K0, facts(4 * 16384, 512 * 16384, algo=algo))
    # 8 * band_groups (:116) with the product's XSW_BAND_WG_WAVES = 4 is at most nblocks, which is asked first (:51) ...
    add("band_groups behind nblocks", K0, facts(4 * ((1 << 28) - 1), 1))
    add("band_groups behind nblocks", K0, facts(4 << 28, 1))
    # ... so its own two sides are reached with two-wave workgroups: 0x7ffffff8 and 2^31
    W2 = dict(WAVES, band_wg=2)
    add("8 * band_groups 0x7ffffff8", K0, facts(2 * ((1 << 28) - 1), 1), W2)
    add("8 * band_groups 0x80000000", K0, facts(2 << 28, 1), W2)
    assert len(cases) == 429
    routes = check(driver, cases)
    assert routes == set(ROUTES)
    wants = [parent_launch(K, F, W) for _, K, F, W in cases]
    assert {w.get("limit") for w in wants} == set(LIMITS)
    # the corners the issue names, seen at least once each among the expected values
    chain = [w for w in wants if w["route"] == "chain"]
    assert {w["area_max"] for w in chain} >= {2048, NEVER} and {w["wide_min"] for w in chain} >= {16, NEVER}
    assert {w["arc_min"] for w in chain} >= {8, 32, NEVER} and {w["tail_max"] for w in chain} >= {0, 256}
    assert all(w["area_crowd_max"] == 1 << 20 for w in chain)
    for key in ("count_inst", "band2", "records", "blocks3", "masks"):
        assert {w[key] for w in chain} == {False, True}, key
