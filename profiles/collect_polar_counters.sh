#!/bin/bash
# Issue / wait / LDS counters of k_wind_polar beside k_wind_grid and k_ancillary_model on the 20000 x 20000 workload of
# profiles/bench_polar.py (staged path only, every variant dispatched once), two rocprofv3 --pmc passes of one process each
# (counters are collected in runs of their own: no tracing beside them).  Run on the GPU machine from the repository root:
#   bash profiles/collect_polar_counters.sh [out_dir]      -> <out_dir>/summary.json, by default build/polar_counters/  (kept as
#   profiles/polar_pmc_counters_summary.json)
# A pass that fails ends the script.
set -e -o pipefail
R=$(pwd)
OUT=${1:-$R/build/polar_counters}
mkdir -p "$OUT"; rm -rf "$OUT"/p[0-9]*
i=0
for set in \
 "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA" \
 "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE" ; do
  i=$((i+1))
  timeout -k 10 280 rocprofv3 --pmc $set --output-format csv -d "$OUT/p$i" -- python3 "$R/profiles/bench_polar.py" --paths lds --steps 1 --warmup 0 --out "" > "$OUT/p$i.log" 2>&1
done
python3 - "$OUT" <<'PY'
import collections, csv, glob, json, re, sys
out = sys.argv[1]
px = 20000 * 20000
# per kernel name, the dispatches in order: bench_polar.py runs "2km x 4" before "1km x 72" for each source
label = {"k_wind_polar": ["2km x 4", "1km x 72"], "k_wind_grid": ["0.1"], "k_ancillary_model": [""]}
rows = collections.defaultdict(dict)
for f in glob.glob(out + "/p*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        if any(k in name for k in label):
            d = rows[(name, re.search(r"/p(\d)/", f).group(1))].setdefault(int(r.get("Dispatch_Id") or r["Correlation_Id"]), {})
            d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])   # (one row per counter instance)
res = {}
for (name, _), by_id in sorted(rows.items()):
    key = next(k for k in label if k in name)
    src = "complex128" if "SrcC128" in name else "codes" if "SrcCodes" in name else ""
    for k, d in enumerate(sorted(by_id)):
        tag = " ".join(x for x in (key, src, label[key][min(k, len(label[key]) - 1)]) if x)
        res.setdefault(tag, {}).update({c: round(v / px, 3) if c != "GRBM_GUI_ACTIVE" else v for c, v in by_id[d].items()})
json.dump({"per_pixel_except_GRBM_GUI_ACTIVE": res, "raster": [20000, 20000]}, open(out + "/summary.json", "w"), indent=1)
print(json.dumps(res, indent=1))
PY
rm -rf "$OUT"/p[0-9]   # the raw per-dispatch CSVs are large; the summary and the logs stay
