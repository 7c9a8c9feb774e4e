#!/bin/bash
# The state-layout study on one box (run on the GPU box from the repo root,
# tools/ubench_layout built):  bash tools/gpu_ubench_layout.sh OUTDIR
# 1. tools/parent_stats.py: the survivors of the bench's C2 run and the lines
#    each layout would fetch; its ancestors feed the "c2" pattern below.
# 2. tools/ubench_layout: gather + store timings per layout and pattern.
# 3. FETCH_SIZE and WRITE_SIZE of the same kernels, each counter a run of its
#    own, summarised per kernel as MB per launch (FETCH_SIZE both as counted and
#    doubled: tools/pmc_json.py on gfx950's half count of streaming reads).
set -e
OUT=$PWD/${1:-out/ubench_layout}
mkdir -p $OUT
export TMPDIR=/tmp
ANC=$(mktemp)
trap 'rm -f $ANC' EXIT
timeout -k 10 240 python3 tools/parent_stats.py --out $ANC > $OUT/parent_stats.txt 2>&1 || { tail -20 $OUT/parent_stats.txt; exit 1; }
tail -6 $OUT/parent_stats.txt
timeout -k 10 120 tools/ubench_layout $ANC > $OUT/ubench_layout.txt 2>&1 || { tail -20 $OUT/ubench_layout.txt; exit 1; }
cat $OUT/ubench_layout.txt
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 240 rocprofv3 --pmc $ctr -d $OUT/pmc_$ctr -o run --output-format csv -- tools/ubench_layout $ANC --pmc > $OUT/pmc_$ctr.log 2>&1 || { tail -20 $OUT/pmc_$ctr.log; exit 1; }
done
python3 - $OUT <<'PY' | tee $OUT/ubench_layout_pmc.txt
import collections, csv, glob, re, sys
out = sys.argv[1]
lay = ["pair_64", "row", "row_lds3", "row_lds5", "chunk_32", "row_ldsh"]
pat = ["id", "c2", "u4"]
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"{out}/pmc_*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r"k_lay<(\d+), *(\d+)>", r["Kernel_Name"])
        if m:
            agg[f"{lay[int(m.group(1))]}.{pat[int(m.group(2))]}"][r["Counter_Name"]].append(float(r["Counter_Value"]))
print(f"{'variant':14s} {'FETCH_SIZE MB':>14s} {'x2 MB':>8s} {'WRITE_SIZE MB':>14s}   (per launch, mean of the launches; KiB counters x 1024)")
for p in ("c2", "u4", "id"):
    for l in lay:
        d = agg.get(f"{l}.{p}")
        if not d:
            continue
        f = sum(d["FETCH_SIZE"]) / max(len(d["FETCH_SIZE"]), 1) * 1024 / 1e6
        w = sum(d["WRITE_SIZE"]) / max(len(d["WRITE_SIZE"]), 1) * 1024 / 1e6
        print(f"{l + '.' + p:14s} {f:14.1f} {2 * f:8.1f} {w:14.1f}")
PY
