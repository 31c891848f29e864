# Two --pmc passes of SQ counters (--kernel-trace only) over `bench.py --full --steps 20 --warmup 5`; prints per-launch averages
# for the fused kernels (the per-sample A/B leg of --full).  Output under $OUT (default: profile_out/ in the repository root).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/profile_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
BENCH="python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-roofline"
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS --output-format csv -d "$OUT/pmc1" -- $BENCH > "$OUT/pmc1.log" 2>&1
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_IFETCH SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_ACTIVE_INST_SCA --output-format csv -d "$OUT/pmc2" -- $BENCH > "$OUT/pmc2.log" 2>&1
python3 - "$OUT" <<'PY'
import csv, glob, collections, os, sys
for d in ("pmc1","pmc2"):
    for f in glob.glob(os.path.join(sys.argv[1], d, "**", "*counter_collection.csv"), recursive=True):
        agg=collections.defaultdict(lambda: collections.defaultdict(list))
        for r in csv.DictReader(open(f)):
            k=r["Kernel_Name"][:40]
            agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for k,v in agg.items():
            if "fused" not in k: continue
            print(d,k,{c: round(sum(x)/len(x)) for c,x in v.items()})
PY
