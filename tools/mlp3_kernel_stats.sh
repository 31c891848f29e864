# rocprofv3 --kernel-trace --stats (no counters in the same run) of the hipGraph loop on the sphere script's models
# (tools/time_mlp3.py, batch 100, 2 000 timed steps per shape): shows the launches per step of csrc/fused_mlp3.hip.
# Copies the per-kernel summary to $OUT/mlp3_kernel_stats.csv.
#   bash tools/mlp3_kernel_stats.sh          (OUT defaults to profile_out/ in the repository root)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/profile_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/ks_mlp3" -- python3 "$R/tools/time_mlp3.py" --batches 100 --steps 2000 --repeats 1 > "$OUT/ks_mlp3.log" 2>&1
F=$(find "$OUT/ks_mlp3" -name "*kernel_stats.csv" | head -1)
cp "$F" "$OUT/mlp3_kernel_stats.csv"
cat "$OUT/ks_mlp3.log" | grep "^tree=" | cut -c1-200
head -8 "$OUT/mlp3_kernel_stats.csv" | cut -c1-200
