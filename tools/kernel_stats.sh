# rocprofv3 --kernel-trace --stats of one `bench.py --full` command (roofline, A/B and fresh-inputs legs included); copies the
# per-kernel summary to $OUT/<name>_kernel_stats.csv and the JSON line of that run to $OUT/<name>_line.json
#   bash tools/kernel_stats.sh <name> <bench.py flags ...>          (OUT defaults to profile_out/ in the repository root)
set -e
NAME=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/profile_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/ks_$NAME" -- python3 "$R/bench.py" --full --no-cpu-baseline "$@" > "$OUT/ks_$NAME.log" 2>&1
F=$(find "$OUT/ks_$NAME" -name "*kernel_stats.csv" | head -1)
cp "$F" "$OUT/${NAME}_kernel_stats.csv"
grep '^{"metric' "$OUT/ks_$NAME.log" | tail -1 > "$OUT/${NAME}_line.json"
cut -c1-400 "$OUT/${NAME}_line.json"
head -8 "$OUT/${NAME}_kernel_stats.csv" | cut -c1-200
