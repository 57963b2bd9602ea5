# S10 bench with its PMC passes (the fused residual sweep's traffic included), no CPU baseline
# Output: $OUT/bench_pmc.json (default build/bench_pmc/)
set -e
cd $GRAFT_REPO_ROOT
OUT=${OUT:-build/bench_pmc}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 500 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > "$OUT/bench_pmc.json" 2> "$OUT/bench_pmc.err"
