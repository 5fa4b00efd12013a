# the full bench line (no CPU leg) and its rocprofv3 kernel-trace summary, written under $OUT
# usage: [OUT=dir] bash <this script> <tag>     (from the repository root)
OUT=${OUT:-bench_out} && mkdir -p "$OUT" &&
timeout -k 10 420 python bench.py --full --no_cpu_baseline > "$OUT/bench_$1.json.log" 2> "$OUT/bench_$1.err" &&
timeout -k 10 480 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$1" -o run -- python3 bench.py --full --no_cpu_baseline > "$OUT/bench_$1_under_rocprof.json.log" 2> "$OUT/prof_$1.err"
