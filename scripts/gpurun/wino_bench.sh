# Winograd trunk in the product path: trunk/ACT parity tests, then a short full bench line (no CPU leg),
# written under $OUT
# usage: [OUT=dir] bash <this script> <tag>     (from the repository root)
OUT=${OUT:-bench_out} && mkdir -p "$OUT" &&
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread -m gpu tests/test_nn_gpu.py -k "trunk or f32" tests/test_act_full_gpu.py tests/test_winograd_gpu.py > "$OUT/wino_bench_tests_$1.log" 2>&1 &&
timeout -k 10 600 python bench.py --full --steps 12 --warmup 3 --no_cpu_baseline > "$OUT/wino_bench_$1.json" 2> "$OUT/wino_bench_$1.err"
