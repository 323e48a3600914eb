# fused forward builder against the tuned library GEMM + epilogue, per BASELINE config.  Usage: bash scripts/builder_ab.sh
export OUT=$(realpath -m "${OUT:-bench_out}")   # bench lines and profiler output
mkdir -p "$OUT"
for c in c3 c2 c4 c5; do
  st=16; [ $c = c5 ] && st=8; [ $c = c4 ] && st=8
  for mode in fused library fused library; do
    FTR_BUILDER_GEMM=$mode timeout -k 10 300 python bench.py --full --config $c --steps $st --warmup 4 --no-cpu-baseline --no-dense --no-graph > $OUT/ab.json 2> $OUT/ab.err || { echo "bench failed"; tail -5 $OUT/ab.err; exit 1; }
    python - "$c" "$mode" <<'PY'
import json, os, sys
d = json.load(open(os.environ["OUT"] + "/ab.json")); k = d["kernels"]
pick = {n: round(v["avg_us"], 1) for n, v in k.items() if "logprobs" in n and "pruned" not in n or "gemm" in n}
print(sys.argv[1], sys.argv[2], d["ms_per_step"], pick)
PY
  done
done
