export OUT=$(realpath -m "${OUT:-bench_out}")   # bench lines and profiler output
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -m gpu -q -x > $OUT/pytest.log 2>&1; rc=$?; echo "pytest exit $rc" >> $OUT/pytest.log
grep -E "FAILED|passed|failed" $OUT/pytest.log | tail -15
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err; rc=$?; echo "bench exit $rc" >> $OUT/bench.err
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then exit $rc; fi
python - <<'PY'
import json, os
d = json.load(open(os.environ['OUT'] + '/bench.json'))
print("graph", d.get("graph_replay")); print("ms/step", d["ms_per_step"], "value", d["value"], "native_us", d["native_us_per_step"], "peak MB", d["peak_mem_mb"], "roofline", d["roofline"])
for k,v in d["kernels"].items(): print(f"  {k:40s} {v['avg_us']:8.1f} us x{v['calls_per_step']}  {v['GBps']} GB/s")
PY
timeout -k 10 300 python bench.py --full --config c4 --steps 12 --warmup 4 --no-cpu-baseline > $OUT/bench_c4.json 2> $OUT/bench_c4.err; rc=$?; echo "bench c4 exit $rc"
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then exit $rc; fi
python - <<'PY'
import json, os
try:
    d = json.load(open(os.environ['OUT'] + '/bench_c4.json'))
    print("c4 ms/step", d["ms_per_step"], "value", d["value"], "native_us", d["native_us_per_step"], "peak MB", d["peak_mem_mb"])
    for k,v in d["kernels"].items(): print(f"  {k:40s} {v['avg_us']:8.1f} us x{v['calls_per_step']}  {v['GBps']} GB/s")
except Exception as e: print("c4 parse failed", e)
PY
if [ -z "$FTR_PROFILE" ]; then exit 0; fi
rm -rf $OUT/prof_r1 $OUT/pmc_fetch $OUT/pmc_write
R=$PWD; cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r1 -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-graph > $OUT/prof_bench.json 2> $OUT/prof.err; echo "prof exit $?" >> $OUT/prof.err
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/pmc_fetch.json 2> $OUT/pmc_fetch.err
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/pmc_write.json 2> $OUT/pmc_write.err
rm -rf $OUT/prof_c4
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c4 -- python3 $R/bench.py --full --config c4 --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/prof_bench_c4.json 2> $OUT/prof_c4.err; echo "prof c4 exit $?" >> $OUT/prof_c4.err
cd $R; tail -2 $OUT/prof.err; ls $OUT/pmc_fetch/*/ | head -3
