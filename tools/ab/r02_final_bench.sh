cd /root/repo
OUT=${1:?usage: tools/ab/r02_final_bench.sh OUTDIR}
mkdir -p $OUT
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
for c in c1 c3 c4 c5; do
  timeout -k 10 300 python bench.py --config $c --full --steps 5 --warmup 1 --cpu-budget 5 > $OUT/bench_$c.json 2> $OUT/bench_$c.err || echo "bench $c failed"
done
python tools/config_perf.py dropin 2>&1 | grep -v amdgpu.ids > $OUT/dropin.txt
cat $OUT/dropin.txt
head -c 600 $OUT/bench_default.json
