#!/bin/bash
# What the eight hot exp-table reads per lane-timestep of the headline kernel (wg256x4s) cost the LDS: two builds of libpfgrad --
# production and -DPFG_EXP_TABLANE (every hot exp reads table entry tid & 127: conflict-free, the real index kept alive; NOT a
# valid sampler) -- one PMC pass each over bench.py's c2 launch (12288 chains) + the HIP-event kernel time of the same run.
# Builds first:  python -m sgmcmc_ssm_amd._build tablane -DPFG_EXP_TABLANE=1
# usage (on the GPU): tools/lds_table_split.sh [output directory]   -> <output directory>/summary.txt
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-${TMPDIR:-/tmp}/r08_lds_table_split}
C=$ROOT/stochastic-gradient-mcmc-for-non-linear-state-models---mth422_amd/csrc
mkdir -p $OUT; rm -rf $OUT/prod $OUT/tablane
export TMPDIR=/tmp PFG_BENCH_KNOCKOUT=1
ARGS="--config c2 --steps 4 --warmup 1 --no-cpu-baseline --no-single-chain"
for tag in prod tablane; do
  LIB=$C/libpfgrad_$tag.so; [ $tag = prod ] && LIB=$C/libpfgrad.so
  PFGRAD_LIB=$LIB timeout -k 10 200 rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_WAIT_INST_LDS SQ_BUSY_CYCLES GRBM_GUI_ACTIVE \
      --output-format csv -d $OUT/$tag -o pmc -- python3 $ROOT/bench.py $ARGS > $OUT/$tag.json 2> $OUT/$tag.err || { echo "$tag: pass failed"; exit 1; }
done
python3 - $OUT <<'PY' | tee $OUT/summary.txt
import collections, csv, glob, json, sys
out = {}
for tag in ("prod", "tablane"):
    acc = collections.defaultdict(list)
    for f in glob.glob("%s/%s/**/*counter_collection.csv" % (sys.argv[1], tag), recursive=True):
        for r in csv.DictReader(open(f)):
            if "pf_reg_kernel" in r["Kernel_Name"]:
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    line = json.loads([l for l in open("%s/%s.json" % (sys.argv[1], tag)) if l.startswith("{")][-1])
    out[tag] = dict(kernel_ms=line["roofline"]["kernel_ms"], **{k: sum(v) / len(v) for k, v in acc.items()})
print(json.dumps(out, indent=1))
p, k = out["prod"], out["tablane"]
for c in ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"):
    print("%s per launch: production %.3e | conflict-free table reads %.3e => the table reads' share %.1f %%" % (c, p[c], k[c], 100 * (p[c] - k[c]) / p[c]))
print("kernel ms: production %.2f, conflict-free table reads %.2f (%+.1f %%)" % (p["kernel_ms"], k["kernel_ms"], 100 * (k["kernel_ms"] / p["kernel_ms"] - 1)))
PY
