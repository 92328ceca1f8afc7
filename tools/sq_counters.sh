#!/bin/bash
# SQ instruction / wait counters of the fused and the end-of-tick kernel for one library build and workload (PMC passes, counters only).
#   tools/sq_counters.sh <lib.so> <workload> <outdir>
# SQ_PASSES: the counter sets, one pass each, separated by ';' (default: the three sets below).  SQ_BENCH_ARGS: bench.py's arguments
# (default: the --full run of 40 steps), e.g. "--profile-run --workload config3 --steps 60 --warmup 10".
set -o pipefail
LIB=$(realpath $1); W=$2; OUT=$3; mkdir -p $OUT
export TMPDIR=/tmp SC_TICK_LIB=$LIB SC_TICK_LAX_BIND=1
PASSES=${SQ_PASSES:-"SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES;SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_BUSY_CYCLES SQ_INSTS_SMEM;SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQ_IFETCH"}
BENCH=${SQ_BENCH_ARGS:-"--full --workload $W --steps 40 --warmup 10 --no-cpu-baseline --no-parity"}
IFS=';' read -ra SETS <<< "$PASSES"
P=0
for C in "${SETS[@]}"; do
  P=$((P+1))
  timeout -k 10 300 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pass$P -o sq -- python3 bench.py $BENCH > $OUT/pass$P.log 2>&1 || { tail -5 $OUT/pass$P.log; exit 1; }
done
python3 - $OUT <<'PY'
import csv, glob, json, os, sys
from collections import defaultdict
out = sys.argv[1]
acc = defaultdict(lambda: defaultdict(list))
for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        for k in ("k_xform_cull", "k_compact_pairs"):
            if k in r["Kernel_Name"]:
                acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
res = {k: {c: round(sum(v[len(v)//4:]) / len(v[len(v)//4:])) for c, v in sorted(cs.items())} for k, cs in acc.items()}
json.dump(res, open(os.path.join(out, "sq.json"), "w"), indent=1)
print(json.dumps(res))
PY
