#!/bin/bash
# Collects the round's evidence on an MI355X: OUT_DIR=<dir> tools/profile_round.sh <tag>   (e.g. r01_v4)
#   $OUT_DIR/<tag>_bench.json                 full bench line (--full)
#   $OUT_DIR/<tag>_stats_serial/              rocprofv3 --kernel-trace --stats, LUPIN_LANES=1 (kernels one at a time: the
#                                             average durations the bench's hipEvent pass must agree with)
#   $OUT_DIR/<tag>_stats_overlap/             the same with the default 3 lanes
#   $OUT_DIR/<tag>_pmc.json                   folded PMC passes (tools/pmc_passes.sh)
set -e
TAG=$1
: "${OUT_DIR:?set OUT_DIR to the output directory (relative to the repository root, or absolute)}"
export OUT_DIR TMPDIR=/tmp
cd "$(dirname "$0")/.." && mkdir -p "$OUT_DIR"
python3 bench.py --full > $OUT_DIR/${TAG}_bench.json 2> $OUT_DIR/${TAG}_bench.err
LUPIN_LANES=1 python3 bench.py --full --no-cpu-baseline > $OUT_DIR/${TAG}_bench_serial.json 2>> $OUT_DIR/${TAG}_bench.err
export LUPIN_LANES=1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/${TAG}_stats_serial -- python3 bench.py --steps 8 --warmup 2 --full --no-cpu-baseline > $OUT_DIR/${TAG}_stats_serial.log 2>&1
unset LUPIN_LANES
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/${TAG}_stats_overlap -- python3 bench.py --steps 8 --warmup 2 --full --no-cpu-baseline > $OUT_DIR/${TAG}_stats_overlap.log 2>&1
tools/pmc_passes.sh ${TAG}_pmc python3 bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-kernel-timing
UNITS=$(grep -h '^{"metric"' $OUT_DIR/${TAG}_pmc1.log | tail -1 | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['path_bounces']*1.5)")
python3 tools/pmc_summary.py $UNITS $OUT_DIR/${TAG}_pmc.json $OUT_DIR/${TAG}_pmc1 $OUT_DIR/${TAG}_pmc2 $OUT_DIR/${TAG}_pmc3 $OUT_DIR/${TAG}_pmc4 $OUT_DIR/${TAG}_pmc5 > $OUT_DIR/${TAG}_pmc_derived.json
cp $OUT_DIR/${TAG}_stats_serial/*/*kernel_stats.csv $OUT_DIR/${TAG}_kernel_stats_serial.csv
cp $OUT_DIR/${TAG}_stats_overlap/*/*kernel_stats.csv $OUT_DIR/${TAG}_kernel_stats_overlap.csv
cat $OUT_DIR/${TAG}_bench.json
