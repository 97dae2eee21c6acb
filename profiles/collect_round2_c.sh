#!/bin/bash
# Runs ON THE GPU BOX (via gpurun), end of round 2 after the launch fusion / SAGE two-step / HIP training head:
#   part A (default):  default workload r02c + stress x 0.3 r02u (stats + PMC), training-step kernel stats, emulate-world lines
#   part B (presets):  PMC summaries of the other presets / kinds
# Usage: bash profiles/collect_round2_c.sh A|B
RESULTS=${RESULTS:-profiles/out}   # where the runs write (git-ignored)
mkdir -p $RESULTS
make -C graph_recsys_benchmark_amd/csrc -j16 -s 2>&1 | grep -E "error"
export TMPDIR=/tmp
one() {  # tag, extra bench flags
  tag=$1; shift
  bash profiles/collect.sh $tag "$@" > $RESULTS/collect_$tag.log 2>&1
  python profiles/summarize.py $RESULTS/prof_$tag $RESULTS/summary_$tag.json > $RESULTS/summary_$tag.txt
  cp $(find $RESULTS/prof_$tag/stats -name "*kernel_stats.csv" | head -n 1) $RESULTS/kernel_stats_$tag.csv
  rm -rf $RESULTS/prof_$tag
}
if [ "${1:-A}" = "A" ]; then
  one r02c
  one r02u --preset stress_10m --scale 0.3
  rocprofv3 --kernel-trace --stats --output-format csv -d $RESULTS/prof_train -- python3 bench.py --full --train-steps 8 --steps 2 --warmup 1 --no-extras --no-cpu-baseline --no-profile > $RESULTS/prof_train.log 2>&1
  cp $(find $RESULTS/prof_train -name "*kernel_stats.csv" | head -n 1) $RESULTS/kernel_stats_train_r02c.csv
  rm -rf $RESULTS/prof_train
  for w in 2 4 8; do python bench.py --full --emulate-world $w --steps 10 --no-extras > $RESULTS/r2c_emu${w}.json 2>/dev/null; done
  python bench.py --full --emulate-world 8 --train-steps 6 --steps 10 --no-extras > $RESULTS/r2c_emu8_train.json 2>/dev/null
  python bench.py --full --train-steps 8 --no-extras --cpu-samples 0 > $RESULTS/r2c_train.json 2>/dev/null
  head -n 8 $RESULTS/summary_r02c.txt
else
  for spec in "ml25m_shaped gcn" "ml25m_shaped sage" "yelp_shaped sage" "yelp_shaped gat" "yelp_shaped gcn" "ml_small gcn" "ml_small gat"; do
    set -- $spec
    one r02c_$1_$2 --preset $1 --kind $2
    python bench.py --full --preset $1 --kind $2 --no-extras --cpu-samples 1 > $RESULTS/r2c_$1_$2.json 2>/dev/null
  done
  ls $RESULTS | grep r02c_ | head -n 30
fi
