make -C graph_recsys_benchmark_amd/csrc -j16 -s 2>&1 | grep -E "error"
RESULTS=${RESULTS:-profiles/out}   # where the runs write (git-ignored)
mkdir -p $RESULTS
bash profiles/collect.sh r02b > $RESULTS/collect_r02b.log 2>&1
python profiles/summarize.py $RESULTS/prof_r02b $RESULTS/summary_r02b.json > $RESULTS/summary_r02b.txt
cp $(find $RESULTS/prof_r02b/stats -name "*kernel_stats.csv" | head -1) $RESULTS/kernel_stats_r02b.csv
rm -rf $RESULTS/prof_r02b
bash profiles/collect.sh r02t --preset stress_10m --scale 0.3 > $RESULTS/collect_r02t.log 2>&1
python profiles/summarize.py $RESULTS/prof_r02t $RESULTS/summary_r02t.json > $RESULTS/summary_r02t.txt
cp $(find $RESULTS/prof_r02t/stats -name "*kernel_stats.csv" | head -1) $RESULTS/kernel_stats_r02t.csv
rm -rf $RESULTS/prof_r02t
for w in 2 4 8; do python bench.py --full --emulate-world $w --steps 10 > $RESULTS/r2_emu${w}_f2.json 2>/dev/null; done
python bench.py --full --emulate-world 8 --train-steps 6 --steps 10 > $RESULTS/r2_emu8_train_f2.json 2>/dev/null
python bench.py --full --train-steps 8 --no-extras --no-cpu-baseline > $RESULTS/r2_train_f2.json 2>/dev/null
for k in gcn sage; do python bench.py --full --kind $k --no-extras --cpu-samples 1 > $RESULTS/r2_ml25m_${k}_f2.json 2>/dev/null; done
python bench.py --full --preset yelp_shaped --kind sage --no-extras --cpu-samples 1 > $RESULTS/r2_yelp_sage_f2.json 2>/dev/null
head -6 $RESULTS/summary_r02b.txt
