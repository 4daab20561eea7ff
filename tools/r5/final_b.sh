#!/bin/bash
# round-5 evidence, part B: kernel stats + PMC passes of both default workloads, layer tables, the --full bench line
R=$GRAFT_REPO_ROOT
O=${1:?usage: tools/r5/final_b.sh <output dir, relative to the repository root>}
mkdir -p $R/$O
bash $R/tools/profile_round.sh $O/prof_r05 g_only > /dev/null 2>&1 || exit 1
echo "g_only profiled"
bash $R/tools/profile_round.sh $O/prof_r05 gan > /dev/null 2>&1 || exit 1
echo "gan profiled"
cd $R
python tools/layer_table.py --workload gan > $O/r05_layer_table_gan.txt 2>/dev/null
python tools/layer_table.py --workload g_only > $O/r05_layer_table_g_only.txt 2>/dev/null
python bench.py --full > $O/r05_default_bench.json 2> $O/r05_default_bench.err || { tail -5 $O/r05_default_bench.err; exit 1; }
tail -c 1500 $O/r05_default_bench.json
