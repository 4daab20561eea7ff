#!/bin/bash
# round-3 final evidence: kernel stats + PMC passes of both default workloads, then the --full bench line
R=$GRAFT_REPO_ROOT
O=${1:?usage: tools/r3/final.sh <output dir, relative to the repository root>}
mkdir -p $R/$O
bash $R/tools/profile_round.sh $O/prof_r03 g_only > /dev/null 2>&1 || exit 1
echo "g_only profiled"
bash $R/tools/profile_round.sh $O/prof_r03 gan > /dev/null 2>&1 || exit 1
echo "gan profiled"
cd $R && python bench.py --full > $O/r03_default_bench.json 2> $O/r03_default_bench.err || { tail -5 $O/r03_default_bench.err; exit 1; }
tail -c 1500 $O/r03_default_bench.json
