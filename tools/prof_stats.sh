#!/bin/bash
# rocprofv3 --kernel-trace --stats of the full bench command (--full) and of the headline alone (GPU box); raw output under
# prof_out/$1/ (PROF_OUT overrides prof_out), summary written by tools/prof_summarize.py.      tools/prof_stats.sh r03
tag=${1:-r03}
cd /tmp && export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-/root/repo}"
out="${PROF_OUT:-prof_out}/$tag"
mkdir -p $out
rm -rf $out/prof_stats $out/prof_stats_hl
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_stats -- python3 bench.py --full --no-pmc --no-cpu-baseline --steps 5 --warmup 1 --detail-out $out/prof_stats_detail.json > $out/prof_stats.log 2>&1
echo "rc=$?" >> $out/prof_stats.log
f=$(find $out/prof_stats -name "*kernel_stats.csv" | head -1)
cp "$f" $out/bench_default_kernel_stats.csv
head -24 "$f" | cut -c1-200
# the headline alone: every launch of its kernel is then a fixed-50, 1M-frame launch
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_stats_hl -- python3 bench.py --steps 10 --warmup 2 --detail-out $out/prof_stats_hl_detail.json > $out/prof_stats_hl.log 2>&1
echo "rc=$?" >> $out/prof_stats_hl.log
f=$(find $out/prof_stats_hl -name "*kernel_stats.csv" | head -1)
cp "$f" $out/bench_headline_kernel_stats.csv
head -4 "$f" | cut -c1-200
