#!/bin/bash
# rocprofv3 kernel summary of the default bench command with --full's kernel timing (no forward sub-record, no CPU baseline, no
# sustained record: exactly 33 training steps of kernels) + the per-family table, written under $PROF_OUT (default prof_out/ in the
# repository).   usage (on the GPU box): tools/prof_step.sh TAG [bench args]
set -e
tag=$1; shift
root=${GRAFT_REPO_ROOT:-/root/repo}
out=${PROF_OUT:-$root/prof_out}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/$tag -o p -- python3 $root/bench.py --full --no-cpu-baseline --no-forward --sustained 0 "$@" > $out/${tag}_bench.json 2> $out/${tag}.err
cd $root
python tools/kernel_categories.py $(ls $out/$tag/*kernel_stats.csv $out/$tag/*/*kernel_stats.csv 2>/dev/null | head -1) 33 > $out/${tag}_cat.txt
cat $out/${tag}_cat.txt
