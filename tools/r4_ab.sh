#!/bin/bash
# same-box A/B of an environment knob: bench line (twice, interleaved) + one step's kernel trace per setting
# usage: tools/r4_ab.sh TAG VAR VAL_A VAL_B     (values beginning with "@" are paths relative to the repository root)
set -e
tag=$1; var=$2
root=${GRAFT_REPO_ROOT:-/root/repo}
va=${3/#@/$root/}; vb=${4/#@/$root/}
out=$root/gpurun_out/$tag
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
for l in a b a b; do
  if [ $l = a ]; then export $var=$va; else export $var=$vb; fi
  python3 $root/bench.py --full --no-cpu-baseline --no-kernel-timing --sustained 100 > $out/bench_$l.json 2> $out/bench_$l.err || { tail -5 $out/bench_$l.err; exit 1; }
  python3 - <<PY
import json
d=json.load(open("$out/bench_$l.json"))
print("$l", "img/s", d["value"], "ms/step", d["ms_per_step"], "fwd ms", d["forward"]["ms"], "sustained", d.get("sustained",{}).get("ms_per_step"))
PY
done
for l in a b; do
  if [ $l = a ]; then export $var=$va; else export $var=$vb; fi
  rocprofv3 --kernel-trace --output-format csv -d $out/trace_$l -o p -- python3 $root/bench.py --no-cpu-baseline --no-forward --no-kernel-timing --sustained 0 --steps 6 --warmup 2 > /dev/null 2> $out/trace_$l.err
  cp $(ls $out/trace_$l/*kernel_trace.csv $out/trace_$l/*/*kernel_trace.csv 2>/dev/null | head -1) $out/trace_$l.csv
  rm -rf $out/trace_$l
done
python3 $root/tools/step_timeline.py $out/trace_a.csv --compare $out/trace_b.csv > $out/timeline.txt
grep -A 30 "per kernel name" $out/timeline.txt
