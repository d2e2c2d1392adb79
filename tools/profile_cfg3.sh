#!/bin/bash
# tools/profile_cfg3.sh OUT.md -- on the GPU box: the three rocprofv3 passes behind profiles/*_rocprof_summary.md and
# profiles/traffic.json for the default bench workload (kernel trace; FETCH_SIZE; WRITE_SIZE -- counters in their own
# runs, never combined with a trace), condensed by tools/summarize_profile.py.  The program comes directly after `--`.
# The raw passes go to a scratch folder beside OUT.md (removed at the end); the bench line of the traced run to
# OUT_bench.json.
set -e
out=${1:?usage: tools/profile_cfg3.sh OUT.md}
w=$(dirname "$out")
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
args="bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-host-api --no-overlap-extra"
rm -rf $w/prof_kt $w/prof_f $w/prof_w
rocprofv3 --kernel-trace --stats --output-format csv -d $w/prof_kt -- python3 $args > $w/prof_kt.log 2>&1
echo "kernel trace done"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $w/prof_f -- python3 $args > $w/prof_f.log 2>&1
echo "FETCH_SIZE done"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $w/prof_w -- python3 $args > $w/prof_w.log 2>&1
echo "WRITE_SIZE done"
python3 tools/summarize_profile.py $(find $w/prof_kt -name "*kernel_trace.csv") $(find $w/prof_f -name "*counter_collection.csv") \
   $(find $w/prof_w -name "*counter_collection.csv") 2560000 $out "round 3: $args (cfg3 N=10M d=128 k=10 Q=10k f32, reference-stream data), MI355X"
grep "^{" $w/prof_kt.log > "${out%.md}_bench.json"
rm -rf $w/prof_kt $w/prof_f $w/prof_w
