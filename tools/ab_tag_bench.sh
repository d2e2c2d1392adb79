#!/bin/bash
# tools/ab_tag_bench.sh BASE_TREE OUT.json.log [PAIRS] -- on the GPU box: the pair-form tagged path of another checkout
# (BASE_TREE: a built tree of the baseline commit, e.g. `git worktree add ../base HEAD~1` and `make` in its csrc) against
# this tree, like for like.  Every process runs ITS OWN tree's tool and library with the same arguments:
#   1. tools/tag_bench.py --rounds 15, no --ranges: base, this, base, this, ... PAIRS times (default 4), one process each;
#   2. tools/tag_stage_ms.py (this tree's script, --root picks the package): the kernel time per stage of the tag_* settings,
#      stage 2 included, base and this alternated PAIRS times;
#   3. tools/tag_bench.py --ranges --rounds 15 of this tree, in a run of its own (the between_* settings).
# Every JSON line goes to OUT stamped with "build" (base / this / this_ranges) and "process" (the pair's number).
# A step that fails ends the script.
set -e -o pipefail
base=$(cd "$1" && pwd); out=$2; pairs=${3:-4}
here=$(cd "$(dirname "$0")/.." && pwd)
: > "$out"
stamp() {  # stamp BUILD PROCESS: JSON lines of stdin, with the two fields in front
  python3 -c '
import json, sys
for l in sys.stdin:
    if l.startswith("{"):
        d = json.loads(l); d.pop("build", None)
        print(json.dumps(dict(build=sys.argv[1], process=int(sys.argv[2]), **d)))' "$1" "$2"
}
for p in $(seq 1 "$pairs"); do
  (cd "$base" && timeout -k 10 200 python3 tools/tag_bench.py --rounds 15) | stamp base "$p" >> "$out"
  (cd "$here" && timeout -k 10 200 python3 tools/tag_bench.py --rounds 15) | stamp this "$p" >> "$out"
done
for p in $(seq 1 "$pairs"); do
  (cd "$here" && timeout -k 10 200 python3 tools/tag_stage_ms.py --root "$base") | stamp base "$p" >> "$out"
  (cd "$here" && timeout -k 10 200 python3 tools/tag_stage_ms.py --root "$here") | stamp this "$p" >> "$out"
done
(cd "$here" && timeout -k 10 200 python3 tools/tag_bench.py --ranges --rounds 15) | stamp this_ranges 1 >> "$out"
echo "wrote $out"
