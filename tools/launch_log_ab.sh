#!/bin/bash
# tools/launch_log_ab.sh PARENT_LIB [OUT_DIR] -- does a change to the executor's host code launch exactly what its parent launched?  Runs each GPU test file below once per
# library (MI355X_LIB) with MI355X_LAUNCH_LOG (one line per launching node of every eager submission: node, op, launches, fused count, shapes; no addresses), one process and
# one log per file, plus the reference's Token2Wav window graph the way tools/t2w_slices.sh takes it, and compares the pairs byte for byte.  Tests that start a child process
# are left out (the child loads the tree's own library and would reopen the log): they are listed in the report.  Without PARENT_LIB the parent commit is built in a
# git worktree first.  The report goes to OUT_DIR/launch_log_ab.txt (default: /tmp/launch_log_ab).
set -u
cd "$(dirname "$0")/.."
NEW=$PWD/llama.cpp-omni_amd/lib/libggml-mi355x.so
OLD=${1:-}
OUT=${2:-/tmp/launch_log_ab}
mkdir -p "$OUT"
if [ -z "$OLD" ]; then
    WT=$(mktemp -d) && git worktree add --detach "$WT" HEAD~1 > /dev/null && make -C "$WT/llama.cpp-omni_amd/csrc" -j16 > "$OUT/parent_build.log" 2>&1 || { echo "parent build failed"; exit 1; }
    OLD=$WT/llama.cpp-omni_amd/lib/libggml-mi355x.so
fi
FILES="test_exec_state_gpu test_gpu_parity test_t2w_gpu test_round2_gpu test_round3_gpu test_round4_gpu test_round5_gpu test_round6_gpu test_prefill_kernels_gpu test_iq4_gpu test_fattn_plan_gpu"
REP=$OUT/launch_log_ab.txt
echo "launch logs, parent library vs this tree (lines parent / lines new / verdict)" > "$REP"
# the tests of a module that reach `subprocess` -- directly, through a helper or through a fixture
spawning() { python3 - "$1" <<'PY'
import ast, sys
tree = ast.parse(open(sys.argv[1]).read())
fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
def names(f): return {x.id for x in ast.walk(f) if isinstance(x, ast.Name)} | {a.arg for a in f.args.args}
bad = {k for k, f in fns.items() if "subprocess" in names(f)}
while True:
    more = {k for k, f in fns.items() if k not in bad and names(f) & bad}
    if not more: break
    bad |= more
print(" ".join(sorted(k for k in bad if k.startswith("test_"))))
PY
}
fail=0
for f in $FILES; do
    skip=$(spawning tests/$f.py); desel=""
    for t in $skip; do desel="$desel --deselect tests/$f.py::$t"; done
    for side in parent new; do
        lib=$OLD; [ $side = new ] && lib=$NEW
        MI355X_LIB=$lib MI355X_LAUNCH_LOG=$OUT/$f.$side.log timeout -k 10 900 python -m pytest tests/$f.py -m gpu -q -x -p no:cacheprovider $desel > "$OUT/$f.$side.out" 2>&1
        rc=$?
        if [ $rc -ne 0 ]; then echo "$f ($side): pytest exit $rc -- stopping" | tee -a "$REP"; tail -5 "$OUT/$f.$side.out"; exit 1; fi
    done
    if cmp -s "$OUT/$f.parent.log" "$OUT/$f.new.log"; then v=identical; else v=DIFFERENT; fail=1; diff "$OUT/$f.parent.log" "$OUT/$f.new.log" | head -20 > "$OUT/$f.diff"; fi
    echo "$f $(wc -l < "$OUT/$f.parent.log") $(wc -l < "$OUT/$f.new.log") $v   ($(tail -1 "$OUT/$f.new.out"))${skip:+   left out: $skip}" | tee -a "$REP"
done
if [ -x oracle/_ref/t2w-min ]; then
    python tools/make_synth_omni_gguf.py --module t2w -o "$OUT/t2w" > /dev/null || exit 1
    for side in parent new; do
        lib=$OLD; [ $side = new ] && lib=$NEW
        GGML_BACKEND_PATH=$lib MI355X_GRAPHS=0 MI355X_LAUNCH_LOG=$OUT/t2w_min.$side.log timeout -k 10 600 oracle/_ref/t2w-min "$OUT/t2w" "$OUT/t2w.$side.f32" gpu --windows 2 > /dev/null 2>&1 || { echo "t2w-min ($side) failed -- stopping" | tee -a "$REP"; exit 1; }
    done
    if cmp -s "$OUT/t2w_min.parent.log" "$OUT/t2w_min.new.log"; then v=identical; else v=DIFFERENT; fail=1; fi
    o=different; cmp -s "$OUT/t2w.parent.f32" "$OUT/t2w.new.f32" && o=identical
    echo "t2w-min_windows2 $(wc -l < "$OUT/t2w_min.parent.log") $(wc -l < "$OUT/t2w_min.new.log") $v   (output samples: $o)" | tee -a "$REP"
else
    echo "t2w-min_windows2: oracle/_ref/t2w-min not built -- not compared" | tee -a "$REP"
fi
exit $fail
