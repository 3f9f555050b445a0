#!/bin/bash
# one GPU visit = one box, one library: the driver's GPU suite RUNS times in a row (default 5), smoke(), the driver's bench command with --full on the library at HEAD
# (-> $OUT/bench_<tag>_driver.json), then the round's bench + profile passes (tools/profile_round.sh) unless the second argument is noprofile
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
export TMPDIR=/tmp
export OUT=$(realpath -m "${OUT:-out}")                 # output directory (default: out/ of the repository)
mkdir -p "$OUT"
tag=${1:-r05a}
: > $OUT/suite_loop_$tag.log
for i in $(seq 1 ${RUNS:-5}); do
  echo "=== run $i ===" >> $OUT/suite_loop_$tag.log
  timeout 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/suite_run_${tag}_$i.log 2>&1
  echo "rc=$?" >> $OUT/suite_loop_$tag.log
  grep -E "passed|failed|error" $OUT/suite_run_${tag}_$i.log | tail -3 >> $OUT/suite_loop_$tag.log
done
cat $OUT/suite_loop_$tag.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$tag.log 2>&1; echo "smoke rc=$?"; tail -2 $OUT/smoke_$tag.log
timeout 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_${tag}_driver.json 2> $OUT/bench_${tag}_driver.err; echo "driver bench rc=$?"
python - "$tag" <<'PY'
import json, os, sys
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_%s_driver.json" % sys.argv[1])).read().strip().splitlines()[-1])
print("driver cmd: %.1f frames/s  %.4f ms/step; library %s" % (d["value"], d["ms_per_step"], d["config"]["library"]))
print("box:", {k: v for k, v in (d.get("box") or {}).items() if k != "how"})
r = d["roofline"]; print("roofline:", r["kernel"][:50], "in-step ms", round(r["avg_launch_ms"], 4), "frac", round(r["frac"], 3), "of box", round(r.get("frac_of_box", 0), 3))
print("in-step candidates:", d.get("per_op_in_step_ms"))
for k in ("bf16x3", "fp32", "mlp_vae", "ppo"):
    print(k, {kk: vv for kk, vv in (d.get(k) or {}).items() if kk in ("frames_per_s", "ms_per_step", "ms_per_update", "error")})
PY
[ "$2" = "noprofile" ] || tools/profile_round.sh $tag
