# developer helper: A/B two builds of the library in ONE GPU call (box-to-box variance is +-3 %).  tools/_ab/libsvhip_A.so vs the in-tree build.
#   bash tools/ab.sh [ecapa|rawnet2]
cd "$(dirname "$0")/.."
OUT=$(mktemp -d)
M=${1:-ecapa}
EXTRA=""
if [ "$M" = "rawnet2" ]; then EXTRA="--model rawnet2 --compute f16"; fi
for rep in 1 2; do
  for v in A B; do
    if [ $v = A ]; then export SVHIP_LIB_PATH=$PWD/tools/_ab/libsvhip_A.so; else unset SVHIP_LIB_PATH; fi
    python bench.py $EXTRA --full --no-cpu-baseline --no-scoring --no-extras --steps 20 --warmup 5 --record-file $OUT/ab_$v.jsonl > $OUT/ab_$v.json 2> $OUT/ab_$v.err
    V=$v OUT=$OUT python - <<'PY'
import json, os
v, out = os.environ["V"], os.environ["OUT"]
d = json.loads(open("%s/ab_%s.json" % (out, v)).read().strip().splitlines()[-1])
kern = [r for r in map(json.loads, open("%s/ab_%s.jsonl" % (out, v))) if r["record"] == "kernels"][0]["kernels"]
print(v, round(d["value"]), round(d["ms_per_step"], 3), "sustained", round(d["sustained"]["value"]), d["check"]["ok"],
      " ".join("%s=%.1f" % (k, x["avg_ms"] * 1e3) for k, x in kern.items() if x["ms_per_step"] > 0.1))
PY
  done
done
