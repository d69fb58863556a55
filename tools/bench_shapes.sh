# usage (GPU box, repo root): tools/bench_shapes.sh <output dir> -- bench.py --full on the K1 / NS / SY shapes and with RotKITTI-range
# rotations; <output dir>/shape_<c>.json / .log per shape, and one summary line each
OUT=${1:?usage: tools/bench_shapes.sh <output dir>}
mkdir -p "$OUT"
for c in K1 NS SY; do
  timeout 600 python bench.py --full --config $c --no-cpu-baseline --e2e-pairs 8 --e2e-hard-pairs 4 --detail "$OUT/shape_$c.json" > "$OUT/shape_$c.log" 2>&1; echo "rc $? $c"
done
timeout 600 python bench.py --full --kind rot --no-cpu-baseline --e2e-pairs 8 --e2e-hard-pairs 4 --detail "$OUT/shape_rot.json" > "$OUT/shape_rot.log" 2>&1; echo "rc $? rot"
python - "$OUT" <<'PY'
import json
import os
import sys
for c in ("K1","NS","SY","rot"):
    f = os.path.join(sys.argv[1], f"shape_{c}.json")
    if not os.path.exists(f): print(c,"NO RESULT"); continue
    d=json.load(open(f))
    e=d.get("end_to_end",{}); h=d.get("end_to_end_hard",{})
    print(c, d["value"], d["config"]["workload"][:60], "e2e", e.get("pairs_per_s"), e.get("rr_1.5deg_0.6m"), e.get("rr_1deg_0.1m"), "hard", h.get("pairs_per_s"), h.get("rr_1.5deg_0.6m"))
PY
