# A/B on one box, alternated: bench.py with every tensor bf16 against bf16 + fp16 pyramid (the decision of DESIGN 4.4: throughput and epe_vs_reference of both)
export D=${OUT:-$(mktemp -d)}
for i in 1 2; do
python bench.py --full --no-cpu-baseline --no-train-probe --no-literal-split > $D/ab_pyr_bf16_$i.json 2>/dev/null
python bench.py --full --no-cpu-baseline --no-train-probe --no-literal-split --pyramid-dtype fp16 > $D/ab_pyr_fp16_$i.json 2>/dev/null
done
python - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.path.join(os.environ['D'], 'ab_pyr_*.json'))):
    d=json.loads(open(f).read().strip().splitlines()[-1])
    print(f, d['value'], d['value_min'], d['value_max'], d['one_step_in_flight']['ms_per_step'], d.get('epe_vs_reference'))
PY
