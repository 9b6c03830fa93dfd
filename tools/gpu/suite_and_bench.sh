cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -4
OUT=${BENCH_OUT_DIR:-$(mktemp -d)}
mkdir -p "$OUT"
timeout -k 10 900 python bench.py --full > "$OUT/default.json" 2> "$OUT/default.err"; echo rc=$? "record: $OUT/default.json"
python - "$OUT/default.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['ms_per_step'], d['value'], d['parity_ok'], d['roofline']['frac'], d['roofline']['lstm_fwd_us'], d['roofline']['lstm_bwd_us'], d['e2e']['ms_per_step'], d['mask_max_abs_err_vs_oracle'], d['mask_err_f32_oracle'])
for k,v in d.get('also',{}).items():
    print(k, v['ms_per_step'], v['value'], v.get('parity_ok'), v['roofline'].get('frac'), v['wall_s'])
PY
