#!/bin/bash
# the whole -m gpu suite, smoke(), then the --full bench line (every leg): bash scripts/r4/full.sh OUTPUT_DIR
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${1:?output directory}; mkdir -p $O
timeout 2400 python -m pytest tests -m gpu -q --maxfail=15 --durations=15 > $O/pytest_gpu_full.log 2>&1
tail -30 $O/pytest_gpu_full.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -3
( time timeout 900 python bench.py --full ) > $O/bench_default.json 2> $O/bench_default.err
tail -5 $O/bench_default.err
python3 - "$O/bench_default.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k:d[k] for k in ('metric','value','ms_per_step','n_gpus')}, d.get('roofline',{}).get('frac'))
print('parity', d.get('parity'))
for k,v in d.get('legs',{}).items():
    print(k, v.get('value'), v.get('value_median'), v.get('roofline',{}).get('frac'), v.get('from_x0',{}).get('value') if isinstance(v.get('from_x0'),dict) else None)
PY
