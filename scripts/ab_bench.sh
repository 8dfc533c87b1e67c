#!/bin/bash
# A/B of engine knobs on the default bench (config 2), one bench process per setting:
#   [OUT=dir] bash scripts/ab_bench.sh "TAG1 VAR=VAL ..." "TAG2 VAR=VAL ..." ...
set -u
OUT=${OUT:-bench_out/ab}
mkdir -p $OUT
for spec in "$@"; do
  set -- $spec; tag=$1; shift
  env "$@" timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 5 --warmup 2 > $OUT/$tag.log 2>&1 \
    || { echo "$tag failed"; tail -5 $OUT/$tag.log; exit 1; }
  python -c "import json; d=json.loads([l for l in open('$OUT/$tag.log') if l.startswith('{')][-1]); print('$tag', d['ms_per_step'], d['value'], d['roofline']['achieved'])"
done
