#!/bin/bash
# Round profile collection on the GPU box (everything lands under OUT_DIR, copy what is judged into profiles/):
#   bench JSON lines (train bf16 default, eval bf16, eval f32, config #4), per-layer timing dumps, rocprofv3 kernel traces
#   + stats (CSV) of the train and eval steps.  PMC traffic: tools/pmc_traffic.py (separate passes).
# usage: tools/prof_train.sh OUT_DIR   (relative to the repository root)
O=${1:?usage: tools/prof_train.sh OUT_DIR}
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
export TMPDIR=/tmp
mkdir -p $O
python bench.py --full --steps 20 --warmup 5 > $O/bench_train_bf16.json 2> $O/bench_train.err
python bench.py --full --mode eval --steps 20 --warmup 5 > $O/bench_bf16.json 2> $O/bench_bf16.err
python bench.py --full --mode eval --dtype f32 --steps 10 --warmup 3 > $O/bench_f32.json 2> /dev/null
python bench.py --full --config c4 --batch 8 --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_c4.json 2> /dev/null
CAVP_BENCH_PER_LAYER=$O/layers_train_bf16.txt python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-f32 > /dev/null 2>&1
CAVP_BENCH_PER_LAYER=$O/layers_bf16.txt python bench.py --full --mode eval --steps 2 --warmup 1 --no-cpu-baseline --no-f32 > /dev/null 2>&1
CAVP_BENCH_PER_LAYER=$O/layers_f32.txt python bench.py --full --mode eval --dtype f32 --steps 2 --warmup 1 --no-cpu-baseline --no-f32 > /dev/null 2>&1
for m in train eval; do
  rm -rf $O/prof_$m
  (cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_$m -o $m -- \
     python $R/bench.py --mode $m --steps 10 --warmup 3 --no-cpu-baseline --no-roofline --no-f32 > $R/$O/prof_$m.log 2>&1)
done
rm -rf $O/prof_eval_f32
(cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_eval_f32 -o evalf32 -- \
   python $R/bench.py --mode eval --dtype f32 --steps 10 --warmup 3 --no-cpu-baseline --no-roofline --no-f32 > /dev/null 2>&1)
ls -R $O/prof_train | head
