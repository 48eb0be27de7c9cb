#!/bin/bash
# GPU box: final collection of the round, all from ONE box and call (boxes of the pool differ by several %):
#   bench line; bench under rocprofv3 --kernel-trace --stats + PMC of the eval forward (profile_mlp.sh); B=32 training kernel
#   stats; training PMC (pmc_train.sh); HBM-bound kernels: stats + PMC (pmc_hbm.sh); launch histogram + ordered launches of a
#   replayed B=4 GAN iteration; training lines; C5 multi-object line.          Usage: tools/collect_round.sh [tag]  (writes runs/<tag>/)
T=${1:-r5}
O=runs/$T
mkdir -p $O
export TMPDIR=/tmp
( time timeout 1500 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err ) 2> $O/bench_wall.txt
bash tools/profile_mlp.sh $T > $O/profile_mlp.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/train32 -o t -- python3 tools/train_bench.py 32 0 30 0 f16x3 > $O/train32.log 2>&1
cp $(find $O/train32 -name '*kernel_stats.csv' | head -1) $O/train32_kernel_stats.csv
bash tools/pmc_train.sh $T > $O/pmc_train.log 2>&1
bash tools/pmc_hbm.sh $T > $O/pmc_hbm.log 2>&1
rocprofv3 --kernel-trace --output-format csv -d $O/gan4 -o t -- python3 tools/train_bench.py 4 1 12 1 f16x3 > $O/gan4.log 2>&1
python3 tools/launch_histogram.py $O/gan4 > $O/launch_histogram.txt 2>&1
python3 tools/launch_sequence.py $O/gan4 > $O/launch_sequence.txt 2>&1
for i in 1 2; do python3 tools/train_bench.py 4 1 200 1 f16x3 2>&1 | tail -1; python3 tools/train_bench.py 4 0 200 1 f16x3 2>&1 | tail -1; python3 tools/train_bench.py 32 0 60 1 f16x3 2>&1 | tail -1; done > $O/train_lines.txt
timeout 600 python bench.py --config c5 > $O/c5.json 2> $O/c5.err
# the GAN loop with one change switched off at a time (same box, alternating with the product configuration)
( for e in TP_X=1 TP_NO_FEAT_CHAIN=1 TP_X=1 TP_NO_DISC_PAIRS=1 TP_X=1 TP_NO_SN_SETS=1 TP_X=1 "TP_NO_FEAT_CHAIN=1 TP_NO_DISC_PAIRS=1 TP_NO_SN_SETS=1" TP_X=1 TP_LINEAR_GRAPHS=0 TP_X=1 TP_FOUR_GRAPHS=0 TP_X=1 TP_PRE_STREAMS=2 "TP_PRE_STREAMS=2 TP_NO_QUEUE_PROBE=1" TP_X=1; do
    echo "$e $(env $e python3 tools/train_bench.py 4 1 200 1 f16x3 2>&1 | tail -1 | cut -c1-75)"; done ) > $O/gan_ablations.txt
python3 tools/tail_bench.py 4 > $O/tail_bench.txt 2>&1
python3 tools/host_time.py > $O/host_time.txt 2>&1
python3 tools/linear_timeline.py 50 > $O/linear_timeline.txt 2>&1
python3 tools/chain_probe.py 50 > $O/chain_probe.txt 2>&1
python3 tools/boundary_probe.py 64 > $O/boundary_probe.txt 2>&1
# fabric traffic of the exact-fp32 forward (profiles/traffic.json: fp32)
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --kernel-include-regex mlp_fwd --output-format csv -d $O/fp32_$c -- python3 tools/render_once.py fp32 2 > $O/fp32_$c.log 2>&1
  cp $(find $O/fp32_$c -name '*counter_collection.csv' | head -1) $O/fp32_${c}_counter_collection.csv; rm -rf $O/fp32_$c
done
( for k in 0 1 2 3; do python3 tools/queue_probe.py $k 8; done ) > $O/queue_probe.txt 2>&1
# the evaluation render with / without the ray-bias variant of the f16x3 kernel, alternating on this box
( for e in TP_X=1 TP_NO_RAY_BIAS=1 TP_X=1 TP_NO_RAY_BIAS=1; do
    echo "$e $(env $e python3 bench.py --full --no-train --no-cpu-baseline --steps 6 --warmup 2 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], d['roofline']['frac'])")"; done ) > $O/ray_bias_ab.txt 2>&1
python3 tools/kstats.py $O/train32 wgrad dgrad mlp_fwd finalize
rm -rf $O/train32 $O/gan4
cat $O/train_lines.txt | cut -c1-100
cat $O/bench_wall.txt
python3 - <<PY
import json
d=json.load(open("$O/bench_full.json"))
print(d["value"], d["ms_per_step"], d["roofline"]["kernel_ms"], d["roofline"]["frac"], d["roofline"]["traffic"])
t=d["train"]; print(t["full_gan_loop"]["value"], t["nerf_step_b4"]["value"], t["nerf_step_b32"]["value"], t["roofline"])
PY
