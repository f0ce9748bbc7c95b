#!/bin/bash
# The round-5 profile set in one go (run on the GPU box; results land in gpurun_out/profiles/r05_*).
R=$(pwd); export TMPDIR=/tmp; export ROUND=r05
P=$R/gpurun_out/profiles; mkdir -p $P
# 1. the default bench command, un-profiled (the driver's form) and under rocprofv3 (kernel trace + stats)
python bench.py --full > $P/r05_bench_config2_default.json 2> /dev/null
rm -rf $R/gpurun_out/prof_bench; mkdir -p $R/gpurun_out/prof_bench
(cd $TMPDIR && rocprofv3 --kernel-trace --stats --output-format csv -d $P/../prof_bench -- python $R/bench.py --full --no-cpu-baseline > $P/../prof_bench/bench.log 2>&1)
python - <<PY
import csv, glob
f = glob.glob('$R/gpurun_out/prof_bench/*/*kernel_stats.csv')[0]
rows = list(csv.DictReader(open(f)))
out = open('$P/r05_bench_default_rocprof_stats.txt', 'w')
out.write('# rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --full --no-cpu-baseline   (MI355X; config 2, hipGraph replay with 4 steps in flight on 4 HIP streams, 10 warm-up + 3 windows of 50 timed steps + 50 steps one at a time,\n# then the roofline probes: 220 + 30 launches of the cost volume at [8,32,96,320], 55 of the 565->128 convolution, the literal-split and training probes)\n')
out.write('# bench line of this run: ' + [l for l in open('$R/gpurun_out/prof_bench/bench.log').read().split('\\n') if l.startswith('{')][-1] + '\\n')
out.write('%-150s %8s %14s %12s %8s\\n' % ('kernel', 'calls', 'total_ns', 'avg_ns', 'pct'))
for r in rows[:45]:
    out.write('%-150s %8s %14s %12s %8s\\n' % (r['Name'][:150], r['Calls'], r['TotalDurationNs'], r['AverageNs'].split('.')[0], r['Percentage']))
PY
# 2. one steady-state forward, eager (per-kernel tables): config 2 and the native KITTI frame
bash tools/eager_profile_any.sh config2_b4 > /dev/null 2>&1
bash tools/eager_profile_any.sh kitti_native_b4 --workload kitti_native > /dev/null 2>&1
# 3. KITTI-native frames: batch 4 (4 steps in flight + one) with the batch-1 evaluation probe; batch 1 by itself (one step in flight: graph / eager)
python bench.py --full --workload kitti_native --no-cpu-baseline --no-train-probe --no-literal-split 2>/dev/null | tail -1 > $P/r05_bench_kitti_native.json
(python bench.py --full --workload kitti_native --batch 1 --streams 1 --no-cpu-baseline --no-train-probe --no-literal-split --no-eval-probe 2>/dev/null | tail -1; python bench.py --full --workload kitti_native --batch 1 --streams 1 --no-graph --no-cpu-baseline --no-train-probe --no-literal-split --no-eval-probe 2>/dev/null | tail -1) > $P/r05_bench_kitti_native_b1.json
# 4. cost volume: rocprof + PMC of the normalising, octet-writing variant (the kernel inside the step) at the 1/4-resolution level of config 2, config 5 and the native KITTI frame (row-pitched features, PADW kernel)
tools/prof_corr_run.sh 8 32 96 320 bf16 normc8_l4_cfg2_stacked_bf16 norm_c8 r05 > /dev/null 2>&1
tools/prof_corr_run.sh 8 32 94 311 bf16 normc8_l4_kitti_stacked_bf16 norm_c8 r05 > /dev/null 2>&1
tools/prof_corr_run.sh 2 32 240 720 bf16 normc8_l4_cfg5_stacked_bf16 norm_c8 r05 > /dev/null 2>&1
rm -rf $R/gpurun_out/prof_normc8_*
# 5. training step
tools/train_profile.sh train_bf16 --no-graph > /dev/null 2>&1
python bench.py --mode train > $P/r05_train_bf16_bench.json 2>/dev/null
# 6. precision options and the other workloads
python bench.py --full --pyramid-dtype fp16 --no-cpu-baseline --no-train-probe 2>/dev/null | tail -1 > $P/r05_bench_config2_pyramid_fp16.json
python bench.py --full --dtype fp16 --no-cpu-baseline --no-train-probe 2>/dev/null | tail -1 > $P/r05_bench_config2_fp16.json
for wl in config4 config5; do python bench.py --full --workload $wl --no-cpu-baseline --no-train-probe 2>/dev/null | tail -1 > $P/r05_bench_$wl.json; done
# 7. every other operator at the level shapes
python tools/kbench.py > $P/r05_kbench.txt 2>&1
rm -rf $R/gpurun_out/prof_bench/*/ $R/gpurun_out/prof_eager*/*/ $R/gpurun_out/prof_train_bf16/trace
du -sh $R/gpurun_out
ls -la $P
