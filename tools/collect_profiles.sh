#!/bin/bash
# Measurement evidence of a round, collected on the GPU box (gpurun): the bench lines, rocprofv3 kernel stats of the bench
# commands (restricted to the timed window where warm-up would be averaged in) and the counter passes of the search kernel.
# Outputs under gpurun_out/prof6/ (the summaries are copied into profiles/ afterwards, named r06_*).
# Every command runs under `timeout`: a hang must not take the box.  Under rocprofv3 the program itself follows `--`.
set -u
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
O=gpurun_out/prof6
rm -rf $O; mkdir -p $O
CLEAN="--sweep-instances 0 --no-tail --no-cpu-baseline --no-secondary"
# gpurun boxes differ: about one in ten runs the search launch 35 % slower than the others (every other kernel the same, four
# times the fabric traffic on its counters).  Such a box is no longer skipped: the set is collected all the same and TAGGED
# (slowbox.txt next to it), so that profiles/ can hold one set of each kind side by side.
KMS=$(timeout 300 python3 bench.py --steps 300 --warmup 150 $CLEAN --profile-steps 0 2>/dev/null | python3 -c "import json,sys; print(json.loads(sys.stdin.read())['roofline']['kernel_ms'])")
echo "probe: search launch $KMS ms" | tee $O/probe.txt
if python3 -c "import sys; sys.exit(0 if float('$KMS') > 0.038 else 1)"; then
  echo "slow-search box: this set is the SLOW kind" | tee $O/slowbox.txt
  { date; rocm-smi --showcomputepartition --showmemorypartition --showclocks --showperflevel --showpower 2>&1; rocminfo 2>&1 | grep -i -E "xnack|Compute Unit|Max Clock|Cacheline|L2|L3|Marketing|Coherent|Memory Properties" | sort | uniq -c; env | grep -E "^(HSA|HIP|ROC|GPU|AMD)" ; } >> $O/slowbox.txt 2>&1
fi
# 0. the bench lines (no profiler)
timeout 900 python3 bench.py --full > $O/bench_default.json 2> $O/bench_default.err
timeout 300 python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-secondary > $O/bench_driver_args.json 2> $O/bench_driver_args.err
timeout 600 python3 bench.py --config kinematic > $O/bench_kinematic.json 2> $O/bench_kinematic.err
timeout 600 python3 bench.py --config nao_recipe > $O/bench_nao_recipe.json 2> $O/bench_nao_recipe.err
timeout 600 python3 bench.py --config nao > $O/bench_nao.json 2> $O/bench_nao.err
# 1. kernel stats of the clean headline command (every launch belongs to the measured instance)
timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $O/stats_clean -- python3 bench.py $CLEAN > $O/bench_clean_under_rocprof.json 2> $O/stats_clean.err
# 2. counter passes of the search kernel (separate runs, --kernel-trace only), eager launches so that every dispatch is visible
for C in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_SALU SQ_INSTS_LDS; do
  timeout 600 rocprofv3 --kernel-trace --pmc $C -f csv -d $O/pmc_$C -- python3 bench.py --steps 300 --warmup 150 --no-graph --profile-steps 0 $CLEAN > $O/pmc_$C.json 2> $O/pmc_$C.err
done
# 3. the kinematic projection and the README recipe: per-dispatch traces, statistics over the TIMED WINDOW only (the last
#    dispatches of every kernel: the cold solve and the warm-up re-solves that precede the timed iterations stay out)
timeout 900 rocprofv3 --kernel-trace -f csv -d $O/trace_kinematic -- python3 bench.py --config kinematic --no-cpu-baseline > $O/bench_kinematic_under_rocprof.json 2> $O/trace_kinematic.err
f=$(find $O/trace_kinematic -name "*kernel_trace.csv" | head -1)
[ -n "$f" ] && python3 tools/kernel_window_stats.py "$f" --last 100 > $O/kernel_stats_kinematic_window.csv
timeout 900 rocprofv3 --kernel-trace -f csv -d $O/trace_recipe -- python3 bench.py --config nao_recipe --no-cpu-baseline > $O/bench_nao_recipe_under_rocprof.json 2> $O/trace_recipe.err
f=$(find $O/trace_recipe -name "*kernel_trace.csv" | head -1)
[ -n "$f" ] && python3 tools/kernel_window_stats.py "$f" --last 1999 --match lap_ > $O/kernel_stats_nao_recipe_window.csv
timeout 900 rocprofv3 --kernel-trace -f csv -d $O/trace_projection -- python3 bench.py --config nao_projection --steps 1500 --no-cpu-baseline --one-mode > $O/bench_nao_projection_1500_under_rocprof.json 2> $O/trace_projection.err
f=$(find $O/trace_projection -name "*kernel_trace.csv" | head -1)
# the trace holds the recipe that precedes the projection too: its n = 1024 kernels are `<16, ...>` instances -- the window is everything
# AFTER the recipe's last search launch, minus the cold first solve (the r05 file mixed the two runs)
[ -n "$f" ] && python3 tools/kernel_window_stats.py "$f" --after-last "lap_jvmw_kernel<16" --skip 1 --match lap_ > $O/kernel_stats_nao_projection_window.csv
[ -n "$f" ] && python3 tools/solve_spans.py "$f" --last 1490 > $O/solve_spans_nao_projection.txt
[ -n "$f" ] && python3 tools/iteration_glue.py "$f" 1000 > $O/iteration_glue_nao_projection.txt
# launch by launch through a refresh period: every kernel's duration and the idle time in front of it
[ -n "$f" ] && python3 tools/solve_gaps.py "$f" --last 1400 > $O/solve_gaps_nao_projection.txt
f=$(find $O/trace_recipe -name "*kernel_trace.csv" | head -1)
[ -n "$f" ] && python3 tools/solve_gaps.py "$f" --last 1900 > $O/solve_gaps_nao_recipe.txt
# 3a. per-kernel account of REPLAYED solves (dumps under tools/_states/: git-ignored, present where tools/exp_tail.py DUMP=... took them)
for d in proj recipe; do
  if [ -f tools/_states/r05s_$d.npz ]; then
    ORDER=morton REPS=2 RAW_OUT=$O/raw timeout 500 rocprofv3 --kernel-trace -f csv -d $O/rk_$d -- python3 tools/replay_tail.py tools/_states/r05s_$d.npz > $O/replay_tail_$d.txt 2>&1
    f=$(find $O/rk_$d -name "*kernel_trace.csv" | head -1)
    [ -n "$f" ] && python3 tools/replay_kernels.py "$f" $O/raw.r05s_$d.npz > $O/replay_kernels_${d}_after.txt 2>&1
  fi
done
# 3b. README.md:125 on nao, the whole run (15 000 iterations, a snapshot every 10), and the solve-by-solve account of both recipes
timeout 900 python3 tools/run_nao.py --projection 2>/dev/null | grep -v "joint types" > $O/run_nao_projection_det_1.txt
timeout 900 python3 tools/run_nao.py --projection 2>/dev/null | grep -v "joint types" > $O/run_nao_projection_det_2.txt
timeout 900 python3 tools/run_nao.py --projection --no-deterministic 2>/dev/null | grep -v "joint types" > $O/run_nao_projection_nodet.txt
timeout 500 python3 tools/exp_kin_determinism.py 2>&1 | grep -v "amdgpu.ids\|joint types" > $O/exp_kin_determinism.txt
MODE=recipe timeout 400 python3 tools/exp_tail.py 2>/dev/null | grep -v amdgpu.ids > $O/exp_tail_recipe.txt
MODE=projection P_ITERS=3000 timeout 400 python3 tools/exp_tail.py 2>/dev/null | grep -v "amdgpu.ids\|joint types" > $O/exp_tail_projection.txt
# 3d. the solver's constants on sequences they were not tuned on: tools/holdout.sh (its own gpurun call: builds r4 / r5 variants first)
# 4. the README recipe as a sweep on one GPU: 20 canonical frames of one generated sequence, both phases in shared launches, the groups concurrently
rm -rf /tmp/sweep_recipe
timeout 900 python3 -m reart_amd.sweep --synthetic 1 --synthetic_frames 20 --cano all --n_iter 15000 --use_flow_loss --use_assign_loss --energy --save_root /tmp/sweep_recipe > $O/sweep_recipe.line.json 2> $O/sweep_recipe.err
cp /tmp/sweep_recipe/sweep.json $O/sweep_recipe_20x15000_energy.json 2>/dev/null
# summaries
f=$(find $O/stats_clean -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $O/kernel_stats_clean.csv
for C in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_SALU SQ_INSTS_LDS; do
  python3 tools/pmc_sum.py $O/pmc_$C knn_group > $O/pmc_$C.txt 2>&1
done
# the counter summary the bench line cites, stamped with the sources it was measured on
python3 tools/pmc_search_json.py $O > $O/pmc_search.json 2> $O/pmc_search_json.err
# the bench line of the driver's command with every leg, last (both modes of the projection)
timeout 900 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench_driver_default.json 2> $O/bench_driver_default.err
# keep the merge-back small: only the summaries travel
find $O -mindepth 1 -maxdepth 1 -type d -exec rm -rf {} +
ls -la $O
