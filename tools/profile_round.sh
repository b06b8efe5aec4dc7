#!/bin/bash
# Profiling passes of one round, run ON THE GPU BOX:   gpurun -- 'bash tools/profile_round.sh r02'
#   1. rocprofv3 --kernel-trace --stats of one full default bench step (decode synchronised every 64 steps: the tracer
#      segfaults with > ~150 graph launches queued);
#   2. three SEPARATE --pmc passes (FETCH_SIZE / WRITE_SIZE / MFMA busy + GRBM_GUI_ACTIVE) of a short eager step (6 new tokens),
#      each with --kernel-trace only (gpurun refuses --pmc together with the other trace domains).
# Summaries land in gpurun_out/prof_<tag>/ and are copied to profiles/ by the builder.
TAG=${1:-r03}
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$REPO/gpurun_out/prof_$TAG
rm -rf "$OUT"
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
BENCH="python $REPO/bench.py --full --no-cpu-baseline --no-power"
if [ "$2" != "pmc" ]; then
for attempt in 1 2 3; do      # the tracer itself segfaults now and then inside a kernel launch: retry
  rm -rf "$OUT/trace"
  timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o trace -- $BENCH --steps 1 --warmup 0 --decode-chunk 64 > "$OUT/trace.log" 2>&1 && break
done
python "$REPO/tools/rocprof_summary.py" stats "$OUT/trace" "$OUT/${TAG}_kernel_stats.txt" > /dev/null
python "$REPO/tools/rocprof_summary.py" shapes "$OUT/trace" "$OUT/${TAG}_kernel_shapes.txt" > /dev/null
# 1b. (round 5) the kernels of the schedule the driver TIMES: the default overlapped continuous-batching loop itself.
#     Round 6: the loop bounds its own run-ahead (<= 24 graph replays queued, front ends as graph replays), which the tracer survives as
#     it is - no --sync-chunks any more: this IS the timed loop.  One fill + warm-up cycles + one timed cycle.
# the tracer (rocprofv3 of this image) segfaults in some runs of the loop as it is; fall back to a chunk-synchronised loop, then to eager front ends
for extra in "" "--sync-chunks" "--sync-chunks --front-graph 0"; do
  rm -rf "$OUT/trace_ov"
  echo "overlapped trace: flags [$extra]" >> "$OUT/trace_ov_attempts.log"
  timeout 1500 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_ov" -o trace -- $BENCH --steps 1 --warmup 2 --no-instrument --no-single-stream --no-latency-point $extra > "$OUT/trace_ov.log" 2>&1 && break
done
python "$REPO/tools/rocprof_summary.py" stats "$OUT/trace_ov" "$OUT/${TAG}_kernel_stats_overlapped.txt" > /dev/null
python "$REPO/tools/overlap_trace_summary.py" "$OUT/trace_ov" > "$OUT/${TAG}_overlap_trace_summary.txt" 2>&1
tail -1 "$OUT/trace_ov.log" | cut -c1-300
fi
# counters serialise every dispatch.  Round 3: the pass runs at the DEFAULT batch (128 slots) with the default schedule's prefill groups
# of 4 clips, so that every kernel is counted at the launch shape the bench line quotes it at (decode kernels at 128 rows and a context
# of 2142 + <= 5 tokens; prefill GEMMs at M = 4 x 2144) - VERDICT r2: round 2 scaled a 64-row pass and quoted an M = 17152 GEMM
SHORT="$BENCH --batch ${PMC_BATCH:-128} --prefill-group 4 --steps 1 --warmup 0 --max_new_tokens 6 --no-graph --no-instrument --batch-mode --sync-front"
# rocprofv3's counter mode segfaults now and then in a kernel launch (round 3: in the first 128-row skinny launch, three times out of four;
# the same pass ran clean earlier the same day) - retry every pass, and fall back to 120 slots (the same 8-column-group kernels) if 128 keeps failing
pmc_pass() {   # name, counters...
  local name=$1; shift
  for attempt in 1 2 3 4; do
    rm -rf "$OUT/pmc_$name"
    timeout 1500 rocprofv3 --pmc "$@" --kernel-trace --output-format csv -d "$OUT/pmc_$name" -o $name -- $SHORT > "$OUT/pmc_$name.log" 2>&1 && return 0
    echo "pmc pass $name: attempt $attempt failed (rc $?)"
  done
  return 1
}
pmc_pass fetch FETCH_SIZE
pmc_pass write WRITE_SIZE
pmc_pass mfma SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE
pmc_pass ealat TCC_EA0_RDREQ_LEVEL_sum TCC_EA0_RDREQ_sum
python "$REPO/tools/pmc_summary.py" "$OUT" "$OUT/${TAG}_pmc.json" $(( ${PMC_BATCH:-128} * 2145 )) > "$OUT/${TAG}_pmc_summary.txt" 2>&1
# keep the merge-back under 64 MiB: drop the raw per-dispatch csv / db files, keep logs + summaries
for f in $(find "$OUT" -name "*counter_collection.csv" | head -3); do head -3 "$f" > "$f.head.txt"; done
find "$OUT" -name "*.csv" -size +2M -delete
find "$OUT" -name "*.db" -delete
ls -la "$OUT"
tail -3 "$OUT/trace.log"
head -50 "$OUT/${TAG}_pmc_summary.txt"
