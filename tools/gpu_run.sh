#!/bin/bash
# tools/gpu_run.sh -- THE gpurun command list, one parameterised runner (GPU box): [ROUND=r04] bash tools/gpu_run.sh <task> [args...]
# (Rounds 2 and 3 kept one throw-away script per call -- 22 of them; their tasks are the cases below.)
# Output goes to gpurun_out/$ROUND/; what is to be judged is copied to profiles/${ROUND}_* afterwards.
#   variants <v...>        parity of the listed VKMR_MAP_VARIANT values (tests/test_gpu_random.py), then interleaved bench A/B of them
#   ab <label:ENV=..>...   interleaved bench A/B (tools/ab_env.sh)
#   clock <log2> [variant] tools/kernel_clock.py on the stamped library (product twin, or the experiments twin with a variant)
#   suite                  the GPU test suite + smoke
#   bench [args]           one bench line
#   measure                PMC passes -> profiles/pmc_latest.json, rocprofv3 kernel stats of the bench command, the full bench line (--full)
#   e2e [log2...]          `vkmr hip:0 < file` of 2^k strings (default 25 26): printed time and process wall, N runs each, the distribution
#   frontend               VKMR_TIMING=1 phases, a pipe, hip-api stats and copy/kernel overlap of `vkmr hip:0`
#   rehearsals             soaks against the oracle; torchrun --nproc 2 (gloo rehearsal; plain N=2 must fail on one GPU); --force-dist (RCCL, one rank)
#   forestupdate [args]    tools/forest_update_timing.py: leaf updates of a stored forest against a rebuild and against the single tree's
#                          update (one JSON line), then the same run under rocprofv3 --kernel-trace --stats; stops at the first failing step
#   sortentries [args]     tools/sort_entries_timing.py: entries sorted on the device in front of a forest update against the route through
#                          the host, and the sort alone beside torch.sort (one JSON line), then the same run under rocprofv3
#                          --kernel-trace --stats; stops at the first failing step
#   find [args]            tools/find_timing.py: the lookup by digest beside a read-only pass of torch's over as many bytes (one JSON line)
#   diff [args]            tools/diff_timing.py: the diff of two stored forests beside torch's compare of the two level-0 buffers, and
#                          sync_from beside a rebuild (one JSON line)
#   audit [args]           tools/audit_timing.py: the audit of a stored forest or tree beside its build, masks only and with the list
#                          (one JSON line), then the same run under rocprofv3 --kernel-trace --stats; stops at the first failing step
#   forest_append [args]   tools/forest_append_timing.py: trees appended to a stored forest (1, 8, 64 of 2 048 leaves; 2^26 and 2^16 leaves
#                          resident) beside the stored build of the final forest and the roots-only reduction of the new leaves (one JSON line)
#   forest_extend [args]   tools/forest_extend_timing.py: the open tree of a stored forest grown by leaves (one tree of 2^26; the last of 2^15
#                          trees) beside truncate + append of the whole tree and the stored build (one JSON line)
#   frontier_extend [args] tools/frontier_extend_timing.py: a holder of the frontier alone following the same growth, beside the primary's
#                          extend and the reduction of all the leaves (one JSON line)
#   consistency [args]     tools/consistency_timing.py: consistency proofs gathered from a stored forest and checked by a holder of two roots
#                          (2^15 trees of 2 048; one tree of 2^26 at Q = 1 and 2^16), beside verify_frontier and the follower's extend (one JSON line)
#   proofs_at [args]       tools/proofs_at_timing.py: inclusion proofs as of an earlier count out of a stored forest (2^15 trees of 2 048 with 32
#                          queries an epoch; one tree of 2^26 - 2^16 at E = 1, k = 2^20 and at E = k = 2^16), beside what they replace: a second
#                          stored forest built from the prefix leaves plus its proof gather (one JSON line)
#   merkleblocks [args]    tools/merkleblocks_timing.py: partial Merkle trees in BIP37 order out of a stored forest (2^15 trees of 2 048; 2^10, 2^16,
#                          2^20 random entries, 2^16 filling whole trees) beside the multiproof gather, its downloads and the gather of a host reordering
#                          (one JSON line)
#   absence [args]         tools/absence_timing.py: sorted trees (2^26 sorted leaves as 2^15 trees of 2 048 and as one tree; Q = 2^10, 2^16, 2^20, half
#                          present): the sorted pass beside torch's sum over as many bytes, the lower bound, the gather, and the verifier beside
#                          vkmr_hip_verify_forest_proofs_async over 2 Q plain proofs (one JSON line)
#   leafsort [args]        tools/leafsort_timing.py: the leaves sorted on the device (2^26 random leaves as 2^15 trees of 2 048 and as one tree): the
#                          sort alone, the sort and the stored build, the build alone, the worst case of the tie step, beside the host route
#                          (download, vk.sort_digests, upload) and torch.sort of as many int64 keys (one JSON line)
#   merge [args]           tools/merge_timing.py: a batch merged into sorted trees (2^26 leaves as 2^15 trees of 2 048 and as one tree): the union with
#                          2^10, 2^16, 2^20 and 2^24 new digests, the difference at 2^16, the union and the stored build, beside the parent's route
#                          (the concatenation sorted again by vkmr_hip_forest_sort_leaves_async) and vkmr_hip_forest_copy_trees_async (one JSON line)
#   range [args]           tools/range_timing.py: range proofs over sorted trees (2^26 leaves as 2^15 trees of 2 048 and as one tree): gather, check and
#                          counting call for 2^10, 2^16 and 2^20 ranges of 16 leaves, 2^10 ranges of 2^16, every tree whole, beside the parent's route
#                          (vkmr_hip_forest_multiproof_async over explicit entries and its check) and vkmr_hip_reduce_forest_async (one JSON line)
#   sorted_set [args]      tests/test_gpu_sorted_set.py: every shape of a sorted tree of up to 40 leaves and the walk of a sorted set, each test with its
#                          duration (pytest --durations=0; further pytest arguments are passed on)
#   scratch [args]         tests/test_gpu_scratch.py: every entry point that takes a scratch_dev from dirty scratch of exactly its size (0x00, 0xFF,
#                          random words, another call's leftovers) and back to back on one stream, each case with its duration (pytest
#                          --durations=0; further pytest arguments are passed on)
#   forest_repack [args]   tools/forest_repack_timing.py: the oldest trees of a stored forest dropped and the rest (or all) copied into an
#                          empty forest, beside the stored build over the same leaves (one JSON line)
#   cumask                 tools/cu_mask_probe.py: where CU-mask bits land, map/reduce on half the CUs with and without neighbours
#   issue <set>            tools/issue_patterns (python3 tools/gen_issue_patterns.py <set> and a build beforehand)
#   proofs                 tools/proof_timing.py: a slice reduced with and without proofs written in the pass
#   treeproofs [args]      tools/tree_proofs_timing.py: stored tree, proof gather, batch verify (one JSON line), then the same run under
#                          rocprofv3 --kernel-trace --stats for the kernel times; stops at the first failing step
#   treeupdate [args]      tools/tree_update_timing.py: leaf updates of a stored tree against a rebuild (one JSON line), then the same
#                          run under rocprofv3 --kernel-trace --stats for the kernel times; stops at the first failing step
cd ${GRAFT_REPO_ROOT:-.}
ROUND=${ROUND:-r04}
OUT=gpurun_out/$ROUND
mkdir -p $OUT
task=$1; shift
case $task in
variants)
  sel=$(printf "%s or " "$@"); sel=${sel% or }
  timeout -k 10 900 python -m pytest tests/test_gpu_random.py -m gpu -q -k "fetch_mode and ($sel)" > $OUT/pytest_variants.log 2>&1; echo "pytest rc=$?"; tail -5 $OUT/pytest_variants.log
  specs="default:"; for v in "$@"; do [ "$v" != 0 ] && specs="$specs exp$v:VKMR_HIP_LIB=$PWD/build/ab/libexp.so,VKMR_MAP_VARIANT=$v"; done
  bash tools/ab_env.sh $specs | tee -a $OUT/ab_variants.txt
  ;;
ab)
  bash tools/ab_env.sh "$@" | tee -a $OUT/ab.txt
  ;;
clock)
  log2=$1; variant=$2
  if [ -n "$variant" ]; then
    VKMR_MAP_VARIANT=$variant timeout -k 10 300 python3 tools/kernel_clock.py --leaves-log2 $log2 --lib build/ab/libexp_stamps.so > $OUT/kernel_clock_${log2}_v$variant.json 2> $OUT/kernel_clock_${log2}_v$variant.err; echo "kernel_clock v$variant rc=$?"
    tail -c 1200 $OUT/kernel_clock_${log2}_v$variant.json
  else
    timeout -k 10 300 python3 tools/kernel_clock.py --leaves-log2 $log2 > $OUT/kernel_clock_$log2.json 2> $OUT/kernel_clock_$log2.err; echo "kernel_clock rc=$?"
    tail -c 1500 $OUT/kernel_clock_$log2.json; tail -12 $OUT/kernel_clock_$log2.err
  fi
  ;;
suite)
  timeout -k 10 1100 python -m pytest tests -m gpu -q --durations=8 > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -14 $OUT/pytest_gpu.log
  python -c "import __graft_entry__ as g; g.smoke()"; echo "smoke rc=$?"
  ;;
bench)
  timeout -k 10 600 python bench.py "$@" > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"; tail -c 3000 $OUT/bench.json
  ;;
measure)
  bash tools/pmc_profile.sh $ROUND > $OUT/pmc.log 2>&1
  ( cd /tmp && export TMPDIR=/tmp
    for c in FETCH_SIZE WRITE_SIZE; do timeout -k 10 120 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $GRAFT_REPO_ROOT/gpurun_out/pmc_${ROUND}_long/$c -- python3 $GRAFT_REPO_ROOT/tools/long_strings_probe.py > /dev/null 2>&1; done )
  python3 tools/pmc_to_json.py gpurun_out/pmc_$ROUND $OUT/pmc_$ROUND.json --long-strings-dir gpurun_out/pmc_${ROUND}_long > /dev/null
  cp $OUT/pmc_$ROUND.json profiles/pmc_latest.json
  cp gpurun_out/pmc_$ROUND/summary.txt $OUT/pmc_summary.txt
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $GRAFT_REPO_ROOT/gpurun_out/prof_$ROUND -- python3 $GRAFT_REPO_ROOT/bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-pipeline --no-clock-leg > $GRAFT_REPO_ROOT/$OUT/prof_bench.json 2> $GRAFT_REPO_ROOT/$OUT/prof_bench.err )
  find gpurun_out/prof_$ROUND -name "*kernel_stats.csv" -exec cp {} $OUT/kernel_stats.csv \;
  timeout -k 10 600 python bench.py --steps 20 --warmup 5 --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"
  ;;
e2e)
  [ $# -eq 0 ] && set -- 25 26
  for k in "$@"; do
    vk_merkle_roots_amd/bin/rndm 42 $((1 << k)) 127 > /tmp/g$k.txt 2>/dev/null
    vk_merkle_roots_amd/bin/vkmr hip:0 < /tmp/g$k.txt > /dev/null 2>&1
    python3 - $k ${E2E_RUNS:-12} <<'PY'
import subprocess, sys, time, statistics
k, n = int(sys.argv[1]), int(sys.argv[2])
printed, wall = [], []
for _ in range(n):
    t = time.time()
    r = subprocess.run(["vk_merkle_roots_amd/bin/vkmr", "hip:0"], stdin=open(f"/tmp/g{k}.txt", "rb"), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    wall.append(time.time() - t)
    line = [l for l in r.stdout.decode().splitlines() if "computed root" in l][-1]
    printed.append(float(line.rsplit(" in ", 1)[1]))
q = statistics.quantiles(printed, n=4)
print(f"vkmr hip:0 < 2^{k} strings, {n} runs: printed min {min(printed):.1f}  quartiles {q[0]:.1f} / {q[1]:.1f} / {q[2]:.1f}  max {max(printed):.1f} ms; process wall median {statistics.median(wall):.3f} s (min {min(wall):.3f})")
print("  printed:", " ".join(f"{p:.1f}" for p in printed))
PY
    rm -f /tmp/g$k.txt
  done 2>&1 | tee $OUT/end_to_end.txt
  ;;
frontend)
  {
  vk_merkle_roots_amd/bin/rndm 42 33554432 127 > /tmp/g25.txt 2>/dev/null
  echo "# VKMR_TIMING=1 vkmr hip:0 < file (2^25 strings)"
  for i in 1 2 3; do python3 -c "
import subprocess, time, os
t=time.time(); r=subprocess.run(['vk_merkle_roots_amd/bin/vkmr','hip:0'], stdin=open('/tmp/g25.txt','rb'), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, VKMR_TIMING='1')); w=time.time()-t
line=[l for l in r.stdout.decode().splitlines() if 'computed root' in l][-1]
print('process wall %.3f s; printed %s ms;' % (w, line.rsplit(' in ',1)[1]), ' | '.join(l for l in r.stderr.decode().splitlines() if 'timing' in l))"; done
  echo "# cat file | vkmr hip:0"
  for i in 1 2 3; do cat /tmp/g25.txt | vk_merkle_roots_amd/bin/vkmr hip:0 2>/dev/null | tail -1; done
  } > $OUT/frontend.txt 2>&1; cat $OUT/frontend.txt
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 120 rocprofv3 --hip-trace --stats --output-format csv -d /tmp/fe_trace -- $GRAFT_REPO_ROOT/vk_merkle_roots_amd/bin/vkmr hip:0 < /tmp/g25.txt > /dev/null 2>&1; find /tmp/fe_trace -name '*hip_api_stats.csv' -exec head -16 {} \; ) > $OUT/frontend_api_stats.txt 2>&1
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 120 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $GRAFT_REPO_ROOT/gpurun_out/trace_$ROUND -- $GRAFT_REPO_ROOT/vk_merkle_roots_amd/bin/vkmr hip:0 < /tmp/g25.txt > /dev/null 2>&1 )
  python3 tools/overlap_from_trace.py gpurun_out/trace_$ROUND > $OUT/copy_map_overlap.txt 2>&1; cat $OUT/copy_map_overlap.txt
  ;;
rehearsals)
  timeout -k 10 300 python3 tests/soak/soak_abi.py ${SOAK_ABI:-150} > $OUT/soak_abi.txt 2>&1; tail -2 $OUT/soak_abi.txt
  timeout -k 10 400 python3 tests/soak/soak_frontend.py ${SOAK_FRONTEND:-200} > $OUT/soak_frontend.txt 2>&1; tail -3 $OUT/soak_frontend.txt
  timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --rehearse-gloo --steps 3 --warmup 1 --full --no-config5 --no-long-strings --cpu-sample-log2 20 > $OUT/bench_torchrun_gloo2.json 2> $OUT/bench_torchrun_gloo2.err; echo "torchrun rehearsal rc=$?"; python3 -c "
import json
d=json.loads(open('$OUT/bench_torchrun_gloo2.json').read().splitlines()[-1]); print({k:d.get(k) for k in ('n_gpus','ms_per_step','root_matches_golden','sub_roots_match_golden')}, d['config']['collective'], 'cpu_baseline' in d, 'valu_roofline' in d)"
  timeout -k 10 200 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29534 bench.py --gpus 2 --steps 2 > $OUT/bench_torchrun_2.json 2> $OUT/bench_torchrun_2.err; echo "torchrun N=2 on one GPU rc=$? (must be non-zero)"; wc -c $OUT/bench_torchrun_2.json
  timeout -k 10 200 python bench.py --force-dist --steps 5 --warmup 2 --no-cpu-baseline --no-pipeline --no-long-strings --no-clock-leg > $OUT/bench_force_dist.json 2> $OUT/bench_force_dist.err; echo "force-dist rc=$?"; python3 -c "
import json
d=json.loads(open('$OUT/bench_force_dist.json').read().splitlines()[-1]); print(d['config']['rccl'], d['gather_ms'], d['root_matches_golden'])"
  ;;
issue)
  timeout -k 10 600 ./tools/issue_patterns ${2:-2.0} > $OUT/issue_patterns_$1.txt 2>&1; tail -40 $OUT/issue_patterns_$1.txt
  ;;
proofs)
  for k in "26 8" "26 1" "26 16" "23 16"; do set -- $k; timeout -k 10 300 python3 tools/proof_timing.py --log2 $1 --proofs $2; done > $OUT/proof_timing.txt 2>&1; cat $OUT/proof_timing.txt
  ;;
treeproofs)
  timeout -k 10 400 python3 tools/tree_proofs_timing.py "$@" > $OUT/tree_proofs_timing.json 2> $OUT/tree_proofs_timing.err && echo "tree_proofs_timing ok" &&
  cat $OUT/tree_proofs_timing.json &&
  repo=$(pwd) &&
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $repo/$OUT/prof_tree -- python3 $repo/tools/tree_proofs_timing.py "$@" > $repo/$OUT/tree_proofs_prof.json 2> $repo/$OUT/tree_proofs_prof.err ) &&
  find $OUT/prof_tree -name "*kernel_stats.csv" -exec cp {} $OUT/tree_proofs_kernel_stats.csv \; &&
  cat $OUT/tree_proofs_kernel_stats.csv
  echo "treeproofs rc=$?"
  ;;
treeupdate)
  timeout -k 10 400 python3 tools/tree_update_timing.py "$@" > $OUT/tree_update_timing.json 2> $OUT/tree_update_timing.err && echo "tree_update_timing ok" &&
  cat $OUT/tree_update_timing.json &&
  repo=$(pwd) &&
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $repo/$OUT/prof_update -- python3 $repo/tools/tree_update_timing.py "$@" > $repo/$OUT/tree_update_prof.json 2> $repo/$OUT/tree_update_prof.err ) &&
  find $OUT/prof_update -name "*kernel_stats.csv" -exec cp {} $OUT/tree_update_kernel_stats.csv \; &&
  cat $OUT/tree_update_kernel_stats.csv
  echo "treeupdate rc=$?"
  ;;
forestupdate)
  timeout -k 10 400 python3 tools/forest_update_timing.py "$@" --out $OUT/forest_update_timing.json > /dev/null 2> $OUT/forest_update_timing.err && echo "forest_update_timing ok" &&
  cat $OUT/forest_update_timing.json &&
  repo=$(pwd) &&
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $repo/$OUT/prof_forest_update -- python3 $repo/tools/forest_update_timing.py "$@" > $repo/$OUT/forest_update_prof.json 2> $repo/$OUT/forest_update_prof.err ) &&
  find $OUT/prof_forest_update -name "*kernel_stats.csv" -exec cp {} $OUT/forest_update_kernel_stats.csv \; &&
  cat $OUT/forest_update_kernel_stats.csv
  echo "forestupdate rc=$?"
  ;;
sortentries)
  timeout -k 10 500 python3 tools/sort_entries_timing.py "$@" --out $OUT/sort_entries_timing.json > /dev/null 2> $OUT/sort_entries_timing.err && echo "sort_entries_timing ok" &&
  cat $OUT/sort_entries_timing.json &&
  repo=$(pwd) &&
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $repo/$OUT/prof_sort_entries -- python3 $repo/tools/sort_entries_timing.py "$@" --runs 3 > $repo/$OUT/sort_entries_prof.json 2> $repo/$OUT/sort_entries_prof.err ) &&
  find $OUT/prof_sort_entries -name "*kernel_stats.csv" -exec cp {} $OUT/sort_entries_kernel_stats.csv \; &&
  cat $OUT/sort_entries_kernel_stats.csv
  echo "sortentries rc=$?"
  ;;
find)
  timeout -k 10 500 python3 tools/find_timing.py "$@" --out $OUT/find_timing.json > /dev/null 2> $OUT/find_timing.err && echo "find_timing ok" &&
  cat $OUT/find_timing.json
  echo "find rc=$?"
  ;;
diff)
  timeout -k 10 500 python3 tools/diff_timing.py "$@" --out $OUT/diff_timing.json > /dev/null 2> $OUT/diff_timing.err && echo "diff_timing ok" &&
  cat $OUT/diff_timing.json
  echo "diff rc=$?"
  ;;
audit)
  timeout -k 10 500 python3 tools/audit_timing.py "$@" --out $OUT/audit_timing.json > /dev/null 2> $OUT/audit_timing.err && echo "audit_timing ok" &&
  cat $OUT/audit_timing.json &&
  repo=$(pwd) &&
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $repo/$OUT/prof_audit -- python3 $repo/tools/audit_timing.py "$@" --runs 3 > $repo/$OUT/audit_prof.json 2> $repo/$OUT/audit_prof.err ) &&
  find $OUT/prof_audit -name "*kernel_stats.csv" -exec cp {} $OUT/audit_kernel_stats.csv \; &&
  cat $OUT/audit_kernel_stats.csv
  echo "audit rc=$?"
  ;;
forest_append)
  timeout -k 10 500 python3 tools/forest_append_timing.py "$@" --out $OUT/forest_append_timing.json > /dev/null 2> $OUT/forest_append_timing.err && echo "forest_append_timing ok" &&
  cat $OUT/forest_append_timing.json
  echo "forest_append rc=$?"
  ;;
forest_extend)
  timeout -k 10 500 python3 tools/forest_extend_timing.py "$@" --out $OUT/forest_extend_timing.json > /dev/null 2> $OUT/forest_extend_timing.err && echo "forest_extend_timing ok" &&
  cat $OUT/forest_extend_timing.json
  echo "forest_extend rc=$?"
  ;;
frontier_extend)
  timeout -k 10 500 python3 tools/frontier_extend_timing.py "$@" --out $OUT/frontier_extend_timing.json > /dev/null 2> $OUT/frontier_extend_timing.err && echo "frontier_extend_timing ok" &&
  cat $OUT/frontier_extend_timing.json
  echo "frontier_extend rc=$?"
  ;;
consistency)
  timeout -k 10 500 python3 tools/consistency_timing.py "$@" --out $OUT/consistency_timing.json > /dev/null 2> $OUT/consistency_timing.err && echo "consistency_timing ok" &&
  cat $OUT/consistency_timing.json
  echo "consistency rc=$?"
  ;;
merkleblocks)
  timeout -k 10 500 python3 tools/merkleblocks_timing.py "$@" --out $OUT/merkleblocks_timing.json > /dev/null 2> $OUT/merkleblocks_timing.err && echo "merkleblocks_timing ok" &&
  cat $OUT/merkleblocks_timing.json
  echo "merkleblocks rc=$?"
  ;;
proofs_at)
  timeout -k 10 500 python3 tools/proofs_at_timing.py "$@" --out $OUT/proofs_at_timing.json > /dev/null 2> $OUT/proofs_at_timing.err && echo "proofs_at_timing ok" &&
  cat $OUT/proofs_at_timing.json
  echo "proofs_at rc=$?"
  ;;
absence)
  timeout -k 10 500 python3 tools/absence_timing.py "$@" --out $OUT/absence_timing.json > /dev/null 2> $OUT/absence_timing.err && echo "absence_timing ok" &&
  cat $OUT/absence_timing.json
  echo "absence rc=$?"
  ;;
leafsort)
  timeout -k 10 900 python3 tools/leafsort_timing.py "$@" --out $OUT/leafsort_timing.json > /dev/null 2> $OUT/leafsort_timing.err && echo "leafsort_timing ok" &&
  cat $OUT/leafsort_timing.json
  echo "leafsort rc=$?"
  ;;
merge)
  timeout -k 10 900 python3 tools/merge_timing.py "$@" --out $OUT/merge_timing.json > /dev/null 2> $OUT/merge_timing.err && echo "merge_timing ok" &&
  cat $OUT/merge_timing.json
  echo "merge rc=$?"
  ;;
range)
  timeout -k 10 900 python3 tools/range_timing.py "$@" --out $OUT/range_timing.json > /dev/null 2> $OUT/range_timing.err && echo "range_timing ok" &&
  cat $OUT/range_timing.json
  echo "range rc=$?"
  ;;
sorted_set)
  timeout -k 10 600 python -m pytest tests/test_gpu_sorted_set.py -m gpu -q --durations=0 "$@" > $OUT/pytest_sorted_set.log 2>&1 && echo "sorted_set ok" &&
  grep -E "passed|call " $OUT/pytest_sorted_set.log || tail -40 $OUT/pytest_sorted_set.log
  echo "sorted_set rc=$?"
  ;;
scratch)
  timeout -k 10 600 python -m pytest tests/test_gpu_scratch.py -m gpu -q --durations=0 "$@" > $OUT/pytest_scratch.log 2>&1 && echo "scratch ok" &&
  grep -E "passed|call " $OUT/pytest_scratch.log || tail -60 $OUT/pytest_scratch.log
  echo "scratch rc=$?"
  ;;
forest_repack)
  timeout -k 10 500 python3 tools/forest_repack_timing.py "$@" --out $OUT/forest_repack_timing.json > /dev/null 2> $OUT/forest_repack_timing.err && echo "forest_repack_timing ok" &&
  cat $OUT/forest_repack_timing.json
  echo "forest_repack rc=$?"
  ;;
cumask)
  hipcc --offload-arch=gfx950 -O2 -shared -fPIC -o tools/libwhere.so tools/where.hip
  timeout -k 10 400 python3 tools/cu_mask_probe.py > $OUT/cu_mask_probe.txt 2>&1; tail -14 $OUT/cu_mask_probe.txt
  ;;
*) echo "unknown task $task"; exit 2;;
esac
