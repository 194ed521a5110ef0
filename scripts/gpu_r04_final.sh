#!/bin/bash
# Round-4 round-end evidence on one MI355X (records under gpurun_out/r04_final/<tag>):
#   gpurun --timeout 1200 -- 'bash scripts/gpu_r04_final.sh <tag>'
#   1. the whole GPU suite (pytest -m gpu) and smoke();
#   2. the default bench line (PMC passes in child processes, CPU baseline on the same graph);
#   3. rocprofv3 --kernel-trace --stats of the bench (no PMC, no CPU baseline);
#   4. the carrier steps (HCCF variants incl. the reference's mask stream, LocalAware).
# Each step has its own limit; the first failure ends the script.
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
O=gpurun_out/r04_final/${1:-final}
mkdir -p $O
export TMPDIR=/tmp
( while sleep 45; do echo "[r04 final] $(date +%T) $(ls -t $O | head -1)"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null' EXIT
git_head=$(cat .git_head 2>/dev/null || echo unknown)
echo "HEAD $git_head" > $O/HEAD.txt
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
    -p no:cacheprovider > $O/pytest.txt 2>&1 && tail -1 $O/pytest.txt && \
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1 && \
tail -1 $O/smoke.txt && \
timeout -k 10 600 python -u bench.py --full > $O/bench.json 2> $O/bench.err && echo "bench ok" && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- \
    python bench.py --no-cpu-baseline --pmc off > $O/bench_prof.json 2> $O/bench_prof.err && \
find $O/prof -name '*kernel_stats.csv' -exec cp {} $O/bench_kernel_stats.csv \; && \
rm -rf $O/prof && echo "prof ok" && \
timeout -k 10 300 python -u scripts/bench_hccf.py \
    --variants hgd_cpu_mask,hgd_device_mask,hgd_graph,hgd_graph_cpu_mask > $O/hccf.jsonl 2>&1 && \
timeout -k 10 300 python -u scripts/bench_local_aware.py > $O/la.jsonl 2>&1 && echo "carriers ok"
rc=$?
echo "rc=$rc"
exit $rc
