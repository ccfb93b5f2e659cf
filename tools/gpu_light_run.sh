# a short GPU run for commits that change host-side code only (the PMC stamp and the kernel statistics of the last consolidated run stay
# valid): tests, then the bench line.   usage (GPU box, repo root): ALVA_COMMIT=<sha> TAG=r5x OUT=<results dir> tools/gpu_light_run.sh
# Every GPU step has a time limit of its own, and the first step that fails, faults or times out ends the run.
set -eo pipefail
export ALVA_COMMIT=${ALVA_COMMIT:-unknown}
T=${TAG:-r5}
: "${OUT:?OUT=<results dir> is required}"
mkdir -p "$OUT"
O=$(cd "$OUT" && pwd)
timeout -k 10 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/${T}_pytest.log
cat $O/${T}_pytest.log
timeout -k 10 660 python bench.py --full > $O/${T}_bench_line.json 2> $O/${T}_bench.err
cp bench_detail.json $O/${T}_bench_detail.json
tail -c 200 $O/${T}_bench.err
wc -c $O/${T}_bench_line.json
