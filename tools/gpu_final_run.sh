# consolidated GPU run: tests, PMC passes (stamped), bench line (reads the fresh stamp), rocprofv3 kernel stats of the same command,
# ORB (configs[2]) kernel times + HBM traffic.   usage (GPU box, repo root): ALVA_COMMIT=<sha> TAG=r5x OUT=<results dir> tools/gpu_final_run.sh
# Every GPU step has a time limit of its own, and the first step that fails, faults or times out ends the run.
set -eo pipefail
export ALVA_COMMIT=${ALVA_COMMIT:-unknown}
T=${TAG:-r6}
: "${OUT:?OUT=<results dir> is required}"
mkdir -p "$OUT"
O=$(cd "$OUT" && pwd)
timeout -k 10 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/${T}_pytest.log
timeout -k 10 1800 tools/pmc_klt.sh > $O/${T}_pmc.log 2>&1
cp gpurun_out/r6_pmc_track_klt.json profiles/r6_pmc_track_klt.json
timeout -k 10 660 python bench.py --full > $O/${T}_bench_line.json 2> $O/${T}_bench.err
cp bench_detail.json $O/${T}_bench_detail.json
tail -c 300 $O/${T}_bench.err
R=$PWD
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d /tmp/prof_$T -o bench --output-format csv -- python $R/bench.py --full --no-cpu-baseline --quick > $O/${T}_bench_prof.log 2>&1
cp $(find /tmp/prof_$T -name '*kernel_stats.csv' | head -1) $O/${T}_kernel_stats_bench.csv
cd $R
timeout -k 10 300 python tools/orb_kernels.py 1280 720 4000 > $O/${T}_orb_kernels_720p.txt 2>&1
LINES_OUT=12 timeout -k 10 900 tools/pmc_traffic.sh ${T}_orb720 python tools/orb_kernels.py 1280 720 4000 > $O/${T}_orb720_pmc.txt 2>&1
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > $O/${T}_smoke.log 2>&1; tail -1 $O/${T}_smoke.log
cat $O/${T}_pytest.log
wc -c $O/${T}_bench_line.json
# optional: the sustained loop under the in-tree build against every ab_variants/lib_*.so (ALVA_LIB), alternating, when AB=1
if [ "${AB:-0}" = 1 ] && ls ab_variants/lib_*.so >/dev/null 2>&1; then
  timeout -k 10 1800 bash tools/variant_run.sh "python tools/system_sustained.py" > $O/${T}_ab.txt 2>&1
  grep -n "^==\|frames/s" $O/${T}_ab.txt | cut -c1-160 || true
fi
