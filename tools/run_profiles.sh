# Evidence run of a round: bash tools/run_profiles.sh <rNN>.  Everything lands under bench_out/<rNN>/:
#   bench_line.json     the LAST stdout line of `python bench.py --full`; bench_stdout.txt = all of it (the `paths` line first)
#   small_workloads.json  bench_small.py: the reference's own benchmark sizes, per call
#   stats_headline/     rocprofv3 --kernel-trace --stats of `bench.py --full` without the CPU leg and without `paths`
#   stats/              the same with `paths`: kernel averages of every other row's kernels
#   pmc_headline.json   FETCH/WRITE/TCC/SQ counters of the headline kernel (one counter group per run, --kernel-trace only)
#   pmc_paths/          FETCH_SIZE / WRITE_SIZE / TCC / SQ passes over bench_paths.py (every other section-8 row)
cd "$(dirname "$0")/.." || exit 1
R=$PWD
R5=${1:-r05}
O=$R/bench_out/$R5
mkdir -p $O/pmc_paths
timeout 600 python bench.py --full --steps 20 --warmup 5 > $O/bench_stdout.txt 2> $O/bench_stderr.txt
tail -1 $O/bench_stdout.txt > $O/bench_line.json
timeout 900 python bench_small.py --profile --out $O/small_workloads.json > $O/small_workloads.txt 2>&1
# rocprofv3 runs from the temporary directory: nothing of its own lands in the tree
cd "${TMPDIR:-/tmp}" || exit 1
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_headline -o b -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu --no-paths > $O/stats_headline.log 2>&1
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o b -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu > $O/stats.log 2>&1
bash $R/tools/tools_pmc.sh $R5 spmm_tiled fetch write tcc sq > $O/pmc_headline.json 2>&1
run() { name=$1; shift; timeout 600 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $O/pmc_paths/$name -o p -- python $R/bench_paths.py > $O/pmc_paths/$name.log 2>&1; }
run fetch FETCH_SIZE
run write WRITE_SIZE
run tcc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum
run lds SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY
python $R/tools/summarise_profiles.py $O > $O/summary.txt 2>&1
# only summaries are kept: the raw per-dispatch counter tables are deleted
find $O -name '*counter_collection.csv' -delete
find $O -name '*kernel_trace.csv' -delete
ls $O
