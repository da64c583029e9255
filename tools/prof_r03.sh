# rocprofv3 passes behind profiles/r03* (run on the GPU box from the repository root: bash tools/prof_r03.sh)
: "${GRAFT_REPO_ROOT:=$(cd "$(dirname "$0")/.." && pwd)}"; export GRAFT_REPO_ROOT    # the repository root (gpurun exports it; derived from $0 elsewhere)
R=$GRAFT_REPO_ROOT; cd /tmp; export TMPDIR=/tmp
set -e    # every pass has its own time limit; a failed, faulted or timed-out pass ends the script
O=${PROF_OUT:-$R/prof_out}; mkdir -p $O; export PROF_OUT=$O    # output directory of the passes (PROF_OUT, default prof_out/)
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/r03_trace -o r03 -- python3 $R/bench.py --full --no-cpu-baseline --steps 3 --warmup 1 > $O/r03_bench_under_rocprof.log 2>&1
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/r03_pmc_fetch -o f -- python3 $R/tools/pmc_kernels.py > $O/r03_pmc_fetch.log 2>&1
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/r03_pmc_write -o w -- python3 $R/tools/pmc_kernels.py > $O/r03_pmc_write.log 2>&1
timeout -k 10 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $O/r03_pmc_mfma -o m -- python3 $R/bench.py --full --no-cpu-baseline --no-secondary --steps 1 --warmup 0 > $O/r03_pmc_mfma.log 2>&1
cd $R; python3 tools/prof_r03_summarise.py
