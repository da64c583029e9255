cd /tmp; export TMPDIR=/tmp
: "${GRAFT_REPO_ROOT:=$(cd "$(dirname "$0")/../.." && pwd)}"; export GRAFT_REPO_ROOT
R=$GRAFT_REPO_ROOT
set -e    # every pass has its own time limit; a failed, faulted or timed-out pass ends the script
O=${PROF_OUT:-$R/prof_out}; mkdir -p $O; export PROF_OUT=$O    # output directory of the passes (PROF_OUT, default prof_out/)
timeout -k 10 600 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum --kernel-trace --output-format csv -d $O/pmc_l2a -o a -- python3 $R/bench.py --full --no-cpu-baseline --no-secondary --steps 1 --warmup 0 > $O/pmc_l2a.log 2>&1
timeout -k 10 600 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum TCC_EA0_RDREQ_32B_sum --kernel-trace --output-format csv -d $O/pmc_l2b -o b -- python3 $R/bench.py --full --no-cpu-baseline --no-secondary --steps 1 --warmup 0 > $O/pmc_l2b.log 2>&1
cd $R
python3 - <<'PY'
import csv, glob, collections, os
for tag in ('a','b'):
    G=os.environ['PROF_OUT']; f=glob.glob(G + '/pmc_l2%s/**/*counter_collection.csv' % tag, recursive=True)
    if not f: print(tag,'no csv', glob.glob(G + '/pmc_l2%s/**/*' % tag, recursive=True)[:5]); continue
    acc=collections.defaultdict(lambda: collections.defaultdict(float)); n=collections.Counter()
    for row in csv.DictReader(open(f[0])):
        k=row['Kernel_Name'][:60]
        acc[k][row['Counter_Name']]+=float(row['Counter_Value']); 
    for k,v in acc.items():
        if 'lean' in k or 'proj' in k: print(tag, k, dict(v))
PY
