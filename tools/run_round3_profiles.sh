# Round-3 evidence: GPU tests, default bench line, kernel trace + stats, FETCH_SIZE / WRITE_SIZE passes (separate runs, no trace flags).
# usage (on the MI355X): bash tools/run_round3_profiles.sh <tag>      -> $OUT/<tag>/ (OUT: runs/ of the repository unless set)
set -o pipefail
export TMPDIR=/tmp
TAG=${1:-r3a}
R=$(cd "$(dirname "$0")/.." && pwd)
D=${OUT:-$R/runs}/$TAG
mkdir -p $D
( time timeout -k 10 500 python $R/bench.py --full > $D/bench_default.json 2> $D/bench_default.err ) 2>&1 | grep real
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/kt -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $D/kt.log 2>&1; echo "kt rc=$?"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D/pf -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --in-flight 1 > $D/pf.log 2>&1; echo "pf rc=$?"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $D/pw -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --in-flight 1 > $D/pw.log 2>&1; echo "pw rc=$?"
cd $R
find $D/kt -name "*kernel_trace.csv" -delete
python3 tools/pmc_traffic.py $(find $D/pf -name "*counter_collection.csv" | head -1) $(find $D/pw -name "*counter_collection.csv" | head -1) $D/pmc_traffic.json > $D/pmc_traffic.log 2>&1; tail -3 $D/pmc_traffic.log
head -c 300 $D/bench_default.json
