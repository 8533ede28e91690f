set -o pipefail
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
D=${OUT:-$R/runs}/r2a
mkdir -p $D
cd $R
timeout -k 10 600 python -m pytest tests -x -q -m gpu > $D/gpu_tests.log 2>&1 ; echo "tests rc=$?"; tail -3 $D/gpu_tests.log
( time timeout -k 10 500 python bench.py --full > $D/bench_default.log 2>&1 ) 2>&1 | grep real; tail -c 600 $D/bench_default.log
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/kt -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $D/kt.log 2>&1; echo "kt rc=$?"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D/pf -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --in-flight 1 > $D/pf.log 2>&1; echo "pf rc=$?"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $D/pw -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --in-flight 1 > $D/pw.log 2>&1; echo "pw rc=$?"
cd $R
find $D -name "*.csv" | head -20
# keep only the small summaries
find $D/kt -name "*kernel_trace.csv" -delete
