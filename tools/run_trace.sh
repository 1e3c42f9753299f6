# Kernel trace of one bench step: bash tools/run_trace.sh <outdir> <bench args...>
cd /root/repo
export TMPDIR=/tmp
O=gpurun_out/$1
shift
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace -o b -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline "$@" > $O/trace.log 2>&1 || exit 1
echo ALLDONE
