# per-kernel profile of the bench step (single stream, so that kernel times add up): rocprofv3 --kernel-trace --stats
# usage (GPU box): bash tools/profile_step.sh TAG [bench args]   -> $MEANT_PROFILE_OUT/prof_TAG/{stats.csv,bench.log}
# (MEANT_PROFILE_OUT: the output directory, default profile_out/ in the repository)
R=$(cd "$(dirname "$0")/.." && pwd); TAG=$1; shift
D=${MEANT_PROFILE_OUT:-$R/profile_out}/prof_$TAG
cd /tmp && export TMPDIR=/tmp
mkdir -p $D
MEANT_TWO_STREAMS=0 rocprofv3 --kernel-trace --stats -d $D -o x -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline "$@" > $D/bench.log 2>&1
python3 $R/tools/rocprof_stats.py $D/x_results.db $D/stats.csv | head -40
tail -1 $D/bench.log | cut -c1-200
