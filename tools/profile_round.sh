# one call that collects what profiles/ holds for a build (GPU box): bash tools/profile_round.sh TAG
#   $MEANT_PROFILE_OUT/TAG_pmc_fetch_size, TAG_pmc_write_size (+ TAG_hbm_traffic.json), sq_TAG.txt, prof_TAG/, TAG_bench.json
#   (MEANT_PROFILE_OUT: the output directory, default profile_out/ in the repository)
R=$(cd "$(dirname "$0")/.." && pwd); TAG=$1
O=${MEANT_PROFILE_OUT:-$R/profile_out}; export MEANT_PROFILE_OUT=$O
cd /tmp && export TMPDIR=/tmp
mkdir -p $O
for c in FETCH_SIZE WRITE_SIZE; do
  d=$O/${TAG}_pmc_$(echo $c | tr A-Z a-z); rm -rf $d
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $d -o x -- python3 $R/tools/pmc_step_kernels.py > $d.log 2>&1
done
python3 $R/tools/parse_pmc_kernels.py $O/${TAG}_pmc_fetch_size $O/${TAG}_pmc_write_size $O/${TAG}_hbm_traffic.json > /dev/null 2> $O/${TAG}_parse.err
echo "== traffic"; grep -A8 "attn_bwd1" $O/${TAG}_hbm_traffic.json | grep -E "attn_bwd1|in_units"
bash $R/tools/pmc_sq.sh $TAG tools/probe_attn2.py 2 2> /dev/null > $O/sq_$TAG.txt
echo "== sq"; grep -A1 "attn_" $O/sq_$TAG.txt | cut -c1-400
bash $R/tools/profile_step.sh $TAG > $O/${TAG}_profile_step.log 2>&1
echo "== step"; head -14 $O/${TAG}_profile_step.log | cut -c1-160
cd $R && python3 bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
echo "== bench"; tail -1 $O/${TAG}_bench.json | cut -c1-400
