# usage (GPU box): bash tools/round_end.sh <tag> <out-dir>   -> the GPU suite's log and the full bench line (bench.py --full) in
# <out-dir>; the round's profiles (tools/prof_round.sh, tools/small_shapes_profile.sh) go where those scripts write them
R=$(cd "$(dirname "$0")/.." && pwd)
tag=${1:-r06}
out=$(mkdir -p "${2:?usage: round_end.sh <tag> <out-dir>}" && cd "$2" && pwd)
cd $R
timeout 1500 python3 -m pytest tests -m gpu -x -q > $out/${tag}_pytest_gpu.log 2>&1
tail -3 $out/${tag}_pytest_gpu.log
timeout 900 bash tools/prof_round.sh $tag
cd $R
timeout 900 bash tools/small_shapes_profile.sh $tag > $out/${tag}_small_shapes.log 2>&1
cd $R
timeout 900 python3 bench.py --full --steps 20 --warmup 3 > $out/${tag}_bench_line.json 2> $out/${tag}_bench_line.err
cut -c1-400 $out/${tag}_bench_line.json
