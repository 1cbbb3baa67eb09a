# Floors for the cfg2 launch (tools/microbench.hip, prebuilt) + a quick cfg2 bench line.
# usage: bash tools/gpu_floor.sh [output directory]
set -u
cd "$GRAFT_REPO_ROOT"
O="${1:-genome-assembly-using-overlap-graphs_amd/build/floor}"
mkdir -p "$O"
timeout -k 10 120 genome-assembly-using-overlap-graphs_amd/build/microbench > "$O/microbench.txt" 2>&1 || exit 1
cat "$O/microbench.txt"
timeout -k 10 300 python bench.py --full --steps 2000 --warmup 20 --no-extra --no-cpu-baseline > "$O/cfg2.json" 2> "$O/cfg2.err" || { tail -5 "$O/cfg2.err"; exit 1; }
python -c "import json; d=json.loads(open('$O/cfg2.json').read().strip().splitlines()[-1]); print(d['value'], d['roofline']['launch_ms'], d['kernel_only_roofline']['kernel_ms'])"
