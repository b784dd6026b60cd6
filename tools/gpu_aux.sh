#!/bin/bash
# Beyond-configs[1] measurements in one call: Gatys 512^2 Adam step (+ rocprofv3 stats of it), per-architecture
# frames/s, configs[4] mask step, the CLI with host PNG/JPEG I/O, the post chain.  Each step under its own limit.
#   bash tools/gpu_aux.sh <tag>
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
OUT=${NST_OUT_DIR:-out}  # where the logs and results go
mkdir -p "$OUT"
export TMPDIR=/tmp
T=${1:-aux}
timeout -k 10 300 python -u bench.py --steps 20 --warmup 5 --full --no-cpu-baseline > $OUT/bench_$T.json 2> $OUT/bench_$T.err || { echo "bench failed"; tail -30 $OUT/bench_$T.err; exit 1; }
python tools/bench_brief.py $OUT/bench_$T.json
timeout -k 10 200 python -u tools/batch_sweep.py 8 4 2 1 > $OUT/batch_$T.txt 2>&1 || { tail -20 $OUT/batch_$T.txt; exit 1; }
grep batch $OUT/batch_$T.txt
GATYS_STEPS=100 timeout -k 10 240 python -u tools/gatys_bench.py > $OUT/gatys_$T.json 2> $OUT/gatys_$T.err || { tail -20 $OUT/gatys_$T.err; exit 1; }
cat $OUT/gatys_$T.json
GATYS_STEPS=30 timeout -s KILL 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_gatys_$T -o gatys -- python3 tools/gatys_bench.py > $OUT/prof_gatys_$T.log 2>&1 || { echo "gatys prof failed"; tail -20 $OUT/prof_gatys_$T.log; exit 1; }
timeout -k 10 300 python -u tools/arch_bench.py > $OUT/arch_$T.txt 2>&1 || { tail -20 $OUT/arch_$T.txt; exit 1; }
grep -v amdgpu.ids $OUT/arch_$T.txt
timeout -k 10 300 python -u tools/seg_bench.py > $OUT/seg_$T.json 2> $OUT/seg_$T.err || { tail -20 $OUT/seg_$T.err; exit 1; }
tail -3 $OUT/seg_$T.json
timeout -k 10 400 python -u tools/cli_bench.py --frames 48 > $OUT/cli_$T.json 2> $OUT/cli_$T.err || { tail -20 $OUT/cli_$T.err; exit 1; }
tail -3 $OUT/cli_$T.json
timeout -k 10 200 python -u tools/post_bench.py > $OUT/post_$T.txt 2>&1 || { echo "post bench failed"; tail -5 $OUT/post_$T.txt; exit 1; }
grep -v amdgpu.ids $OUT/post_$T.txt | tail -30
