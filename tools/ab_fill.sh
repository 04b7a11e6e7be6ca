# kernel-trace stats of the bench's headline and per-kernel legs, then the same bench unprofiled
# usage (from the repository root): tools/ab_fill.sh [output folder, default out]
set -e
export TMPDIR=/tmp
out=${1:-out}
mkdir -p "$out"
B="python bench.py --full --skip-256 --skip-config5 --skip-ob02 --no-cpu-baseline"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out/ab" -o run -- $B --steps 20 > "$out/ab.json" 2>"$out/ab.err"
timeout -k 10 300 $B --steps 50 > "$out/ab2.json" 2>"$out/ab2.err"
