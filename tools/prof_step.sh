# usage: prof_step.sh <tag> [bench args...]   kernel-trace of bench.py --full, summary of the last 3 steps
#        -> $OUT_DIR/step_<tag>_kernels.csv (default out/ in the repository)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
tag=$1; shift
out=${OUT_DIR:-$R/out}; mkdir -p $out
rm -rf /tmp/profs_$tag
rocprofv3 --kernel-trace --memory-copy-trace -d /tmp/profs_$tag -- python3 $R/bench.py --full --steps 4 --warmup 3 --no-cpu-baseline --no-split-line --no-op-line "$@" > $out/step_${tag}.json 2> $out/step_${tag}.err
python3 $R/tools/prof_summary.py $(dirname $(find /tmp/profs_$tag -name "*.db" | head -1)) $out/step_${tag}_kernels.csv 3
python3 $R/tools/prof_sequence.py $(dirname $(find /tmp/profs_$tag -name "*.db" | head -1)) $out/step_${tag}_sequence.txt
python3 $R/tools/prof_gaps.py $(dirname $(find /tmp/profs_$tag -name "*.db" | head -1)) 1 20 > $out/step_${tag}_gaps.txt 2>&1
