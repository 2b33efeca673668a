#!/bin/bash
# the GPU suite, the full bench line and a rocprofv3 kernel-trace pass of the headline, written under OUT_DIR (relative to the repository root)
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
O=${1:?usage: tools/gpu_full.sh OUT_DIR}; mkdir -p $O
timeout 2400 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > $O/gputests.txt
python bench.py --full > $O/bench.json 2> $O/bench.err
rocprofv3 --kernel-trace --stats -d $O/prof -o stats -- python bench.py --no-cpu-baseline --no-roofline > $O/prof_bench.json 2> $O/prof.err
python tools/rocpd_summary.py $(ls $O/prof/*/*.db $O/prof/*.db 2>/dev/null | head -1) > $O/kernel_stats.txt 2>&1
cat $O/gputests.txt; cut -c1-600 $O/bench.json; head -12 $O/kernel_stats.txt
