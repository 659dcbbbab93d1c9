#!/bin/bash
# usage: scripts/prof_bench.sh <tag> [out_dir]  -- untraced bench line + rocprofv3 kernel trace of the whole bench (--full), from the repo root on a machine with an MI355X;
# the files go to out_dir (default: prof_out/ in the repo root)
tag=$1
R=${GRAFT_REPO_ROOT:-$(pwd)}
out=$(realpath -m "${2:-$R/prof_out}")
mkdir -p "$out"
cd $R
python bench.py --full --no-cpu-baseline > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$tag -- python $R/bench.py --full --no-cpu-baseline > "$out/${tag}_bench_traced.json" 2> "$out/${tag}_prof.err"
f=$(find /tmp/prof_$tag -name "*kernel_stats.csv" | head -1)
python - "$f" > "$out/${tag}_kernel_stats.csv" <<'P'
import sys, csv
rows = list(csv.reader(open(sys.argv[1])))
print(",".join('"%s"' % c for c in rows[0]))
for r in rows[1:]:
    if r[0].startswith(("gf", "void gf")):
        print(",".join('"%s"' % c for c in r))
P
