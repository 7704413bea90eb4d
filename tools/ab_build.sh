#!/bin/bash
# A/B libraries with the product's own flags (__graft_entry__.HIPCC_FLAGS):
#   tools/ab_build.sh <tag> [--src DIR] [-DNAME=v ...]  ->  tools/_ab/lib_<tag>.so of this tree
# --src DIR builds the sources of another checkout (default: this tree), e.g. of the parent commit, into this tree's
# tools/_ab next to the others; tools/ab_run.sh runs them.
set -o pipefail
tag=$1; shift
here=$(cd "$(dirname "$0")/.." && pwd)
src=$here
if [ "$1" = "--src" ]; then src=$(cd "$2" && pwd) || exit 1; shift 2; fi
out=$here/tools/_ab
mkdir -p "$out"
flags=$(cd "$here" && python3 -c "import __graft_entry__ as g; print(' '.join(g.HIPCC_FLAGS))") || exit 1
cd "$src/grasptrajopt_amd/csrc" || exit 1
${HIPCC:-/opt/rocm/bin/hipcc} $flags "$@" -Rpass-analysis=kernel-resource-usage gto_api.hip -o "$out/lib_$tag.so" 2> "$out/lib_$tag.remarks" \
  || { grep -v "remark:" "$out/lib_$tag.remarks" | tail -20; exit 1; }
python3 - "$out/lib_$tag.remarks" <<'P'
import re,sys
rows=[];
for line in open(sys.argv[1]):
    m=re.search(r"Function Name: (\S+)",line)
    if m: rows.append({"name":m.group(1)}); continue
    m=re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)",line)
    if m and rows: rows[-1][m.group(1).split(" ")[0]]=int(m.group(2))
for r in rows:
    if any(k in r["name"] for k in ("k_obstacle_gramILi8ELi1ELb0ELb1","k_obstacle_gramILi16ELi1ELb0ELb1","k_lm_stepILi4","k_lm_stepILi8","k_lm_step_wide")):
        print(" ", r)
P
echo "$out/lib_$tag.so"
