#!/bin/bash
# Instruction count and a hash of the instruction stream of every kernel of one translation unit, from the compiler's assembly (no GPU needed).
# Two revisions whose lines agree compile to the same instructions; it prints what it finds and looks for nothing.
#   tools/kernel_isa.sh [nh_solve.hip | nh_collide.hip | ... , default nh_solve.hip] [name-filter]      ->  <instructions> <md5 of them> <kernel, by its symbol like kernel_resources.sh>
# KEEP=<dir> keeps each kernel's hashed lines there as <dir>/<symbol, first 200 characters>.isa, for a diff between two revisions.
# Hashed are the instruction lines alone: directives, comments and the numbers of the .LBB labels are dropped (they move with unrelated code).
cd "$(dirname "$0")/../nudge_amd/csrc" || exit 1
src=${1:-nh_solve.hip}; filt=${2:-.}
tmp=$(mktemp -d /tmp/nhisa.XXXX) || exit 1
trap 'rm -rf "$tmp"' EXIT
/opt/rocm/bin/hipcc $EXTRA -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -fPIC -w --cuda-device-only -S "$src" -o "$tmp/unit.s" || exit 1
awk -v dir="$tmp" '
  /^[ \t]*\.type[ \t].*@function/ { name=$2; sub(/,.*/,"",name); ++nr; print name > (dir "/" nr ".name"); next }
  /^\.Lfunc_end/ { name=""; next }
  name == "" { next }
  { line=$0; sub(/[ \t]*;.*/,"",line); sub(/^[ \t]+/,"",line) }
  line == "" || line ~ /^\./ || line ~ /:$/ { next }
  { gsub(/\.LBB[0-9]+_[0-9]+/,".LBB",line); print line > (dir "/" nr ".isa") }' "$tmp/unit.s"
for f in "$tmp"/*.isa; do
  [ -e "$f" ] || continue
  [ -n "$KEEP" ] && mkdir -p "$KEEP" && cp "$f" "$KEEP/$(cut -c1-200 "${f%.isa}.name").isa"
  echo "$(wc -l < "$f") $(md5sum < "$f" | cut -c1-32) $(cat "${f%.isa}.name")"
done | awk -v f="$filt" '{ n=$0; sub(/^[0-9]+ [0-9a-f]+ /,"",n) } n ~ f' | sort -k3
