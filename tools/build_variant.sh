#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags] [git rev of the sources, default: working tree]  ->  nudge_amd/_ab/lib<name>.so   (A/B builds for tests/gpu_ab_libs.py)
set -e
name=$1; extra=${2:-}; rev=${3:-}
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d /tmp/nhvar.XXXX)
mkdir -p $tmp/nudge_amd/csrc $tmp/include $root/nudge_amd/_ab
if [ -n "$rev" ]; then
  # every .hip and .h the revision has in nudge_amd/csrc (the file set differs from revision to revision)
  for f in $(git -C $root ls-tree --name-only $rev nudge_amd/csrc/ | grep -E '\.(hip|h)$'); do git -C $root show $rev:$f > $tmp/nudge_amd/csrc/$(basename $f); done
  git -C $root show $rev:include/nudge_hip.h > $tmp/include/nudge_hip.h
else
  cp $root/nudge_amd/csrc/*.hip $root/nudge_amd/csrc/*.h $tmp/nudge_amd/csrc/; cp $root/include/nudge_hip.h $tmp/include/
fi
cd $tmp/nudge_amd/csrc
if [ -n "$NH_VARIANT_PATCH" ]; then python $root/$NH_VARIANT_PATCH nh_solve.hip nh_solve.patched && mv nh_solve.patched nh_solve.hip; fi
for f in *.hip; do
  /opt/rocm/bin/hipcc $extra -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -fPIC -w -c $f -o ${f%.hip}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC *.o -o $root/nudge_amd/_ab/lib$name.so
rm -rf $tmp
ls -la $root/nudge_amd/_ab/lib$name.so
