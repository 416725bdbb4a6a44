#!/bin/bash
# build a variant library: build_variant.sh NAME "-DFLAG ..." file.hip [file2.hip ...]  ->  csrc/libddpm_hip_NAME.so (the named sources rebuilt with the flags, the other objects reused)
# The source list and the compiler flags are those of csrc/build.py.
set -e
cd "$(dirname "$0")/../ddpm-torch_amd/csrc"
name=$1; flags=$2; shift 2
sources=$(python3 -c 'import build; print(" ".join(s[:-4] for s in build.SOURCES))')
base=$(python3 -c 'import build; print(" ".join(build.FLAGS))')
objs=""
for s in $sources; do
  if [[ " $* " == *" $s.hip "* ]]; then
    /opt/rocm/bin/hipcc $base $flags -c $s.hip -o /tmp/${s}_$name.o
    objs="$objs /tmp/${s}_$name.o"
  else objs="$objs $s.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libddpm_hip_$name.so $objs
echo built libddpm_hip_$name.so
