#!/bin/bash
# Is the device code of engine.hip the same as at another git revision?   tools/isa_same.sh <git-ref> [-DFLAG ...]
# Compiles engine.hip of <git-ref> (from a git archive, like tools/build_variant.sh) and of the working tree to gfx950 assembly under the same
# -cuid, and compares the two files byte by byte: every kernel, every .amdhsa_* resource line, in the same order.  Without flags it goes through
# the default build and the instrumented builds the tools use.  It compares and prints, nothing else; exit status 1 if any pair differs.
set -u
REF=${1:?usage: tools/isa_same.sh <git-ref> [-DFLAG ...]}; shift
ROOT=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
D=$(mktemp -d); trap 'rm -rf "$D"' EXIT
git -C "$ROOT" archive "$REF" gencore_amd/csrc include | tar -x -C "$D"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ $# -gt 0 ]; then SETS=("$*"); else
    SETS=("" "-DVB_PROF" "-DVB_PROF -DVB_COUNT" "-DVB_PROF -DDV_PROF" "-DVB_STOP=5" "-DCL_PROF" "-DPS_STOP=3" "-DGCE_SI_CANARY" "-DGCE_SI_CHECK")
fi
asm() { "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -cuid=isa_same $2 "$1/gencore_amd/csrc/engine.hip" -o "$3" 2> "$3.err" || { cat "$3.err"; return 1; }; }
bad=0; k=0
for FL in "${SETS[@]}"; do
    k=$((k + 1))
    asm "$D" "$FL" "$D/ref$k.s" & asm "$ROOT" "$FL" "$D/new$k.s" & wait
    if [ -s "$D/ref$k.s" ] && cmp -s "$D/ref$k.s" "$D/new$k.s"; then echo "identical  $(wc -c < "$D/new$k.s") bytes, $(wc -l < "$D/new$k.s") lines  [${FL:-default}]"
    else echo "DIFFERENT or not compiled  [${FL:-default}]"; bad=1; fi
done
exit $bad
