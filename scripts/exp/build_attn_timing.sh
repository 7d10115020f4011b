#!/bin/bash
# timing builds of the hand-scheduled attention forward: one libattn_timing_<tag>.so per argument.
# An argument is "<tag>" or "<tag>:<ARG,ARG,...>" (arguments of gen_attn_asm.py, e.g. "a7:--ahead=7,--defer"); tag "base" = no ablation; any other bare tag is an --ablate mode.
# With --ahead the dQ stream, which shares the forward's ring, is regenerated for the same value (the kernel checks that the two agree).
# TC_ATTN_TIMING=0 in the environment of this script builds without the s_memtime stamps (--timing).
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
for arg in "$@"; do
  v=${arg%%:*}; gargs=""
  [[ "$arg" == *:* ]] && gargs=$(echo "${arg#*:}" | tr ',' ' ')
  d=$(mktemp -d)
  cp $ROOT/transception_amd/csrc/*.hip $ROOT/transception_amd/csrc/*.h $ROOT/transception_amd/csrc/*.inc $ROOT/transception_amd/csrc/*.py $d/
  [[ "$arg" != *:* && $v != base ]] && gargs="--ablate $v"
  [[ "${TC_ATTN_TIMING:-1}" != 0 ]] && gargs="$gargs --timing"
  ( cd $d && { [[ -z "$gargs" ]] || { python gen_attn_asm.py $gargs --out variant.inc && mv variant.inc attn_fwd_asm.inc; }; } && \
    { ah=$(echo "$gargs" | grep -oE -- '--ahead[= ][0-9]+'); [[ -z "$ah" ]] || { python gen_dq_asm.py $ah --out variant.inc && mv variant.inc attn_dq_asm.inc; }; } && \
    sed -i 's|#include "../../include/transception_hip.h"|#include "'$ROOT'/include/transception_hip.h"|' tc_common.h && \
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=fast -munsafe-fp-atomics -o $ROOT/scripts/exp/libattn_timing_$v.so attention_seg.hip attention.hip; rm -rf $d ) 2>&1 | grep -v hip-link &
done
wait
