#!/usr/bin/env bash
# Build libwm_hip.so for gfx950 (cross-compiles without a GPU).  Usage: csrc/build.sh
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# -pragma-unroll-threshold: the hand-scheduled MFMA loops (conv64bf3, resblock_eval) must unroll completely; above the default
# 16K-instruction limit the compiler silently unrolls by 2 and the register-resident weight fragments land in scratch memory
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -mllvm -pragma-unroll-threshold=100000 ${WM_EXTRA_FLAGS:-}"
mkdir -p obj
newest_hpp=$(ls -t *.hpp | head -n 1)            # every object depends on every header
pids=()
objs=()
# the one list of translation units (= the stems of *.hip): compiled from it, linked from it.  obj/ may hold objects of units
# that no longer exist (it is not under version control), so the link line never globs
for f in conv64_fwd conv64_k7 conv64_wgrad conv64_fp32 conv64_eval conv64_dwgrad bn small_convs lstm_fwd lstm_bwd lstm_grad postproc stft_loss losses gconv_fwd gconv_wgrad gconv_small lstm_seq resample biquad distort mdct_codec fir_rows time_warp wsola lpc_codec stoi splice clip_scores clip_features masking noise_suppress; do
  objs+=(obj/$f.o)
  if [ ! -f obj/$f.o ] || [ $f.hip -nt obj/$f.o ] || [ $newest_hpp -nt obj/$f.o ]; then
    $HIPCC $FLAGS -c $f.hip -o obj/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libwm_hip.so "${objs[@]}"
echo "built $(cd .. && pwd)/libwm_hip.so"
