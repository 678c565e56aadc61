#!/bin/bash
# Host-side AddressSanitizer build of every libisg source + the ABI driver, and of the
# executor's stream-order check:
#   tools/asan/build.sh [OUTDIR]       -> OUTDIR/abi_host_check, OUTDIR/exec_order_check
#                                         (default tools/asan/_build)
#   tools/asan/build.sh OUTDIR order   -> OUTDIR/exec_order_check only (no kernels: seconds)
# Device code is compiled normally (gfx950; GPU ASan is unavailable on this pool); only
# the host half is instrumented (-Xarch_host -fsanitize=address).
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
OUT=${1:-$HERE/_build}
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# the executor's stream-order check: exec.cpp and error.cpp host-only against the stubs; no
# kernel is compiled and no HIP runtime linked
mkdir -p "$OUT/order"
for s in "$ROOT"/instancesegmentation_amd/csrc/exec.cpp "$ROOT"/instancesegmentation_amd/csrc/error.cpp \
         "$HERE/exec_stubs.cpp" "$HERE/exec_order_check.cpp"; do
  $HIPCC -x hip --offload-host-only -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 \
    -std=c++17 -Wall -c "$s" -o "$OUT/order/$(basename "${s%.*}").o" &
done
wait
${CXX:-/opt/rocm/llvm/bin/clang++} -fsanitize=address,undefined -fno-gpu-sanitize -g "$OUT"/order/*.o -o "$OUT/exec_order_check"
[ "${2:-}" = order ] && exit 0
# device code at -O0: the checks run without a GPU and never execute it (optimising the
# device half of every kernel took most of a 7-minute build; 3 minutes now)
FLAGS="--offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer -Xarch_host -g -Xarch_host -O1 -Xarch_device -O0 -std=c++17"
objs=()
pids=()
for s in "$ROOT"/instancesegmentation_amd/csrc/*.hip "$ROOT"/instancesegmentation_amd/csrc/api.cpp \
         "$ROOT"/instancesegmentation_amd/csrc/error.cpp \
         "$ROOT"/instancesegmentation_amd/csrc/exec.cpp \
         "$HERE/abi_host_check.cpp"; do
  o="$OUT/$(basename "${s%.*}").o"
  objs+=("$o")
  stale=0
  if [ -f "$o" ]; then  # stale against its source and every header
    for d in "$s" "$ROOT"/instancesegmentation_amd/csrc/*.h "$ROOT/include/isg.h"; do
      [ "$o" -nt "$d" ] || stale=1
    done
    [ $stale = 1 ] || continue
  fi
  lang=""; case "$s" in *.cpp) lang="-x hip";; esac
  $HIPCC $FLAGS $lang -c "$s" -o "$o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
$HIPCC --offload-arch=gfx950 -Xarch_host -fsanitize=address -fno-gpu-sanitize -g "${objs[@]}" -o "$OUT/abi_host_check"
