#!/bin/bash
# Host-side sanitizer run of an entry's refusal paths: the library's translation units and ONE stand-alone host program with
# its own main (tools/register_batch_refusals.cpp: rrl_se3_adam_step_batch / rrl_register_epoch; tools/register_newton_refusals.cpp:
# rrl_pose_normal_eq / rrl_se3_newton_step_batch / rrl_register_newton_epoch) compiled with AddressSanitizer + UBSan on the
# HOST side only (the device code is compiled as always and never runs: every call is refused before a launch), linked, run.
# Needs hipcc, no GPU.  usage (repo root): tools/refusals_sanitize.sh <program.cpp> [build dir]
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
PROG=$(realpath "${1:?usage: tools/refusals_sanitize.sh <program.cpp> [build dir]}")
OUT=${2:-$(mktemp -d)}
mkdir -p "$OUT"
HIPCC=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -g"
FLAGS="--offload-arch=gfx950 -O1 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function"
cd "$R/a-robust-registration-loss_amd/csrc"
ls *.hip | xargs -P 8 -I{} sh -c "$HIPCC $FLAGS $SAN \$( [ {} = rrl_cull.hip ] && echo -fno-slp-vectorize ) -c {} -o $OUT/{}.o"
$HIPCC $FLAGS $SAN -I"$R/include" -x hip -c "$PROG" -o "$OUT/refusals.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT"/*.o -o "$OUT/refusals" -ldl
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/refusals"
