#!/usr/bin/env bash
# Builds libmarlsched.so (gfx950) in-tree: the HIP kernels + the C ABI.
# An object is rebuilt when the sha256 of its source, the headers it includes, the compiler
# version and the flags differs from the key stored beside it (not by mtime: a restored or
# copied tree keeps no trustworthy timestamps). MS_CLEAN=1 rebuilds everything.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${MS_OUT:-${HERE}/libmarlsched.so}"   # MS_OUT / MS_OBJDIR / MS_EXTRA_FLAGS: experiment variants (tools/)
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
ARCH="${MS_OFFLOAD_ARCH:-gfx950}"
FLAGS=(-O3 -std=c++17 -fPIC --offload-arch="${ARCH}" -Wall -Wno-unused-function
       -I"${HERE}/../include" ${MS_EXTRA_FLAGS:-})
OBJDIR="${MS_OBJDIR:-${HERE}/build}"
[[ "${MS_CLEAN:-0}" == 1 ]] && rm -rf "${OBJDIR}"
mkdir -p "${OBJDIR}"
HEADERS=("${HERE}"/csrc/*.h "${HERE}/../include/marlsched.h")  # every header: one missing here means stale objects
CCVER="$("${HIPCC}" --version 2>/dev/null | head -3 | tr '\n' ' ')"
objs=()
pids=()
for src in env_kernels.hip env_auct_kernels.hip acc_fill_kernels.hip policy_kernels.hip act_pair_kernels.hip greedy_kernels.hip evaluate_kernels.hip action_hist_kernels.hip action_table_kernels.hip returns_kernels.hip ppo_kernels.hip agg_kernels.hip dqn_kernels.hip bdqn_kernels.hip bdqn_update_kernels.hip wide_kernels.hip snapshot_kernels.hip capi.cpp; do
  obj="${OBJDIR}/${src%.*}.o"
  # the env round reproduces Python's float64 arithmetic: no contraction there; the policy
  # and PPO kernels follow torch's f32 (which fuses freely) within tolerance: fma allowed
  # (the action histogram and the action table count in integers only and keep the default)
  contract=(-ffp-contract=off)
  [[ "${src}" == policy_kernels.hip || "${src}" == act_pair_kernels.hip || "${src}" == greedy_kernels.hip || "${src}" == returns_kernels.hip ]] && contract=(-ffp-contract=fast)
  # the gradient kernel's variants (common rows by bytes or by owners) must agree bit for bit: fma only
  # where an expression asks for it, never across statements (fast contraction depends on the code around)
  [[ "${src}" == ppo_kernels.hip || "${src}" == bdqn_kernels.hip || "${src}" == wide_kernels.hip ]] && contract=(-ffp-contract=on)
  # the evaluation kernel (log-prob, value, entropy) takes the forward from the acting headers, which contract
  # freely under their own pragma and so round as k_act does; its own softmax tail and entropy sum fuse only where
  # an expression says so (on), so an output does not depend on which others the caller asked for
  [[ "${src}" == evaluate_kernels.hip ]] && contract=(-ffp-contract=on)
  # cfg3's paired acting kernel is a latency-bound chain: the ILP-first machine scheduler shortens it
  # (rollout 12.14 -> 11.88 ms, profiles/r3f2/ab_sched_ilp_act.txt); the env round gains nothing, and the
  # gradient, returns and the other acting kernels (k_act / k_act_common, cfg4) lose with it, so they keep the
  # default; each acting kernel is defined in one unit only (ms_act_kernels.h holds what the units share)
  [[ "${src}" == act_pair_kernels.hip && "${MS_NO_ILP:-0}" != 1 ]] && contract+=(-mllvm -amdgpu-sched-strategy=max-ilp)
  key="$( { cat "${HERE}/csrc/${src}" "${HEADERS[@]}"; echo "${CCVER} ${FLAGS[*]} ${contract[*]}"; } | sha256sum | cut -d' ' -f1)"
  if [[ ! -f "${obj}" || "$(cat "${obj}.key" 2>/dev/null)" != "${key}" ]]; then
    rm -f "${obj}.key"
    lang=()
    [[ "${src}" == *.cpp ]] && lang=(-x hip)
    # the objects compile in parallel; a key is written only after its object built
    ( "${HIPCC}" "${FLAGS[@]}" "${contract[@]}" "${lang[@]}" -c "${HERE}/csrc/${src}" -o "${obj}" &&
      echo "${key}" > "${obj}.key" ) &
    pids+=($!)
  fi
  objs+=("${obj}")
done
for p in "${pids[@]}"; do wait "${p}"; done
"${HIPCC}" -shared -fPIC --offload-arch="${ARCH}" -o "${OUT}" "${objs[@]}"
echo "${OUT}"
