// Row compaction for cached contexts that let shots go: ONE launch moves the per-shot rows of up to 4 row sets that
// share one plan.
//
//   dst_i[t][s][:] = plan[t][s] >= 0 ? src_i[t][plan[t][s]][:] : 0          row sets i = 0 .. sets - 1, fp32 rows of W_i floats in [T][cap][W_i]
//
// plan [T][cap] (int32, DEVICE memory) names the source slot of every destination slot, -1 = "a row of exact zeros, src is not read".
// A value outside -1 .. cap - 1 is held to -1, so every index stays in bounds whatever arrives.  The selection is by index, never a
// product with a mask: a NaN or Inf in a row that no plan entry names does not reach dst.  EVERY row of dst is written.
//
// The kernel is a stream.  Per task the rows of all sets lie side by side as one list of float4 slots - slot q is row q / w4, column
// q % w4, w4 = sum_i W_i / 4, and the column says which set it belongs to - and a workgroup owns RC_U * 256 consecutive slots of one
// task: a lane issues its RC_U plan reads and its RC_U loads, then its RC_U stores (float4, global_load / global_store_dwordx4).
// Grid (ceil(cap w4 / (256 RC_U)), min(T, 65535)): the 4096-slot, W = 2048 case is 2048 workgroups per task, cap = 1 is one workgroup
// per task.  No LDS, no atomics, nothing exchanged between workgroups; dst overlaps no src (the entry refuses it).
#pragma once
#include "common.h"

namespace mlhot {

constexpr int ROWS_COMPACT_MAX_SETS = 4;
constexpr int ROWS_COMPACT_MAX_CAP = 4096;

#ifndef MLHOT_HOSTSIM
namespace rc {

constexpr int RC_U = 4;                   // float4 slots per lane

struct Args {
  const float* src[ROWS_COMPACT_MAX_SETS];
  float* dst[ROWS_COMPACT_MAX_SETS];
  int w4[ROWS_COMPACT_MAX_SETS];          // float4 slots per row of each set
  const int32_t* plan;
  int T, cap;
  unsigned wtot4, n4;                     // float4 slots per row over all sets, and per task (cap wtot4 < 2^31)
};

template <int SETS>
__global__ __launch_bounds__(256) void compact_kernel(const Args a) {
  const unsigned q0 = blockIdx.x * (256u * RC_U) + threadIdx.x;
  for (int t = blockIdx.y; t < a.T; t += gridDim.y) {
    const int32_t* plan = a.plan + (size_t)t * a.cap;
    float4 x[RC_U];
    float4* to[RC_U];                     // the slot's place in its dst, nullptr behind the task's last slot
#pragma unroll
    for (int u = 0; u < RC_U; ++u) {
      const unsigned q = q0 + 256u * u;
      x[u] = float4{0.f, 0.f, 0.f, 0.f};
      to[u] = nullptr;
      if (q >= a.n4) continue;
      const unsigned row = q / a.wtot4;
      // the set of the column: the widths in front are taken off one by one (k is a constant after unrolling: the kernel arguments
      // are never indexed by a lane's value)
      int col = (int)(q - row * a.wtot4), w4 = a.w4[0];
      const float* sp = a.src[0];
      float* dp = a.dst[0];
      bool found = false;
#pragma unroll
      for (int k = 1; k < SETS; ++k) {
        if (!found && col >= w4) { col -= w4; w4 = a.w4[k]; sp = a.src[k]; dp = a.dst[k]; }
        else found = true;
      }
      const int p = plan[row];
      to[u] = reinterpret_cast<float4*>(dp) + ((size_t)t * a.cap + row) * w4 + col;
      if (p >= 0 && p < a.cap) x[u] = reinterpret_cast<const float4*>(sp)[((size_t)t * a.cap + p) * w4 + col];
    }
#pragma unroll
    for (int u = 0; u < RC_U; ++u)
      if (to[u]) *to[u] = x[u];
  }
}

}  // namespace rc
#endif

// src, dst, W: `sets` entries each, in HOST memory; plan in DEVICE memory
inline int rows_compact(const float* const* src, float* const* dst, const int* W, int sets, const int32_t* plan, int T, int cap, hipStream_t s) {
  if (!src || !dst || !W || !plan || T <= 0 || cap <= 0 || sets <= 0) { set_error("rows_compact: bad argument"); return MLHOT_ERR_ARG; }
  for (int i = 0; i < sets && i < ROWS_COMPACT_MAX_SETS; ++i)
    if (!src[i] || !dst[i] || W[i] <= 0) { set_error("rows_compact: set %d has a NULL pointer or no width", i); return MLHOT_ERR_ARG; }
#ifdef MLHOT_HOSTSIM
  (void)s; set_error("rows_compact: GPU build only"); return MLHOT_ERR_UNSUPPORTED;
#else
  bool ok = sets <= ROWS_COMPACT_MAX_SETS && cap <= ROWS_COMPACT_MAX_CAP && (reinterpret_cast<uintptr_t>(plan) & 3) == 0;
  long long wtot4 = 0;
  for (int i = 0; ok && i < sets; ++i) {
    ok = W[i] % 4 == 0 && (reinterpret_cast<uintptr_t>(src[i]) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst[i]) & 15) == 0;
    wtot4 += W[i] / 4;
  }
  if (ok && wtot4 * cap >= (1ll << 31)) ok = false;
  if (!ok) {
    set_error("rows_compact serves 1 .. 4 row sets of W %% 4 == 0 floats, 16-byte aligned pointers, 1 <= cap <= 4096 and fewer than 2^31 float4 per "
              "task (sets=%d cap=%d)", sets, cap);
    return MLHOT_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < sets; ++i) {
    const char* d0 = (const char*)dst[i];
    const size_t db = (size_t)T * cap * W[i] * sizeof(float);
    for (int j = 0; j < sets; ++j) {
      const char* s0 = (const char*)src[j];
      const size_t sb = (size_t)T * cap * W[j] * sizeof(float);
      if (s0 < d0 + db && d0 < s0 + sb) { set_error("rows_compact: dst %d overlaps src %d; the compacted rows need their own buffer", i, j); return MLHOT_ERR_ARG; }
      const char* e0 = (const char*)dst[j];
      if (j != i && e0 < d0 + db && d0 < e0 + sb) { set_error("rows_compact: dst %d overlaps dst %d", i, j); return MLHOT_ERR_ARG; }
    }
  }
  rc::Args a{};
  for (int i = 0; i < ROWS_COMPACT_MAX_SETS; ++i) {      // the slots behind `sets` are never looked up
    const int k = i < sets ? i : 0;
    a.src[i] = src[k]; a.dst[i] = dst[k]; a.w4[i] = W[k] / 4;
  }
  a.plan = plan; a.T = T; a.cap = cap; a.wtot4 = (unsigned)wtot4; a.n4 = (unsigned)(wtot4 * cap);
  ProfScope ps("rows.compact", s);
  const dim3 grid((a.n4 + 256u * rc::RC_U - 1) / (256u * rc::RC_U), (unsigned)(T < 65535 ? T : 65535));
  switch (sets) {
    case 1: hipLaunchKernelGGL((rc::compact_kernel<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((rc::compact_kernel<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((rc::compact_kernel<3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((rc::compact_kernel<4>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch("rows.compact");
#endif
}

}  // namespace mlhot
