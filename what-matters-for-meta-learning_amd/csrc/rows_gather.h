// Row gather for cached contexts that are joined or regrouped across states: ONE launch fills the per-shot rows of
// up to 2 row sets of a new state from the rows of up to 8 source states that share one plan.
//
//   dst_i[t][s][:] = (0 <= ps < nsrc and 0 <= pr < rows[ps]) ? src_{ps,i}[pr][:] : 0      (ps, pr) = plan[t][s]
//                                                              row sets i = 0 .. sets - 1, fp32 rows of W_i floats, dst_i [T][cap][W_i]
//
// Source j is a flat list of rows[j] = T_j cap_j rows per set; the sources may differ in T_j and cap_j, the kernel needs rows[j] for
// the bound alone.  plan [T][cap][2] (int32, DEVICE memory) names (source, flat row in it) of every destination slot; a source
// outside 0 .. nsrc - 1 or a row outside 0 .. rows[ps] - 1 - (-1, -1) is the fill - gives a row of exact zeros and no source is read
// for it, so every index stays in bounds whatever arrives.  The selection is by index, never a product with a mask: a NaN or Inf in
// a row that no plan entry names does not reach dst.  One source row may be named by any number of destination rows.  EVERY row of
// dst is written.
//
// The kernel is rc::compact_kernel's stream (csrc/rows_compact.h).  Per task the rows of all sets lie side by side as one list of
// float4 slots - slot q is row q / w4, column q % w4, w4 = sum_i W_i / 4, and the column says which set it belongs to - and a
// workgroup owns RG_U * 256 consecutive slots of one task: a lane issues its RG_U plan reads (one 8-byte load each) and its RG_U
// loads, then its RG_U stores (float4, global_load / global_store_dwordx4).  The source of a slot is found by a compare chain over
// the NSRC descriptors of the kernel arguments.  Every argument is read ONCE per workgroup, by a scalar load at a constant offset,
// and passed through scalar_arg(), which hides the load from the optimiser: left to itself it turns `lane ? a.src[1][k] :
// a.src[0][k]` into a VECTOR load from the kernel-argument segment through a chosen address - NSRC dependent loads per slot between
// the plan read and the row read.  Behind scalar_arg the chain carries the pointers of BOTH sets as values (v_cndmask) and the set
// is chosen at the end: the arguments are never indexed by a lane's value, nothing goes to scratch, and the code of every
// instantiation holds exactly RG_U 8-byte loads, RG_U float4 loads and RG_U float4 stores.  NSRC is nsrc rounded up to 1, 2, 4 or
// 8; the descriptors behind nsrc hold rows = 0 and match nothing.  Grid (ceil(cap w4 / (256 RG_U)), min(T, 65535)).  No LDS, no
// atomics, nothing exchanged between workgroups; dst overlaps no src (the entry refuses it).
#pragma once
#include "common.h"

namespace mlhot {

constexpr int ROWS_GATHER_MAX_SETS = 2;
constexpr int ROWS_GATHER_MAX_SRC = 8;
constexpr int ROWS_GATHER_MAX_CAP = 4096;

#ifndef MLHOT_HOSTSIM
namespace rg {

constexpr int RG_U = 4;                   // float4 slots per lane

struct Args {
  const float* src[ROWS_GATHER_MAX_SETS][ROWS_GATHER_MAX_SRC];
  int rows[ROWS_GATHER_MAX_SRC];          // rows per set of each source; 0 behind nsrc
  float* dst[ROWS_GATHER_MAX_SETS];
  int w4[ROWS_GATHER_MAX_SETS];           // float4 slots per row of each set
  const int2* plan;
  int T, cap;
  unsigned wtot4, n4;                     // float4 slots per row over all sets, and per task (cap wtot4 < 2^31)
};

typedef float f4v __attribute__((ext_vector_type(4)));          // 16 bytes as a builtin vector: it may carry an address space
typedef __attribute__((address_space(1))) f4v gfloat4;         // ... global memory: behind scalar_arg the address space is stated, not inferred

// A kernel argument as a value in scalar registers that the compiler cannot trace back to its load: a choice between two such
// values by a lane's condition stays a v_cndmask of the values and cannot be turned into one load through a chosen address.
template <typename V>
__device__ __forceinline__ V scalar_arg(V v) {
  asm volatile("" : "+s"(v));
  return v;
}

template <int SETS, int NSRC>
__global__ __launch_bounds__(256) void gather_kernel(const Args a) {
  const float* src[SETS][NSRC];
  int rows[NSRC];
  float* dst[SETS];
  int w4s[SETS];
#pragma unroll
  for (int i = 0; i < SETS; ++i) {          // constant indices: scalar loads, once per workgroup
    dst[i] = scalar_arg(a.dst[i]);
    w4s[i] = scalar_arg(a.w4[i]);
#pragma unroll
    for (int k = 0; k < NSRC; ++k) src[i][k] = scalar_arg(a.src[i][k]);
  }
#pragma unroll
  for (int k = 0; k < NSRC; ++k) rows[k] = scalar_arg(a.rows[k]);
  const unsigned q0 = blockIdx.x * (256u * RG_U) + threadIdx.x;
  for (int t = blockIdx.y; t < a.T; t += gridDim.y) {
    const int2* plan = a.plan + (size_t)t * a.cap;
    int2 p[RG_U];
    unsigned row[RG_U];
#pragma unroll
    for (int u = 0; u < RG_U; ++u) {        // the plan reads, all in flight before the first is used
      const unsigned q = q0 + 256u * u;
      row[u] = q / a.wtot4;
      p[u] = q < a.n4 ? plan[row[u]] : int2{-1, -1};
    }
    f4v x[RG_U];
    gfloat4* to[RG_U];                      // the slot's place in its dst, nullptr behind the task's last slot
#pragma unroll
    for (int u = 0; u < RG_U; ++u) {
      const unsigned q = q0 + 256u * u;
      x[u] = f4v{0.f, 0.f, 0.f, 0.f};
      to[u] = nullptr;
      if (q >= a.n4) continue;
      int col = (int)(q - row[u] * a.wtot4);
      const bool second = SETS > 1 && col >= w4s[0];      // two sets at most: the column is behind the first set's width or not
      // the source's pointer of BOTH sets through the compare chain (k is a constant after unrolling), the set chosen at the end
      const float* sp[SETS];
#pragma unroll
      for (int i = 0; i < SETS; ++i) sp[i] = nullptr;
#pragma unroll
      for (int k = 0; k < NSRC; ++k) {
        const bool hit = p[u].x == k && p[u].y >= 0 && p[u].y < rows[k];
#pragma unroll
        for (int i = 0; i < SETS; ++i) sp[i] = hit ? src[i][k] : sp[i];
      }
      if (second) col -= w4s[0];
      const int w4 = second ? w4s[SETS - 1] : w4s[0];
      float* dp = second ? dst[SETS - 1] : dst[0];
      const float* from = second ? sp[SETS - 1] : sp[0];
      to[u] = (gfloat4*)dp + ((size_t)t * a.cap + row[u]) * w4 + col;
      if (from) x[u] = ((const gfloat4*)from)[(size_t)p[u].y * w4 + col];
    }
#pragma unroll
    for (int u = 0; u < RG_U; ++u)
      if (to[u]) *to[u] = x[u];
  }
}

template <int SETS>
inline void launch(int nsrc, dim3 grid, hipStream_t s, const Args& a) {
  if (nsrc <= 1) hipLaunchKernelGGL((gather_kernel<SETS, 1>), grid, dim3(256), 0, s, a);
  else if (nsrc <= 2) hipLaunchKernelGGL((gather_kernel<SETS, 2>), grid, dim3(256), 0, s, a);
  else if (nsrc <= 4) hipLaunchKernelGGL((gather_kernel<SETS, 4>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gather_kernel<SETS, 8>), grid, dim3(256), 0, s, a);
}

}  // namespace rg
#endif

// src: sets * nsrc entries, src[i * nsrc + j] = set i of source j; rows: nsrc entries; dst, W: `sets` entries - all in HOST memory;
// plan in DEVICE memory
inline int rows_gather(const float* const* src, const int64_t* rows, int nsrc, float* const* dst, const int* W, int sets, const int32_t* plan,
                       int T, int cap, hipStream_t s) {
  if (!src || !rows || !dst || !W || !plan || T <= 0) { set_error("rows_gather: bad argument"); return MLHOT_ERR_ARG; }
  const int ns = nsrc < ROWS_GATHER_MAX_SRC ? nsrc : ROWS_GATHER_MAX_SRC, nt = sets < ROWS_GATHER_MAX_SETS ? sets : ROWS_GATHER_MAX_SETS;
  for (int i = 0; i < nt; ++i) {
    if (!dst[i] || W[i] <= 0) { set_error("rows_gather: set %d has a NULL dst or no width", i); return MLHOT_ERR_ARG; }
    for (int j = 0; j < ns; ++j)
      if (!src[(size_t)i * nsrc + j] || rows[j] <= 0) { set_error("rows_gather: set %d of source %d is NULL or has no rows", i, j); return MLHOT_ERR_ARG; }
  }
#ifdef MLHOT_HOSTSIM
  (void)s; (void)cap; set_error("rows_gather: GPU build only"); return MLHOT_ERR_UNSUPPORTED;
#else
  bool ok = sets >= 1 && sets <= ROWS_GATHER_MAX_SETS && nsrc >= 1 && nsrc <= ROWS_GATHER_MAX_SRC && cap >= 1 && cap <= ROWS_GATHER_MAX_CAP &&
            (reinterpret_cast<uintptr_t>(plan) & 7) == 0;
  long long wtot4 = 0, rmax = 0;
  for (int i = 0; ok && i < sets; ++i) {
    ok = W[i] % 4 == 0 && (reinterpret_cast<uintptr_t>(dst[i]) & 15) == 0;
    for (int j = 0; ok && j < nsrc; ++j) ok = (reinterpret_cast<uintptr_t>(src[(size_t)i * nsrc + j]) & 15) == 0;
    wtot4 += W[i] / 4;
  }
  for (int j = 0; ok && j < nsrc; ++j) {
    if (rows[j] > rmax) rmax = rows[j];
    ok = rows[j] < (1ll << 31);
  }
  if (ok && wtot4 * cap >= (1ll << 31)) ok = false;
  if (!ok) {
    set_error("rows_gather serves 1 .. 2 row sets of W %% 4 == 0 floats from 1 .. 8 sources of fewer than 2^31 rows, 16-byte aligned pointers, "
              "1 <= cap <= 4096 and fewer than 2^31 float4 per task (sets=%d nsrc=%d cap=%d W=%d,%d largest source %lld rows)", sets, nsrc, cap,
              sets >= 1 ? W[0] : 0, sets >= 2 ? W[1] : 0, rmax);
    return MLHOT_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < sets; ++i) {
    const char* d0 = (const char*)dst[i];
    const size_t db = (size_t)T * cap * W[i] * sizeof(float);
    for (int k = 0; k < sets; ++k) {
      for (int j = 0; j < nsrc; ++j) {
        const char* s0 = (const char*)src[(size_t)k * nsrc + j];
        const size_t sb = (size_t)rows[j] * W[k] * sizeof(float);
        if (s0 < d0 + db && d0 < s0 + sb) {
          set_error("rows_gather: dst %d overlaps set %d of source %d; the gathered rows need their own buffer", i, k, j);
          return MLHOT_ERR_ARG;
        }
      }
      const char* e0 = (const char*)dst[k];
      const size_t eb = (size_t)T * cap * W[k] * sizeof(float);
      if (k != i && e0 < d0 + db && d0 < e0 + eb) { set_error("rows_gather: dst %d overlaps dst %d", i, k); return MLHOT_ERR_ARG; }
    }
  }
  rg::Args a{};
  for (int i = 0; i < ROWS_GATHER_MAX_SETS; ++i) {       // the slots behind `sets` and `nsrc` are never read through: rows = 0 matches nothing
    const int k = i < sets ? i : 0;
    a.dst[i] = dst[k]; a.w4[i] = W[k] / 4;
    for (int j = 0; j < ROWS_GATHER_MAX_SRC; ++j) a.src[i][j] = src[(size_t)k * nsrc + (j < nsrc ? j : 0)];
  }
  for (int j = 0; j < ROWS_GATHER_MAX_SRC; ++j) a.rows[j] = j < nsrc ? (int)rows[j] : 0;
  a.plan = reinterpret_cast<const int2*>(plan); a.T = T; a.cap = cap; a.wtot4 = (unsigned)wtot4; a.n4 = (unsigned)(wtot4 * cap);
  ProfScope ps("rows.gather", s);
  const dim3 grid((a.n4 + 256u * rg::RG_U - 1) / (256u * rg::RG_U), (unsigned)(T < 65535 ? T : 65535));
  if (sets == 1) rg::launch<1>(nsrc, grid, s, a);
  else rg::launch<2>(nsrc, grid, s, a);
  return check_launch("rows.gather");
#endif
}

}  // namespace mlhot
