// Shared targets against per-shot key states: ONE set of query rows q [Nq][H][d] asked of all T stored contexts.
//
// The FAVOR+ query features F_q = ratio (exp(dd_q - diag_q - rowmax) + 1e-4) read the query row, proj and the row's own maximum
// (ft::query_front) - nothing of the task.  The per-task query kernels (favor_cached.h, favor_long.h) form them once per (task, head,
// 16-row tile); with the same rows under every task that is T times the dominant work of a tile (16 m d MACs against 16 Nc m for S).
// Here a workgroup owns one (head, 16-row target tile) and a contiguous GROUP of tasks:
//   1. ft::query_front once; F_q stays in LDS
//   2. per task t of its group, the per-task kernel's own steps against that task's F_k, lens[t] and v:
//        cached  ft::s_tile, ft::s_rowsum, the w store, ft::sv_tiles                      (fc::query_body's steps 4. and 5.)
//        long    per 32-slot chunk ft::s_tile and the copy into the wide tile, ft::s_rowsum_wide, the w store, ft::sv_tiles_wide
//                                                                                          (fl2::query_body's)
//   3. out [T][Nq][d H] and w [T][H][Nq][Nc] by vector stores; no atomics, no workspace
// The steps are favor_tile.h's text with the per-task kernel's arguments, so out and w have the BITS of mlhot_favor_query_fwd /
// _weights_fwd / _long_fwd on q expanded to [T][Nq][H][d].  The task-group size only decides which workgroup walks which tasks - a
// task's sums never see another task's - so the bits do not depend on it, and the row invariance of the per-task kernels carries over.
// Between two tasks of a group no barrier is added: ft::s_tile's first barrier stands between the last reads of the S tile, the wide
// tile and D by task t (the w store, the S V chains) and their first writes for task t + 1, which all lie behind it.
// LDS is the per-task kernels' own - F_q was resident between the two passes there as well: 124 KB (cached) and 140 KB (long) of
// gfx950's 160 KB, one workgroup per CU.  What the group buys is steps 1. once instead of once per task.
#pragma once
#include "common.h"
#include "favor_tile.h"
#include "favor_cached.h"
#include "favor_long.h"

namespace mlhot {

#ifndef MLHOT_HOSTSIM
namespace fsh {

using ft::QT;
constexpr int CU_TARGET = 256;            // workgroups the host aims at with task_group == 0: the MI355X's CUs, one workgroup each

struct Args {
  const float *q, *proj, *fk, *v;
  const int32_t* lens;                    // long: [T] on the device, or nullptr; cached: unused (a masked slot is a zero row of F_k)
  float *out, *w;                         // w nullptr: no read-out
  int T, H, Nq, Nc, d, m, mp, ntile, tg;  // tg: tasks per group
  ft::Scales sc;
};

// blockIdx.x = (group * H + head) * ntile + tile
template <bool WOUT>
__device__ __forceinline__ void cached_body(const Args& a) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int gh = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, grp = gh / a.H, h = gh % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  ft::query_front([&](int r) { return n0 + r < Nq ? a.q + ((size_t)(n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const int t1 = min(a.T, (grp + 1) * a.tg);
  for (int t = grp * a.tg; t < t1; ++t) {
    const int th = t * H + h;
    const float* krow[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + ((size_t)th * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
    ft::s_tile(s_f, ft::ldf(mp), krow, (Nc + 15) / 16, mp / 16, Nc, ft::BPlain{}, red, s_S);
    ft::s_rowsum(s_S, Nc, s_D);
    if constexpr (WOUT) {
      float* wt = a.w + ((size_t)th * Nq + n0) * Nc;
      const int lim = min(QT, Nq - n0) * Nc;
      for (int idx = tid; idx < lim; idx += 256) {
        const int row = idx / Nc, np = idx - row * Nc;
        wt[idx] = s_S[row * ft::LDS_S + np] / s_D[row];
      }
    }
    ft::sv_tiles(s_S, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, d, wv, lr, lq, [&](int row, int e, float o) {
      const int n = n0 + row;
      if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
    });
  }
}

template <bool WOUT>
__device__ __forceinline__ void long_body(const Args& a) {
  constexpr int CH = fl2::CH, LDW = fl2::LDW;
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int gh = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, grp = gh / a.H, h = gh % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  ft::query_front([&](int r) { return n0 + r < Nq ? a.q + ((size_t)(n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const int t1 = min(a.T, (grp + 1) * a.tg);
  for (int t = grp * a.tg; t < t1; ++t) {
    const int th = t * H + h;
    const int need = ft::clamp_len(a.lens, t, 1, Nc);
    for (int c0 = 0; c0 < need; c0 += CH) {
      const int ncol = min(CH, need - c0);
      const float* krow[2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < ncol ? a.fk + ((size_t)th * Nc + c0 + 16 * jj + lr) * mp + 4 * lq : nullptr;
      ft::s_tile(s_f, ft::ldf(mp), krow, (ncol + 15) / 16, mp / 16, ncol, ft::BPlain{}, red, s_S);
      for (int idx = tid; idx < QT * CH; idx += 256) {
        const int row = idx / CH, np = idx - row * CH;
        if (np < ncol) s_W[row * LDW + c0 + np] = s_S[row * ft::LDS_S + np];
      }
    }
    __syncthreads();
    ft::s_rowsum_wide(s_W, LDW, need, s_D);
    if constexpr (WOUT) {
      float* wt = a.w + ((size_t)th * Nq + n0) * Nc;
      const int lim = min(QT, Nq - n0) * Nc;
      for (int idx = tid; idx < lim; idx += 256) {
        const int row = idx / Nc, np = idx - row * Nc;
        wt[idx] = np < need ? s_W[row * LDW + np] / s_D[row] : 0.f;
      }
    }
    ft::sv_tiles_wide(s_W, LDW, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, need, d, wv, lr, lq, [&](int row, int e, float o) {
      const int n = n0 + row;
      if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
    });
  }
}

__global__ __launch_bounds__(256) void cached_kernel(const Args a) { cached_body<false>(a); }
__global__ __launch_bounds__(256) void cached_weights_kernel(const Args a) { cached_body<true>(a); }
__global__ __launch_bounds__(256) void long_kernel(const Args a) { long_body<false>(a); }
__global__ __launch_bounds__(256) void long_weights_kernel(const Args a) { long_body<true>(a); }

// tasks per group: the caller's (held to 1 .. T), or with 0 the size at which (groups x H x tiles) covers CU_TARGET about once
inline int tasks_per_group(int task_group, int T, int H, long long ntile) {
  if (task_group > 0) return task_group < T ? task_group : T;
  const long long base = (long long)H * ntile;
  long long groups = (CU_TARGET + base - 1) / base;
  if (groups < 1) groups = 1;
  if (groups > T) groups = T;
  return (int)((T + groups - 1) / groups);
}

}  // namespace fsh
#endif

constexpr size_t FAVOR_SHARED_QUERY_WS = 256;     // the kernels work in LDS alone; ws is favor_query_fwd's token block

inline size_t favor_query_shared_ws_need(int T, int H, int Nq, int Nc, int d, int m) {
  return Nq >= 1 && favor_cached_ok(T, H, Nc, d, m) ? FAVOR_SHARED_QUERY_WS : 0;
}
inline size_t favor_query_long_shared_ws_need(int T, int H, int Nq, int Nc, int d, int m) {
  return Nq >= 1 && favor_long_ok(T, H, Nc, d, m) ? FAVOR_SHARED_QUERY_WS : 0;
}

// mlhot_favor_query_shared_fwd (wide == false: a mlhot_favor_keys_fwd / _ragged_fwd state, Nc <= 32, lens unused) and
// mlhot_favor_query_long_shared_fwd (wide: a mlhot_favor_keys_long_fwd state, Nc <= 256, the state's lens or nullptr).  q [Nq][H][d] is
// shared by the T tasks; out [T][Nq][d H]; w [T][H][Nq][Nc] or nullptr (no read-out).  Envelope, alignment rules and codes are the
// per-task entries'.
inline int favor_query_shared_launch(const char* what, bool wide, const float* q, const void* state, const float* v, const float* proj, const int32_t* lens,
                                     int T, int H, int Nq, int Nc, int d, int m, int task_group, float* out, float* w, void* ws, size_t ws_bytes,
                                     hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || task_group < 0 || !q || !state || !v || !proj || !out) {
    set_error("%s: bad argument", what);
    return MLHOT_ERR_ARG;
  }
  if (!(wide ? favor_long_ok(T, H, Nc, d, m) : favor_cached_ok(T, H, Nc, d, m))) {
    set_error("%s serves Nc <= %d, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, wide ? 256 : 32, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)w; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < FAVOR_SHARED_QUERY_WS) { set_error("%s: workspace too small", what); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fsh::QT - 1) / fsh::QT;
  if (ntile * T * H >= (1ll << 31)) {
    set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what);
    return wide ? MLHOT_ERR_UNSUPPORTED : MLHOT_ERR_ARG;
  }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) {
    set_error("%s: q, proj and state must be 16-byte aligned", what);
    return wide ? MLHOT_ERR_UNSUPPORTED : MLHOT_ERR_ARG;
  }
  if (w && (reinterpret_cast<uintptr_t>(w) & 3) != 0) { set_error("%s: w must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  fsh::Args a{};
  a.q = q; a.proj = proj; a.v = v; a.lens = wide ? lens : nullptr; a.out = out; a.w = w;
  a.T = T; a.H = H; a.Nq = Nq; a.Nc = Nc; a.d = d; a.m = m; a.ntile = (int)ntile;
  a.sc = ft::Scales(d, m);
  if (wide) { const fl2::State st = fl2::carve_state(T, H, Nc, m, const_cast<void*>(state)); a.fk = st.fk; a.mp = st.mp; }
  else { const fc::State st = fc::carve_state(T, H, Nc, m, const_cast<void*>(state)); a.fk = st.fk; a.mp = st.mp; }
  a.tg = fsh::tasks_per_group(task_group, T, H, ntile);
  const long long groups = (T + a.tg - 1) / a.tg;
  const unsigned grid = (unsigned)(groups * H * ntile);           // <= T H ntile < 2^31
  const char* label = wide ? (w ? "favor.lquerysw" : "favor.lquerys") : (w ? "favor.querysw" : "favor.querys");
  ProfScope ps(label, s);
  if (wide) {
    if (w) hipLaunchKernelGGL(fsh::long_weights_kernel, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fsh::long_kernel, dim3(grid), dim3(256), 0, s, a);
  } else {
    if (w) hipLaunchKernelGGL(fsh::cached_weights_kernel, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fsh::cached_kernel, dim3(grid), dim3(256), 0, s, a);
  }
  return check_launch(label);
#endif
}

}  // namespace mlhot
