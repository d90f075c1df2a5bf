// Per-shot FAVOR+ key states beyond 256 context slots: favor_long.h's split with the query's wide S tile walked in PAGES of 256
// slots, up to 4096 slots per task.  The state is fl2::State's and the key side IS fl2's two kernels (they walk
// 32-row chunks of any count); only the query is new.
//   query  grid (task x head x 16-row query tile), ONE launch for any Nq >= 1: ft::query_front once; then per page p0 of the task's
//          need = lens[t] slots: eight ft::s_tile calls into the wide tile S[16][<= 256] (favor_long.h's loop, column 0 = slot p0);
//          D carries on over the page's columns (ft::s_rowsum_page: ONE ascending chain over all slots, never a sum of page sums);
//          the out chains carry on over the page's slots with their accumulators in registers (ft::sv_page); out / D behind the
//          last page.
//   w      needs the final D.  A page that is not the last stores its UNNORMALISED S into w; behind the last page the workgroup
//          divides its own rows in place - thread tid owns column tid of every page, at the store and at the divide, so every
//          thread re-reads only what it wrote itself.  One IEEE divide S / D per element, as favor_long.h's store; the last page
//          (with one page: the only one) is divided straight from LDS.
//   masked pages outside, groups inside (DESIGN.md 6c-10's contract): per page S is formed ONCE; per group ft::s_mask of the page,
//          D_g carried in the workspace (T H ntile G 16 floats), the unnormalised out_g in the group's own out rows, w_g as above -
//          every carried float is written and re-read by the same thread, and an fp32 store and load carries a chain exactly.
// Every summation order is a function of d, m and lens[t] alone; no atomics.  With Nc <= 256 there is one page and every step is
// favor_long.h's (favor_tile.h's text): state, out and w then have the long entries' bits.
// LDS: favor_long.h's arrays exactly (142,848 bytes), one workgroup per CU as before.
#pragma once
#include "common.h"
#include "favor_tile.h"
#include "favor_long.h"

namespace mlhot {

constexpr int FAVOR_PAGED_MAXNC = 4096;           // an envelope decision: F_k and w grow linearly with Nc

// T Nc < 2^31: the reused key kernels index the rows of k as an int
inline bool favor_paged_ok(int T, int H, int Nc, int d, int m) {
#ifdef MLHOT_HOSTSIM
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return false;
#else
  return Nc >= 1 && Nc <= FAVOR_PAGED_MAXNC && ft::envelope_ok(T, H, d, m) && (long long)T * Nc < (1ll << 31);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace fp2 {

using ft::QT;
using fl2::Args;
using fl2::CH;
using fl2::LDW;
constexpr int PAGE = FAVOR_LONG_MAXNC;            // slots per page: the wide tile's columns
static_assert(PAGE == 256, "thread tid owns column tid of a page");

// S of the page p0 .. p0 + pn into the wide tile: favor_long.h's chunk loop, barrier behind it
__device__ __forceinline__ void s_page(const Args& a, int th, int p0, int pn, const float* s_f, float* red, float* s_S, float* s_W, int tid, int lr, int lq) {
  for (int c0 = 0; c0 < pn; c0 += CH) {
    const int ncol = min(CH, pn - c0);
    const float* krow[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < ncol ? a.fk + ((size_t)th * a.Nc + p0 + c0 + 16 * jj + lr) * a.mp + 4 * lq : nullptr;
    ft::s_tile(s_f, ft::ldf(a.mp), krow, (ncol + 15) / 16, a.mp / 16, ncol, ft::BPlain{}, red, s_S);
    for (int idx = tid; idx < QT * CH; idx += 256) {
      const int row = idx / CH, np = idx - row * CH;
      if (np < ncol) s_W[row * LDW + c0 + np] = s_S[row * ft::LDS_S + np];
    }
  }
  __syncthreads();
}

// w of the tile's rows (wt = row 0, column 0; row stride Nc) for the page at p0 held in s_P.  Not the last page: the page
// unnormalised.  The last page: the page / D from LDS, the earlier pages / D in place, zeros behind need.  norm(x, D) is the divide.
template <class Norm>
__device__ __forceinline__ void w_page(float* wt, const float* s_P, const float* s_D, int rows, int p0, int pn, int need, int Nc, bool last, int tid, Norm norm) {
  if (!last) {
    for (int row = 0; row < rows; ++row) wt[(size_t)row * Nc + p0 + tid] = s_P[row * LDW + tid];      // pn == PAGE
    return;
  }
  for (int row = 0; row < rows; ++row) {
    float* wr = wt + (size_t)row * Nc;
    const float D = s_D[row];
    for (int pp = 0; pp < p0; pp += PAGE) wr[pp + tid] = norm(wr[pp + tid], D);
    if (tid < pn) wr[p0 + tid] = norm(s_P[row * LDW + tid], D);
    for (int np = need + tid; np < Nc; np += 256) wr[np] = 0.f;
  }
}

template <bool WOUT>
__device__ __forceinline__ void paged_body(const Args& a) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc), rows = min(QT, Nq - n0);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* v0 = a.v + ((size_t)t * Nc * H + h) * d;
  ft::f32x4_t o[ft::MAXD / 64];                                               // channel tiles wv, wv + 4, ..: carried across the pages
#pragma unroll
  for (int i = 0; i < ft::MAXD / 64; ++i) o[i] = ft::f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int p0 = 0; p0 < need; p0 += PAGE) {
    const int pn = min(PAGE, need - p0);
    const bool last = p0 + PAGE >= need;
    s_page(a, th, p0, pn, s_f, red, s_S, s_W, tid, lr, lq);
    ft::s_rowsum_page(s_W, LDW, pn, s_D, p0 > 0 ? s_D : nullptr);
    if constexpr (WOUT)
      w_page(a.w + ((size_t)th * Nq + n0) * Nc, s_W, s_D, rows, p0, pn, need, Nc, last, tid, [](float x, float D) { return x / D; });
#pragma unroll
    for (int i = 0; i < ft::MAXD / 64; ++i) {
      const int et = wv + 4 * i;
      if (et * 16 < d) o[i] = ft::sv_page(o[i], s_W, LDW, v0, (size_t)H * d, p0, p0 + pn, need, 16 * et + lr, lr, lq);
    }
    __syncthreads();                                                          // the wide tile is the next page's
  }
#pragma unroll
  for (int i = 0; i < ft::MAXD / 64; ++i) {
    const int e = 16 * (wv + 4 * i) + lr;
    if (e < d) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * lq + r;
        if (row < rows) a.out[((size_t)t * Nq + n0 + row) * ((size_t)d * H) + (size_t)e * H + h] = o[i][r] / s_D[row];
      }
    }
  }
}

__global__ __launch_bounds__(256) void query_kernel(const Args a) { paged_body<false>(a); }
__global__ __launch_bounds__(256) void query_weights_kernel(const Args a) { paged_body<true>(a); }

// ---- masked query (mlhot_favor_query_paged_masked_fwd): 6c-10's contract, pages outside and groups inside ---------------------------
// dws [T H ntile][G][16]: D_g of the tile's rows between the pages, written and re-read by thread row < 16 of the same workgroup.
template <bool WOUT>
__device__ __forceinline__ void paged_masked_body(const Args& a, const uint32_t* mask, int G, float* dws) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  static_assert(QT * LDW <= QT * ft::LDX, "the masked wide tile lives in xs");
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc), rows = min(QT, Nq - n0), W = (Nc + 31) / 32;
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* v0 = a.v + ((size_t)t * Nc * H + h) * d;
  float* s_Wm = xs;
  float* dg = dws + (size_t)blockIdx.x * G * QT;
  for (int p0 = 0; p0 < need; p0 += PAGE) {
    const int pn = min(PAGE, need - p0);
    const bool first = p0 == 0, last = p0 + PAGE >= need;
    s_page(a, th, p0, pn, s_f, red, s_S, s_W, tid, lr, lq);
    for (int g = 0; g < G; ++g) {
      const size_t tg = (size_t)t * G + g;
      const uint32_t* mg = mask + (tg * Nq + n0) * W + p0 / 32;
      ft::s_mask(s_W, s_Wm, LDW, pn, [&](int row, int c) { return row < rows ? mg[(size_t)row * W + c] : 0u; });
      ft::s_rowsum_page(s_Wm, LDW, pn, s_D, first ? nullptr : dg + g * QT);
      if (!last && tid < QT) dg[g * QT + tid] = s_D[tid];
      if constexpr (WOUT)
        w_page(a.w + ((tg * H + h) * Nq + n0) * Nc, s_Wm, s_D, rows, p0, pn, need, Nc, last, tid, [](float x, float D) { return ft::div_kept(x, D); });
      for (int et = wv; et * 16 < d; et += 4) {
        const int e = 16 * et + lr;
        float* og = a.out + (tg * Nq + n0) * ((size_t)d * H) + (size_t)e * H + h;            // row 0's element; a lane re-reads its own
        ft::f32x4_t o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = !first && 4 * lq + r < rows ? og[(size_t)(4 * lq + r) * ((size_t)d * H)] : 0.f;
        o = ft::sv_page(o, s_Wm, LDW, v0, (size_t)H * d, p0, p0 + pn, need, e, lr, lq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * lq + r;
          // a row that kept nothing (D == 0) is 0 / 0 there and stores exact zeros here
          if (row < rows) og[(size_t)row * ((size_t)d * H)] = !last ? o[r] : s_D[row] > 0.f ? o[r] / s_D[row] : 0.f;
        }
      }
      __syncthreads();                                                        // s_Wm and s_D are the next group's
    }
  }
}

__global__ __launch_bounds__(256) void query_masked_kernel(const Args a, const uint32_t* mask, int G, float* dws) { paged_masked_body<false>(a, mask, G, dws); }
__global__ __launch_bounds__(256) void query_masked_weights_kernel(const Args a, const uint32_t* mask, int G, float* dws) { paged_masked_body<true>(a, mask, G, dws); }

}  // namespace fp2
#endif

inline size_t favor_keys_paged_need(int T, int H, int Nc, int d, int m) {
#ifndef MLHOT_HOSTSIM
  if (favor_paged_ok(T, H, Nc, d, m)) return fl2::carve_state(T, H, Nc, m, nullptr).floats * sizeof(float);
#endif
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return 0;
}

// workspace of the query entries: G == 0, the unmasked entry - favor_query_fwd's token block (the kernel works in LDS alone);
// G >= 1, the masked entry - D_g between the pages, T H ceil(Nq / 16) G 16 floats.  0 for a shape not served.
inline size_t favor_query_paged_ws_need(int T, int H, int Nq, int Nc, int d, int m, int G) {
#ifndef MLHOT_HOSTSIM
  if (favor_paged_ok(T, H, Nc, d, m) && Nq >= 1 && G >= 0) {
    const size_t ntile = ((size_t)Nq + 15) / 16;
    const size_t dws = (size_t)T * H * ntile * (size_t)G * 16 * sizeof(float);
    return dws > FAVOR_LONG_QUERY_WS ? align_up(dws, (size_t)256) : FAVOR_LONG_QUERY_WS;
  }
#endif
  (void)T; (void)H; (void)Nq; (void)Nc; (void)d; (void)m; (void)G; return 0;
}

#define MLHOT_PAGED_ENVELOPE "%s serves Nc <= 4096, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)"

// the state, lens and the contract are favor_keys_long_forward's; the launches are fl2's own
inline int favor_keys_paged_forward(const float* k, const float* proj, const int32_t* lens, int T, int H, int Nc, int d, int m, void* state,
                                    size_t state_bytes, hipStream_t s) {
  const char* what = "favor_keys_paged_fwd";
  if (T <= 0 || H <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !k || !proj || !state) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_paged_ok(T, H, Nc, d, m)) { set_error(MLHOT_PAGED_ENVELOPE, what, Nc, d, m); return MLHOT_ERR_UNSUPPORTED; }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)state_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const fl2::State st = fl2::carve_state(T, H, Nc, m, state);
  if (state_bytes < st.floats * sizeof(float)) { set_error("%s: state too small (%zu < %zu)", what, state_bytes, st.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(k) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: k, proj and state must be 16-byte aligned", what); return MLHOT_ERR_UNSUPPORTED; }
  fl2::Args a = fl2::make_args(T, H, 0, Nc, d, m, st, lens);
  a.x = k; a.proj = proj;
  {
    ProfScope ps("favor.pkeys1", s);
    hipLaunchKernelGGL(fl2::keys1_kernel, dim3(T * H, st.nch, st.nrc), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor.pkeys1"));
  {
    ProfScope ps("favor.pkeys2", s);
    hipLaunchKernelGGL(fl2::keys2_kernel, dim3(T * H), dim3(256), 0, s, a);
  }
  return check_launch("favor.pkeys2");
#endif
}

// mask == nullptr && G == 0: the unmasked entry, out [T][Nq][d H], w [T][H][Nq][Nc] or nullptr.  Otherwise the masked entry:
// mask [T][G][Nq][ceil(Nc / 32)] words, out [T][G][Nq][d H], w [T][G][H][Nq][Nc] or nullptr.
inline int favor_query_paged_launch(const char* what, bool masked, const float* q, const void* state, const float* v, const float* proj, const int32_t* lens,
                                    const uint32_t* mask, int G, int T, int H, int Nq, int Nc, int d, int m, float* out, float* w, void* ws, size_t ws_bytes,
                                    hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !q || !state || !v || !proj || !out || (masked && (G < 1 || !mask))) {
    set_error("%s: bad argument", what);
    return MLHOT_ERR_ARG;
  }
  if (!favor_paged_ok(T, H, Nc, d, m)) { set_error(MLHOT_PAGED_ENVELOPE, what, Nc, d, m); return MLHOT_ERR_UNSUPPORTED; }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)w; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const long long ntile = ((long long)Nq + fp2::QT - 1) / fp2::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return MLHOT_ERR_UNSUPPORTED; }
  const size_t need = favor_query_paged_ws_need(T, H, Nq, Nc, d, m, masked ? G : 0);
  if (ws == nullptr || ws_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", what, ws_bytes, need); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: q, proj and state must be 16-byte aligned", what); return MLHOT_ERR_UNSUPPORTED; }
  if ((masked && (reinterpret_cast<uintptr_t>(mask) & 3) != 0) || (w && (reinterpret_cast<uintptr_t>(w) & 3) != 0) || (reinterpret_cast<uintptr_t>(ws) & 3) != 0) {
    set_error("%s: mask_words, w and ws must be 4-byte aligned", what);
    return MLHOT_ERR_ARG;
  }
  const fl2::State st = fl2::carve_state(T, H, Nc, m, const_cast<void*>(state));
  fl2::Args a = fl2::make_args(T, H, Nq, Nc, d, m, st, lens);
  a.x = q; a.proj = proj; a.v = v; a.out = out; a.w = w; a.ntile = (int)ntile;
  const dim3 grid((unsigned)(ntile * T * H));
  const char* label = masked ? (w ? "favor.pquerymw" : "favor.pquerym") : (w ? "favor.pqueryw" : "favor.pquery");
  ProfScope ps(label, s);
  if (masked) {
    if (w) hipLaunchKernelGGL(fp2::query_masked_weights_kernel, grid, dim3(256), 0, s, a, mask, G, (float*)ws);
    else hipLaunchKernelGGL(fp2::query_masked_kernel, grid, dim3(256), 0, s, a, mask, G, (float*)ws);
  } else {
    if (w) hipLaunchKernelGGL(fp2::query_weights_kernel, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fp2::query_kernel, grid, dim3(256), 0, s, a);
  }
  return check_launch(label);
#endif
}

}  // namespace mlhot
