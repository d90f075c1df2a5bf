// Per-shot FAVOR+ key states beyond 32 context slots: favor_cached.h's split - condition once, query for any targets - with the
// slots walked in chunks of 32, up to 256 per task.  The state keeps what favor_cached.h's keeps, the finished key
// features of every slot, so it is the form that can read out FAVOR+'s per-shot weights (6c-5) above 32 shots.
//   keys   K1 grid (task x head, 256-feature chunk, 32-row chunk): ft::keys_dd on the chunk's rows into the state, the workgroup's
//          maximum; a chunk wholly behind lens[t] reads no k and leaves -inf
//          K2 grid (task x head): M from ALL workgroup maxima (fast_attention.py:96-97), diag_k and F_k in place, row chunk after
//          row chunk; rows behind lens[t] get exact zeros without a read
//   query  grid (task x head x 16-row query tile), ONE launch for any Nq >= 1: ft::query_front; then per chunk c of the task's
//          need = lens[t] slots ft::s_tile against rows 32 c .. of F_k, copied into columns 32 c .. of the wide tile S[16][<= 256];
//          D = the need columns in order; w = S / D (WOUT); out = one chain per element over the slots in ascending order / D
// State (floats): fc::State's with Nc = the capacity - F_k [T][H][Nc][mp], then M in a block of 64 - then K1's T H nch nrc maxima.
// Masked slots: a row of F_k behind lens[t] is exact zeros, so its column of S is +0 and adds nothing to D or to a chain; the query
// therefore stops at the last chunk that holds a shot and selects zeros by index behind lens[t] - the bits do not depend on the
// capacity the same shots are kept in, and rows of v behind lens[t] are not read at all.
// ROW INVARIANCE as in favor_cached.h: a workgroup owns its 16 rows and every feature and slot of them; every summation order is a
// function of d, m and the task's slot count alone; no atomics.  With at most 32 slots every step is the cached kernels' own
// (favor_tile.h's text, one chunk): the state, out and w then have favor_cached.h's bits.
// LDS of the query: favor_cached.h's 124 KB with the [16][33] S tile kept as s_tile's target, plus the wide tile 16 x 257 floats =
// 16.1 KB: 140 KB of gfx950's 160 KB, one workgroup per CU as before.
#pragma once
#include "common.h"
#include "favor_tile.h"
#include "favor_cached.h"

namespace mlhot {

constexpr int FAVOR_LONG_MAXNC = 256;

inline bool favor_long_ok(int T, int H, int Nc, int d, int m) {
#ifdef MLHOT_HOSTSIM
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return false;
#else
  return Nc >= 1 && Nc <= FAVOR_LONG_MAXNC && ft::envelope_ok(T, H, d, m);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace fl2 {

using ft::QT;
using ft::KCH;
constexpr int CH = ft::MAXNC;                       // slots per chunk
constexpr int LDW = FAVOR_LONG_MAXNC + 1;           // row stride of the wide S tile: odd, as ft::LDS_S

struct State { float* fk; float* M; float* part; int mp, nch, nrc; size_t floats; };
inline State carve_state(int T, int H, int Nc, int m, void* state) {
  State s{};
  s.mp = (m + 15) / 16 * 16; s.nch = (s.mp + KCH - 1) / KCH; s.nrc = (Nc + CH - 1) / CH;
  const size_t nfk = (size_t)T * H * Nc * s.mp;
  s.fk = (float*)state; s.M = s.fk + nfk; s.part = s.M + 64;
  s.floats = nfk + 64 + align_up((size_t)T * H * s.nch * s.nrc, 64);
  return s;
}

struct Args {
  const float *x, *proj, *fk, *v;         // x: the keys (K1, K2) or the queries
  const int32_t* lens;                    // [T] on the device, or nullptr: every task holds Nc shots
  float *fkw, *M, *part, *out, *w;
  int T, H, Nq, Nc, d, m, mp, nch, nrc, ntile;
  ft::Scales sc;
};

// ---- keys, launch 1: dd_k of one 32-row chunk into the state, the workgroup's maximum ------------------------------------------
__global__ __launch_bounds__(256) void keys1_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float xs[CH * ft::LDX];
  __shared__ float s_w[4];
  const int th = blockIdx.x, t = th / a.H, h = th % a.H, r0 = blockIdx.z * CH;
  const int len = min(ft::clamp_len(a.lens, t, 1, a.Nc) - r0, CH);          // this chunk's shots; <= 0: none (one scalar per workgroup)
  float* part = a.part + ((size_t)th * a.nch + blockIdx.y) * a.nrc + blockIdx.z;
  if (len <= 0) {
    if (threadIdx.x == 0) part[0] = -INFINITY;
    return;
  }
  ft::keys_dd<2, false, true>([&](int r) { return a.x + ((size_t)(t * a.Nc + r0 + r) * a.H + h) * a.d; }, len, a.proj, a.sc.c, a.d, a.m, a.mp,
                              a.fkw + ((size_t)th * a.Nc + r0) * a.mp, part, xs, s_w);
}

// ---- keys, launch 2: M, diag_k, F_k = ratio exp(dd - diag - M) + ratio 1e-4 in place, chunk after chunk ----------------------------
__global__ __launch_bounds__(256) void keys2_kernel(const Args a) {
  __shared__ float s_w[4], s_diag[CH];
  const int tid = threadIdx.x;
  const int th = blockIdx.x, t = th / a.H, h = th % a.H;
  const int d = a.d, m = a.m, Nc = a.Nc, mp = a.mp;
  const int len = ft::clamp_len(a.lens, t, 1, Nc);
  ft::part_max(a.part, a.T * a.H * a.nch * a.nrc, s_w, tid);
  __syncthreads();
  const float M = ft::max4(s_w[0], s_w[1], s_w[2], s_w[3]);
  if (th == 0 && tid == 0) a.M[0] = M;
  const int q4 = mp / 4;
  for (int r0 = 0; r0 < Nc; r0 += CH) {
    const int rows = min(CH, Nc - r0);
    float* blk = a.fkw + ((size_t)th * Nc + r0) * mp;
    if (r0 >= len) {                                                        // no shot in this chunk: zeros, nothing read
      for (int idx = tid; idx < rows * q4; idx += 256) reinterpret_cast<float4*>(blk)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    {
      const int r = r0 + (tid >> 3);
      const float dg = ft::key_diag(r < len ? a.x + ((size_t)(t * Nc + r) * a.H + h) * d : nullptr, d, a.sc.c, tid);
      if ((tid & 7) == 0) s_diag[tid >> 3] = dg;
    }
    __syncthreads();
    for (int idx = tid; idx < rows * q4; idx += 256) {
      const int row = idx / q4, j = 4 * (idx - row * q4);
      float4* at = reinterpret_cast<float4*>(blk + (size_t)row * mp + j);
      if (r0 + row >= len) { *at = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
      *at = ft::feature4(*at, s_diag[row] + M, j, m, a.sc);
    }
    __syncthreads();                                                        // s_diag is the next chunk's
  }
}

// ---- query: one workgroup per (task, head, 16 query rows) -------------------------------------------------------------------------
// ft::s_tile writes its [16][33] tile; between its last barrier and the first barrier of the next call nothing else touches that
// tile, so the copy into the wide tile needs no barrier of its own.  WOUT: w[t][h][n][n'] = S / D for the tile's rows and ALL Nc
// columns, exact zeros behind the task's slots (selected by index) - favor_cached.h's store, one IEEE divide per element.
template <bool WOUT>
__device__ __forceinline__ void query_body(const Args& a) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc);
  // 1. - 3. c q and diag, dd and the row maxima, F_q in place
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  // 4. S = F_q F_k^T chunk by chunk, D = rowsum(S)
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
  // 5. out[t][n][e H + h] = sum_n' S[n][n'] v[(t, n', h)][e] / D[n]
  ft::sv_tiles_wide(s_W, LDW, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, need, d, wv, lr, lq, [&](int row, int e, float o) {
    const int n = n0 + row;
    if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
  });
}

__global__ __launch_bounds__(256) void query_kernel(const Args a) { query_body<false>(a); }
__global__ __launch_bounds__(256) void query_weights_kernel(const Args a) { query_body<true>(a); }

// ---- masked query (mlhot_favor_query_long_masked_fwd): G context masks per target row, ONE front half -------------
// Steps 1. - 4. are query_body's, once per tile.  Then per group g: the wide tile with the dropped columns set to +0 (ft::s_mask,
// into the space of the scaled query tile, dead behind step 2), D_g over the task's need columns in order, w_g and out_g by
// query_body's own steps on that tile - with every bit set, query_weights_kernel's bits.  A slot counts iff its bit is set AND it
// is behind no lens[t]: the tile ends at need.  mask [T][G][Nq][W] words, W = ceil(Nc / 32); out [T][G][Nq][d H], w [T][G][H][Nq][Nc].
template <bool WOUT>
__device__ __forceinline__ void query_masked_body(const Args& a, const uint32_t* mask, int G) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  static_assert(QT * LDW <= QT * ft::LDX, "the masked wide tile lives in xs");
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
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
  float* s_Wm = xs;
  const int rows = min(QT, Nq - n0), W = (Nc + 31) / 32;
  for (int g = 0; g < G; ++g) {
    const size_t tg = (size_t)t * G + g;
    const uint32_t* mg = mask + (tg * Nq + n0) * W;
    ft::s_mask(s_W, s_Wm, LDW, need, [&](int row, int c) { return row < rows ? mg[row * W + c] : 0u; });
    ft::s_rowsum_wide(s_Wm, LDW, need, s_D);
    if constexpr (WOUT) {
      float* wt = a.w + ((tg * H + h) * Nq + n0) * Nc;
      for (int idx = tid; idx < rows * Nc; idx += 256) {
        const int row = idx / Nc, np = idx - row * Nc;
        wt[idx] = np < need ? ft::div_kept(s_Wm[row * LDW + np], s_D[row]) : 0.f;
      }
    }
    // sv_tiles_wide hands over o / D: a row that kept nothing (D == 0) is 0 / 0 there and stores exact zeros here
    ft::sv_tiles_wide(s_Wm, LDW, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, need, d, wv, lr, lq, [&](int row, int e, float o) {
      if (row < rows) a.out[(tg * Nq + n0 + row) * ((size_t)d * H) + (size_t)e * H + h] = s_D[row] > 0.f ? o : 0.f;
    });
    __syncthreads();                                                        // s_Wm and s_D are the next group's
  }
}

__global__ __launch_bounds__(256) void query_masked_kernel(const Args a, const uint32_t* mask, int G) { query_masked_body<false>(a, mask, G); }
__global__ __launch_bounds__(256) void query_masked_weights_kernel(const Args a, const uint32_t* mask, int G) { query_masked_body<true>(a, mask, G); }

inline Args make_args(int T, int H, int Nq, int Nc, int d, int m, const State& st, const int32_t* lens) {
  Args a{};
  a.T = T; a.H = H; a.Nq = Nq; a.Nc = Nc; a.d = d; a.m = m; a.mp = st.mp; a.nch = st.nch; a.nrc = st.nrc;
  a.fk = st.fk; a.fkw = st.fk; a.M = st.M; a.part = st.part; a.lens = lens;
  a.sc = ft::Scales(d, m);
  return a;
}

}  // namespace fl2
#endif

inline size_t favor_keys_long_need(int T, int H, int Nc, int d, int m) {
#ifndef MLHOT_HOSTSIM
  if (favor_long_ok(T, H, Nc, d, m)) return fl2::carve_state(T, H, Nc, m, nullptr).floats * sizeof(float);
#endif
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return 0;
}

constexpr size_t FAVOR_LONG_QUERY_WS = 256;       // the query kernel works in LDS alone; the ABI's ws is favor_query_fwd's token block

// lens: int32 [T] on the device (read there: no host synchronisation, the call stays capturable), or nullptr for full tasks
inline int favor_keys_long_forward(const float* k, const float* proj, const int32_t* lens, int T, int H, int Nc, int d, int m, void* state,
                                   size_t state_bytes, hipStream_t s) {
  const char* what = "favor_keys_long_fwd";
  if (T <= 0 || H <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !k || !proj || !state) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_long_ok(T, H, Nc, d, m)) {
    set_error("%s serves Nc <= 256, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)state_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const fl2::State st = fl2::carve_state(T, H, Nc, m, state);
  if (state_bytes < st.floats * sizeof(float)) { set_error("%s: state too small (%zu < %zu)", what, state_bytes, st.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(k) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: k, proj and state must be 16-byte aligned", what); return MLHOT_ERR_UNSUPPORTED; }
  fl2::Args a = fl2::make_args(T, H, 0, Nc, d, m, st, lens);
  a.x = k; a.proj = proj;
  {
    ProfScope ps("favor.lkeys1", s);
    hipLaunchKernelGGL(fl2::keys1_kernel, dim3(T * H, st.nch, st.nrc), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor.lkeys1"));
  {
    ProfScope ps("favor.lkeys2", s);
    hipLaunchKernelGGL(fl2::keys2_kernel, dim3(T * H), dim3(256), 0, s, a);
  }
  return check_launch("favor.lkeys2");
#endif
}

// w == nullptr: out alone; otherwise the read-out instantiation, which also writes w [T][H][Nq][Nc] (4-byte aligned, as every float*)
inline int favor_query_long_forward(const float* q, const void* state, const float* v, const float* proj, const int32_t* lens, int T, int H, int Nq,
                                    int Nc, int d, int m, float* out, float* w, void* ws, size_t ws_bytes, hipStream_t s) {
  const char* what = "favor_query_long_fwd";
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !q || !state || !v || !proj || !out) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_long_ok(T, H, Nc, d, m)) {
    set_error("%s serves Nc <= 256, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)w; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < FAVOR_LONG_QUERY_WS) { set_error("%s: workspace too small", what); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fl2::QT - 1) / fl2::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return MLHOT_ERR_UNSUPPORTED; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: q, proj and state must be 16-byte aligned", what); return MLHOT_ERR_UNSUPPORTED; }
  if (w && (reinterpret_cast<uintptr_t>(w) & 3) != 0) { set_error("%s: w must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  const fl2::State st = fl2::carve_state(T, H, Nc, m, const_cast<void*>(state));
  fl2::Args a = fl2::make_args(T, H, Nq, Nc, d, m, st, lens);
  a.x = q; a.proj = proj; a.v = v; a.out = out; a.w = w; a.ntile = (int)ntile;
  const char* label = w ? "favor.lqueryw" : "favor.lquery";
  ProfScope ps(label, s);
  if (w) hipLaunchKernelGGL(fl2::query_weights_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(fl2::query_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a);
  return check_launch(label);
#endif
}

// mlhot_favor_query_long_masked_fwd: G context masks per target row in one launch - mask [T][G][Nq][ceil(Nc / 32)]
// words on the device, out [T][G][Nq][d H], w [T][G][H][Nq][Nc] or nullptr.  Everything else is favor_query_long_forward's.
inline int favor_query_long_masked_forward(const float* q, const void* state, const float* v, const float* proj, const int32_t* lens, const uint32_t* mask,
                                           int G, int T, int H, int Nq, int Nc, int d, int m, float* out, float* w, void* ws, size_t ws_bytes, hipStream_t s) {
  const char* what = "favor_query_long_masked_fwd";
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || G < 1 || !q || !state || !v || !proj || !out || !mask) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_long_ok(T, H, Nc, d, m)) {
    set_error("%s serves Nc <= 256, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)w; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < FAVOR_LONG_QUERY_WS) { set_error("%s: workspace too small", what); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fl2::QT - 1) / fl2::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return MLHOT_ERR_UNSUPPORTED; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: q, proj and state must be 16-byte aligned", what); return MLHOT_ERR_UNSUPPORTED; }
  if ((reinterpret_cast<uintptr_t>(mask) & 3) != 0 || (w && (reinterpret_cast<uintptr_t>(w) & 3) != 0)) { set_error("%s: mask_words and w must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  const fl2::State st = fl2::carve_state(T, H, Nc, m, const_cast<void*>(state));
  fl2::Args a = fl2::make_args(T, H, Nq, Nc, d, m, st, lens);
  a.x = q; a.proj = proj; a.v = v; a.out = out; a.w = w; a.ntile = (int)ntile;
  const char* label = w ? "favor.lquerymw" : "favor.lquerym";
  ProfScope ps(label, s);
  if (w) hipLaunchKernelGGL(fl2::query_masked_weights_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a, mask, G);
  else hipLaunchKernelGGL(fl2::query_masked_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a, mask, G);
  return check_launch(label);
#endif
}

}  // namespace mlhot
