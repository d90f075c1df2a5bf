// FAVOR+ attention split at the context: condition once, query for any number of targets.
//
// The key features  F_k = ratio (exp(dd_k - diag_k - M) + 1e-4),  M = the maximum of dd_k over the keys of the WHOLE batch
// (fast_attention.py:96-97), depend on the context alone; the query features use their own row maximum (:92-94) and
// out = S V / D with S = F_q F_k^T, D = rowsum(S) is row-wise in the queries.  So:
//   keys   K1 grid (task x head, 256-feature chunk): dd_k = (c k) P^T on the matrix core into the state, the workgroup's maximum
//          K2 grid (task x head): M from the workgroup maxima, diag_k, F_k in place (features >= m are zeros); block 0 leaves M
//   query  grid (task x head x 16-row query tile), ONE launch for any Nq >= 1:
//          dd_q = (c q) P^T into LDS, row maxima, F_q in place, S = F_q F_k^T over all m features, D, out = S V / D (merged order)
// State (floats): F_k [T][H][Nc][mp], mp = m rounded up to 16; then M at offset T H Nc mp; then K1's workgroup maxima.
// Per-task context sizes: the key launches have a masked instantiation - rows n >= lens[t] are never read, stay
// out of M and are exact zeros in F_k; such a row's column of S is 0, so the query launch serves that state unchanged.
//
// ROW INVARIANCE of the query launch, as for linear_rows.h: the bits of out[t, n, :] depend on q[t, n], the state, v, proj and the
// dimensions - not on Nq, on n, on the row's place in its tile, on the grid or on the other query rows.  What makes it so:
//   * a workgroup owns 16 query rows and every feature of them: no split across workgroups, no atomics;
//   * every sum has one order, a function of d, m and Nc alone: dd is one v_mfma_f32_16x16x4_f32 chain over k = 0, 16, .. per
//     element (favor2.h's F1 order); S is four chains - wave w takes the 16-feature chunks w, w + 4, .. in ascending order - folded
//     w = 0, 1, 2, 3; D adds the Nc columns of S in order; out is one chain over the 32 key slots (zeros beyond Nc);
//   * |q|^2 is 16 lanes x 4 float4 per row in a fixed order and a butterfly over the 16 lanes (commutative at every level, so
//     every lane ends with the same bits); the row maximum is exact in any order;
//   * rows >= Nq are read as zeros and never stored; they share no sum with a stored row;
//   * an fp32 MFMA computes an output element the same way at every row of its tile - the assumption linear_rows.h makes too, and
//     tests/test_condition_gpu.py measures (single rows, shifted and permuted rows).
// Tile choice: 32 rows of dd at m = 1419 are 182 KB, over gfx950's 160 KB of LDS; recomputing dd for a second pass doubles the
// dominant cost (16 x 1424 x 256 MACs per tile against 16 x 1424 x 32 for S).  16 rows x (1536 + 8) floats = 96.5 KB stay in LDS
// between the passes; with the scaled query tile (16.5 KB) and the fold buffer (8 KB) the kernel holds 124 KB: one workgroup per CU.
#pragma once
#include "common.h"
#include "favor.h"
#include "favor2.h"
#include "favor_tile.h"

namespace mlhot {

// favor2.h's envelope on the context side; nothing bounds the number of query rows
inline bool favor_cached_ok(int T, int H, int Nc, int d, int m) {
#ifdef MLHOT_HOSTSIM
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return false;
#else
  return Nc >= 1 && Nc <= ft::MAXNC && ft::envelope_ok(T, H, d, m);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace fc {

using ft::QT;
using ft::KCH;

struct State { float* fk; float* M; float* part; int mp, nch; size_t floats; };
inline State carve_state(int T, int H, int Nc, int m, void* state) {
  State s{};
  s.mp = (m + 15) / 16 * 16; s.nch = (s.mp + KCH - 1) / KCH;
  const size_t nfk = (size_t)T * H * Nc * s.mp;
  s.fk = (float*)state; s.M = s.fk + nfk; s.part = s.M + 64;
  s.floats = nfk + 64 + align_up((size_t)T * H * s.nch, 64);
  return s;
}

struct Args {
  const float *x, *proj, *fk, *v;         // x: the keys (K1, K2) or the queries
  float *fkw, *M, *part, *out;
  int T, H, Nq, Nc, d, m, mp, nch, ntile;
  ft::Scales sc;
};

// ---- keys, launch 1: dd_k into the state, the workgroup's maximum (ft::keys_dd) ------------------------------------------------
// RAG (mlhot_favor_keys_ragged_fwd): row n of task t is a context shot iff n < lens[t] (held to 1 .. Nc).  Rows
// behind it are never read, never stored and never enter the maximum; K2 writes their zeros.
template <int RT, bool RAG>
__device__ __forceinline__ void keys1_body(const Args& a, const int32_t* lens) {
  __shared__ __attribute__((aligned(16))) float xs[16 * RT * ft::LDX];
  __shared__ float s_w[4];
  const int th = blockIdx.x, t = th / a.H, h = th % a.H;
  const int len = RAG ? ft::clamp_len(lens, t, 1, a.Nc) : a.Nc;
  ft::keys_dd<RT, false, RAG>([&](int r) { return a.x + ((size_t)(t * a.Nc + r) * a.H + h) * a.d; }, len, a.proj, a.sc.c, a.d, a.m, a.mp,
                         a.fkw + (size_t)th * a.Nc * a.mp, a.part + (size_t)th * a.nch + blockIdx.y, xs, s_w);
}

template <int RT>
__global__ __launch_bounds__(256) void keys1_kernel(const Args a) { keys1_body<RT, false>(a, nullptr); }
template <int RT>
__global__ __launch_bounds__(256) void keys1_ragged_kernel(const Args a, const int32_t* lens) { keys1_body<RT, true>(a, lens); }

// ---- keys, launch 2: M, diag_k, F_k = ratio exp(dd - diag - M) + ratio 1e-4 in place ----------------------------------------
// RAG: every workgroup of K1 held a valid row (lens[t] >= 1), so the fold of the maxima is unchanged; rows n >= lens[t] get exact
// zeros over all mp features without a read of k or of the state.
template <bool RAG>
__device__ __forceinline__ void keys2_body(const Args& a, const int32_t* lens) {
  __shared__ float s_w[4], s_diag[ft::MAXNC];
  const int tid = threadIdx.x;
  const int th = blockIdx.x, t = th / a.H, h = th % a.H;
  const int d = a.d, m = a.m, Nc = a.Nc, mp = a.mp;
  const int len = RAG ? ft::clamp_len(lens, t, 1, Nc) : Nc;
  ft::part_max(a.part, a.T * a.H * a.nch, s_w, tid);
  {
    const int r = tid >> 3;
    const float dg = ft::key_diag(r < len ? a.x + ((size_t)(t * Nc + r) * a.H + h) * d : nullptr, d, a.sc.c, tid);
    if (r < Nc && (tid & 7) == 0) s_diag[r] = dg;
  }
  __syncthreads();
  const float M = ft::max4(s_w[0], s_w[1], s_w[2], s_w[3]);
  if (th == 0 && tid == 0) a.M[0] = M;
  const int q4 = mp / 4;
  float* blk = a.fkw + (size_t)th * Nc * mp;
  for (int idx = tid; idx < Nc * q4; idx += 256) {
    const int row = idx / q4, j = 4 * (idx - row * q4);
    float4* at = reinterpret_cast<float4*>(blk + (size_t)row * mp + j);
    if (RAG && row >= len) { *at = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
    *at = ft::feature4(*at, s_diag[row] + M, j, m, a.sc);
  }
}

__global__ __launch_bounds__(256) void keys2_kernel(const Args a) { keys2_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void keys2_ragged_kernel(const Args a, const int32_t* lens) { keys2_body<true>(a, lens); }

// ---- query: one workgroup per (task, head, 16 query rows) -------------------------------------------------------------------
// WOUT (mlhot_favor_query_weights_fwd): behind D the workgroup also stores FAVOR+'s implied attention
// w[t][h][n][n'] = S[n][n'] / D[n] of its rows n < Nq and the columns n' < Nc - the tile's rows are one contiguous block of
// min(16, Nq - n0) x Nc floats of w [T][H][Nq][Nc], thread i takes the floats i, i + 256: consecutive lanes, consecutive addresses
// (a row of Nc floats has no alignment to speak of: scalar stores).  One IEEE divide per element, the same expression at every
// row of the tile, so w has out's row invariance; a zero row of F_k (a masked slot) is an exactly zero column.  Nothing of the
// S V chain, its fold or its division moves: out has the bits of the plain instantiation.
template <bool WOUT>
__device__ __forceinline__ void query_body(const Args& a, float* w) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  // 1. - 3. c q and diag, dd and the row maxima, F_q in place
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  // 4. S = F_q F_k^T, D = rowsum(S)
  const float* krow[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + ((size_t)th * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
  ft::s_tile(s_f, ft::ldf(mp), krow, (Nc + 15) / 16, mp / 16, Nc, ft::BPlain{}, red, s_S);
  ft::s_rowsum(s_S, Nc, s_D);
  if constexpr (WOUT) {
    float* wt = w + ((size_t)th * Nq + n0) * Nc;
    const int lim = min(QT, Nq - n0) * Nc;
    for (int idx = tid; idx < lim; idx += 256) {
      const int row = idx / Nc, np = idx - row * Nc;
      wt[idx] = s_S[row * ft::LDS_S + np] / s_D[row];
    }
  }
  // 5. out[t][n][e H + h] = sum_n' S[n][n'] v[(t, n', h)][e] / D[n]
  ft::sv_tiles(s_S, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, d, wv, lr, lq, [&](int row, int e, float o) {
    const int n = n0 + row;
    if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
  });
}

__global__ __launch_bounds__(256) void query_kernel(const Args a) { query_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void query_weights_kernel(const Args a, float* w) { query_body<true>(a, w); }

// ---- masked query (mlhot_favor_query_masked_fwd): G context masks per target row, ONE front half ----------------
// Steps 1. - 4. are query_body's, once per tile: nothing in them sees the mask.  Then per group g: S with the dropped columns set
// to +0 (ft::s_mask, into the space of the scaled query tile, which is dead behind step 2), D_g = its Nc columns in order,
// w_g = that tile / D_g, out_g = the same 32-slot chain / D_g - query_body's steps on another tile, so with every bit set the
// bits are query_weights_kernel's.  The value rows do not depend on g: a wave keeps those of its channel tiles in registers.
// mask [T][G][Nq] words (Nc <= 32: one word per row), out [T][G][Nq][d H], w [T][G][H][Nq][Nc].  A row without a kept valid slot
// has D_g == 0 and stores exact zeros.  Rows and groups share no sum: the bits of (t, g, n) depend on that row's words alone.
template <bool WOUT>
__device__ __forceinline__ void query_masked_body(const Args& a, const uint32_t* mask, int G, float* w) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_D[QT], s_diag[QT], s_pm[4][QT];
  static_assert(QT * ft::LDS_S <= QT * ft::LDX, "the masked tile lives in xs");
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* krow[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + ((size_t)th * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
  ft::s_tile(s_f, ft::ldf(mp), krow, (Nc + 15) / 16, mp / 16, Nc, ft::BPlain{}, red, s_S);
  float* s_Sm = xs;
  constexpr int ET = ft::MAXD / 64;                       // 16-channel tiles per wave
  float bv[ET][ft::MAXNC / 4];
#pragma unroll
  for (int k = 0; k < ET; ++k) ft::load_v(bv[k], a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, 16 * (wv + 4 * k) + lr, lq, 16 * (wv + 4 * k) < d);
  const int rows = min(QT, Nq - n0);
  for (int g = 0; g < G; ++g) {
    const size_t tg = (size_t)t * G + g;
    const uint32_t* mg = mask + tg * Nq + n0;
    ft::s_mask(s_S, s_Sm, ft::LDS_S, Nc, [&](int row, int) { return row < rows ? mg[row] : 0u; });
    ft::s_rowsum(s_Sm, Nc, s_D);
    if constexpr (WOUT) {
      float* wt = w + ((tg * H + h) * Nq + n0) * Nc;
      for (int idx = tid; idx < rows * Nc; idx += 256) {
        const int row = idx / Nc, np = idx - row * Nc;
        wt[idx] = ft::div_kept(s_Sm[row * ft::LDS_S + np], s_D[row]);
      }
    }
#pragma unroll
    for (int k = 0; k < ET; ++k) {
      const int e = 16 * (wv + 4 * k) + lr;
      if (16 * (wv + 4 * k) >= d) continue;
      const ft::f32x4_t o = ft::sv_chain(s_Sm, bv[k], Nc, lr, lq);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * lq + r;
        if (row < rows) a.out[(tg * Nq + n0 + row) * ((size_t)d * H) + (size_t)e * H + h] = ft::div_kept(o[r], s_D[row]);
      }
    }
    __syncthreads();                                      // s_Sm and s_D are the next group's
  }
}

__global__ __launch_bounds__(256) void query_masked_kernel(const Args a, const uint32_t* mask, int G) { query_masked_body<false>(a, mask, G, nullptr); }
__global__ __launch_bounds__(256) void query_masked_weights_kernel(const Args a, const uint32_t* mask, int G, float* w) { query_masked_body<true>(a, mask, G, w); }

inline Args make_args(int T, int H, int Nq, int Nc, int d, int m, const State& st) {
  Args a{};
  a.T = T; a.H = H; a.Nq = Nq; a.Nc = Nc; a.d = d; a.m = m; a.mp = st.mp; a.nch = st.nch;
  a.fk = st.fk; a.fkw = st.fk; a.M = st.M; a.part = st.part;
  a.sc = ft::Scales(d, m);
  return a;
}

}  // namespace fc
#endif

inline size_t favor_keys_need(int T, int H, int Nc, int d, int m) {
#ifndef MLHOT_HOSTSIM
  if (favor_cached_ok(T, H, Nc, d, m)) return fc::carve_state(T, H, Nc, m, nullptr).floats * sizeof(float);
#endif
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return 0;
}
inline size_t favor_query_ws_need(int T, int H, int Nq, int Nc, int d, int m) {      // the query kernel works in LDS alone
  return Nq >= 1 && favor_cached_ok(T, H, Nc, d, m) ? 256 : 0;
}

// lens == nullptr: mlhot_favor_keys_fwd; otherwise mlhot_favor_keys_ragged_fwd - the same state, the masked instantiations
inline int favor_keys_launch(const char* what, const float* k, const float* proj, const int32_t* lens, bool ragged, int T, int H, int Nc, int d, int m,
                             void* state, size_t state_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !k || !proj || !state || (ragged && !lens)) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_cached_ok(T, H, Nc, d, m)) {
    set_error("%s serves Nc <= 32, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)state_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const fc::State st = fc::carve_state(T, H, Nc, m, state);
  if (state_bytes < st.floats * sizeof(float)) { set_error("%s: state too small (%zu < %zu)", what, state_bytes, st.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(k) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: k, proj and state must be 16-byte aligned", what); return MLHOT_ERR_ARG; }
  fc::Args a = fc::make_args(T, H, 0, Nc, d, m, st);
  a.x = k; a.proj = proj;
  const char* l1 = ragged ? "favor.keys1r" : "favor.keys1";
  const char* l2 = ragged ? "favor.keys2r" : "favor.keys2";
  {
    ProfScope ps(l1, s);
    if (ragged) {
      if (Nc <= 16) hipLaunchKernelGGL((fc::keys1_ragged_kernel<1>), dim3(T * H, st.nch), dim3(256), 0, s, a, lens);
      else hipLaunchKernelGGL((fc::keys1_ragged_kernel<2>), dim3(T * H, st.nch), dim3(256), 0, s, a, lens);
    } else {
      if (Nc <= 16) hipLaunchKernelGGL((fc::keys1_kernel<1>), dim3(T * H, st.nch), dim3(256), 0, s, a);
      else hipLaunchKernelGGL((fc::keys1_kernel<2>), dim3(T * H, st.nch), dim3(256), 0, s, a);
    }
  }
  MLHOT_TRY(check_launch(l1));
  {
    ProfScope ps(l2, s);
    if (ragged) hipLaunchKernelGGL(fc::keys2_ragged_kernel, dim3(T * H), dim3(256), 0, s, a, lens);
    else hipLaunchKernelGGL(fc::keys2_kernel, dim3(T * H), dim3(256), 0, s, a);
  }
  return check_launch(l2);
#endif
}

inline int favor_keys_forward(const float* k, const float* proj, int T, int H, int Nc, int d, int m, void* state, size_t state_bytes,
                              hipStream_t s) {
  return favor_keys_launch("favor_keys_fwd", k, proj, nullptr, false, T, H, Nc, d, m, state, state_bytes, s);
}

// lens[T] int32 on the device, read there: no host synchronisation, so the call stays capturable
inline int favor_keys_ragged_forward(const float* k, const float* proj, const int32_t* lens, int T, int H, int Nc, int d, int m, void* state,
                                     size_t state_bytes, hipStream_t s) {
  return favor_keys_launch("favor_keys_ragged_fwd", k, proj, lens, true, T, H, Nc, d, m, state, state_bytes, s);
}

// w == nullptr with weights == false: mlhot_favor_query_fwd; otherwise mlhot_favor_query_weights_fwd - the same launch with the
// read-out instantiation, which also writes w [T][H][Nq][Nc] (4-byte aligned, as every float*)
inline int favor_query_launch(const char* what, const float* q, const void* state, const float* v, const float* proj, int T, int H, int Nq, int Nc, int d,
                              int m, float* out, float* w, bool weights, void* ws, size_t ws_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !q || !state || !v || !proj || !out || (weights && !w)) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_cached_ok(T, H, Nc, d, m)) {
    set_error("%s serves Nc <= 32, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < favor_query_ws_need(T, H, Nq, Nc, d, m)) { set_error("%s: workspace too small", what); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fc::QT - 1) / fc::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return MLHOT_ERR_ARG; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: q, proj and state must be 16-byte aligned", what); return MLHOT_ERR_ARG; }
  if (weights && (reinterpret_cast<uintptr_t>(w) & 3) != 0) { set_error("%s: w must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  const fc::State st = fc::carve_state(T, H, Nc, m, const_cast<void*>(state));
  fc::Args a = fc::make_args(T, H, Nq, Nc, d, m, st);
  a.x = q; a.proj = proj; a.v = v; a.out = out; a.ntile = (int)ntile;
  const char* label = weights ? "favor.queryw" : "favor.query";
  ProfScope ps(label, s);
  if (weights) hipLaunchKernelGGL(fc::query_weights_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a, w);
  else hipLaunchKernelGGL(fc::query_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a);
  return check_launch(label);
#endif
}

inline int favor_query_forward(const float* q, const void* state, const float* v, const float* proj, int T, int H, int Nq, int Nc, int d, int m,
                               float* out, void* ws, size_t ws_bytes, hipStream_t s) {
  return favor_query_launch("favor_query_fwd", q, state, v, proj, T, H, Nq, Nc, d, m, out, nullptr, false, ws, ws_bytes, s);
}

// the same with FAVOR+'s per-shot weights w = S / D read out beside out
inline int favor_query_weights_forward(const float* q, const void* state, const float* v, const float* proj, int T, int H, int Nq, int Nc, int d,
                                       int m, float* out, float* w, void* ws, size_t ws_bytes, hipStream_t s) {
  return favor_query_launch("favor_query_weights_fwd", q, state, v, proj, T, H, Nq, Nc, d, m, out, w, true, ws, ws_bytes, s);
}

// mlhot_favor_query_masked_fwd: G context masks per target row in one launch - mask [T][G][Nq] words on the
// device, out [T][G][Nq][d H], w [T][G][H][Nq][Nc] or nullptr.  Envelope, workspace, alignment and codes are favor_query_launch's.
inline int favor_query_masked_forward(const float* q, const void* state, const float* v, const float* proj, const uint32_t* mask, int G, int T, int H,
                                      int Nq, int Nc, int d, int m, float* out, float* w, void* ws, size_t ws_bytes, hipStream_t s) {
  const char* what = "favor_query_masked_fwd";
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || G < 1 || !q || !state || !v || !proj || !out || !mask) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  if (!favor_cached_ok(T, H, Nc, d, m)) {
    set_error("%s serves Nc <= 32, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)w; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < favor_query_ws_need(T, H, Nq, Nc, d, m)) { set_error("%s: workspace too small", what); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fc::QT - 1) / fc::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return MLHOT_ERR_ARG; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("%s: q, proj and state must be 16-byte aligned", what); return MLHOT_ERR_ARG; }
  if ((reinterpret_cast<uintptr_t>(mask) & 3) != 0 || (w && (reinterpret_cast<uintptr_t>(w) & 3) != 0)) { set_error("%s: mask_words and w must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  const fc::State st = fc::carve_state(T, H, Nc, m, const_cast<void*>(state));
  fc::Args a = fc::make_args(T, H, Nq, Nc, d, m, st);
  a.x = q; a.proj = proj; a.v = v; a.out = out; a.ntile = (int)ntile;
  const char* label = w ? "favor.querymw" : "favor.querym";
  ProfScope ps(label, s);
  if (w) hipLaunchKernelGGL(fc::query_masked_weights_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a, mask, G, w);
  else hipLaunchKernelGGL(fc::query_masked_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a, mask, G);
  return check_launch(label);
#endif
}

}  // namespace mlhot
