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

namespace mlhot {

// favor2.h's envelope on the context side; nothing bounds the number of query rows
inline bool favor_cached_ok(int T, int H, int Nc, int d, int m) {
#ifdef MLHOT_HOSTSIM
  (void)T; (void)H; (void)Nc; (void)d; (void)m; return false;
#else
  return T >= 1 && H >= 1 && Nc >= 1 && Nc <= 32 && d >= 16 && d % 16 == 0 && d <= 256 && m >= 16 && m <= 1536 &&
         (long long)T * H < (1 << 20);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace fc {

using fv::f32x4_t;
using fv::mfma4;

constexpr int QT = 16;                    // query rows per workgroup
constexpr int MAXNC = 32, MAXD = 256, MAXM = 1536;
constexpr int NT = 4;                     // 16-feature tiles per wave and trip of the dd loop
constexpr int WF = 16 * NT;               // features per wave and trip
constexpr int KCH = 4 * WF;               // features per K1 workgroup
constexpr int LDX = MAXD + 8;             // LDS row stride of the scaled rows: 8 mod 32, so a b128 read of lanes (lr, lq) is conflict-free
constexpr int ldf(int mp) { return (mp + 31) / 32 * 32 + 8; }      // LDS row stride of dd / F_q, 8 mod 32 as well
constexpr int LDS_S = MAXNC + 1;

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
  float c, ratio, re;                     // d^-1/4, m^-1/2, ratio * 1e-4
};

// acc[i][j] = rows 16 i .. of xs (LDS, scaled by c, stride LDX) times features f0 + 16 j .. of proj: per element ONE chain over
// k = 0, 16, 32, .. (each step four MFMAs: k + {0, 4, 8, 12}, then + 1, + 2, + 3) - favor2.h's F1 order.  The proj loads of 64 k are in flight together.
template <int RT>
__device__ __forceinline__ void dd_tiles(const float* xs, const float* proj, int d, int m, int f0, int lr, int lq, f32x4_t (&acc)[RT][NT]) {
  const float* pr[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) { const int fj = f0 + 16 * j + lr; pr[j] = fj < m ? proj + (size_t)fj * d + 4 * lq : nullptr; }
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  constexpr int UF = 4;
  for (int c0 = 0; c0 < d; c0 += 16 * UF) {
    float4 bv[UF][NT];
#pragma unroll
    for (int u = 0; u < UF; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        bv[u][j] = (c0 + 16 * u < d && pr[j]) ? *reinterpret_cast<const float4*>(pr[j] + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int k0 = c0 + 16 * u;
      float4 av[RT];
#pragma unroll
      for (int i = 0; i < RT; ++i)
        av[i] = k0 < d ? *reinterpret_cast<const float4*>(xs + (16 * i + lr) * LDX + k0 + 4 * lq) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[i][j] = mfma4(av[i].x, bv[u][j].x, acc[i][j]); acc[i][j] = mfma4(av[i].y, bv[u][j].y, acc[i][j]);
          acc[i][j] = mfma4(av[i].z, bv[u][j].z, acc[i][j]); acc[i][j] = mfma4(av[i].w, bv[u][j].w, acc[i][j]);
        }
    }
  }
}

// c * row into xs[r][0 .. d) and the row's sum of squares: PER threads per row, thread `part` takes the float4 at 4 part + 4 PER k
// (k = 0, 1, .. in order), then a butterfly over the PER lanes.  xrow == nullptr: zeros; xs_row == nullptr: the sum only.  Every lane
// returns the row's sum.
template <int PER>
__device__ __forceinline__ float stage_row(const float* xrow, float* xs_row, int d, int part, float c) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXD / (4 * PER); ++k) {
    const int e = 4 * part + 4 * PER * k;
    if (e < d) {
      const float4 u = xrow ? *reinterpret_cast<const float4*>(xrow + e) : make_float4(0.f, 0.f, 0.f, 0.f);
      s += (u.x * u.x + u.y * u.y) + (u.z * u.z + u.w * u.w);
      if (xs_row) *reinterpret_cast<float4*>(xs_row + e) = make_float4(c * u.x, c * u.y, c * u.z, c * u.w);
    }
  }
#pragma unroll
  for (int off = 1; off < PER; off <<= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// ---- keys, launch 1: dd_k into the state, the workgroup's maximum ------------------------------------------------------------
// RAG (mlhot_favor_keys_ragged_fwd): row n of task t is a context shot iff n < lens[t].  Rows behind it are never
// read (they are staged as zeros), never stored and never enter the maximum - selected by row index, so a NaN there goes nowhere;
// a 16-row tile wholly behind lens[t] skips its MFMAs (lens[t] is one scalar per workgroup: wave-uniform).  K2 writes their zeros.
// RAG == false is the code of mlhot_favor_keys_fwd as it was: `len` is Nc at compile time and every masked branch folds away.
template <int RTA, bool RAG>
__device__ __forceinline__ float keys1_store(const f32x4_t (&acc)[RTA][NT], const Args& a, int th, int f0, int lr, int lq, int len, float best) {
  const int m = a.m, mp = a.mp, Nc = a.Nc;
#pragma unroll
  for (int i = 0; i < RTA; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * i + 4 * lq + r;
      if (row >= (RAG ? len : Nc)) continue;
      float* drow = a.fkw + ((size_t)th * Nc + row) * mp;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int fj = f0 + 16 * j + lr;
        if (fj < mp) drow[fj] = fj < m ? acc[i][j][r] : 0.f;
        if (fj < m) best = fmaxf(best, acc[i][j][r]);
      }
    }
  return best;
}

// lens[t] held to 1 .. Nc: the host checks the values (mlhot.ops.favor_keys); the clamp keeps every index in bounds whatever arrives
__device__ __forceinline__ int ragged_len(const int32_t* lens, int t, int Nc) { return min(max((int)lens[t], 1), Nc); }

template <int RT, bool RAG>
__device__ __forceinline__ void keys1_body(const Args& a, const int32_t* lens) {
  __shared__ __attribute__((aligned(16))) float xs[16 * RT * LDX];
  __shared__ float s_w[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x, t = th / a.H, h = th % a.H, chunk = blockIdx.y;
  const int d = a.d, m = a.m, Nc = a.Nc, mp = a.mp;
  const int len = RAG ? ragged_len(lens, t, Nc) : Nc;
  for (int r = tid >> 3; r < 16 * RT; r += 32) {
    const float* xrow = r < len ? a.x + ((size_t)(t * Nc + r) * a.H + h) * d : nullptr;
    stage_row<8>(xrow, xs + r * LDX, d, tid & 7, a.c);
  }
  __syncthreads();
  const int f0 = chunk * KCH + wv * WF;
  float best = -INFINITY;
  if (f0 < mp) {
    if (RAG && RT == 2 && len <= 16) {          // the second tile holds no context shot: the first tile's chains alone, the same per element
      f32x4_t acc[1][NT];
      dd_tiles<1>(xs, a.proj, d, m, f0, lr, lq, acc);
      best = keys1_store<1, RAG>(acc, a, th, f0, lr, lq, len, best);
    } else {
      f32x4_t acc[RT][NT];
      dd_tiles<RT>(xs, a.proj, d, m, f0, lr, lq, acc);
      best = keys1_store<RT, RAG>(acc, a, th, f0, lr, lq, len, best);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if (lane == 0) s_w[wv] = best;
  __syncthreads();
  if (tid == 0) a.part[(size_t)th * a.nch + chunk] = fmaxf(fmaxf(s_w[0], s_w[1]), fmaxf(s_w[2], s_w[3]));
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
  __shared__ float s_w[4], s_diag[MAXNC];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int th = blockIdx.x, t = th / a.H, h = th % a.H;
  const int d = a.d, m = a.m, Nc = a.Nc, mp = a.mp;
  const int len = RAG ? ragged_len(lens, t, Nc) : Nc;
  float best = -INFINITY;
  for (int i = tid; i < a.T * a.H * a.nch; i += 256) best = fmaxf(best, a.part[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if (lane == 0) s_w[wv] = best;
  {
    const int r = tid >> 3;            // 32 rows x 8 threads
    const float* xrow = r < len ? a.x + ((size_t)(t * Nc + r) * a.H + h) * d : nullptr;
    const float s = stage_row<8>(xrow, nullptr, d, tid & 7, 0.f);
    if (r < Nc && (tid & 7) == 0) s_diag[r] = 0.5f * a.c * a.c * s;
  }
  __syncthreads();
  const float M = fmaxf(fmaxf(s_w[0], s_w[1]), fmaxf(s_w[2], s_w[3]));
  if (th == 0 && tid == 0) a.M[0] = M;
  const int q4 = mp / 4;
  float* blk = a.fkw + (size_t)th * Nc * mp;
  for (int idx = tid; idx < Nc * q4; idx += 256) {
    const int row = idx / q4, j = 4 * (idx - row * q4);
    if (RAG && row >= len) { *reinterpret_cast<float4*>(blk + (size_t)row * mp + j) = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
    const float sub = s_diag[row] + M;
    float4 e = *reinterpret_cast<const float4*>(blk + (size_t)row * mp + j);
    e.x = j < m ? a.ratio * expf(e.x - sub) + a.re : 0.f; e.y = j + 1 < m ? a.ratio * expf(e.y - sub) + a.re : 0.f;
    e.z = j + 2 < m ? a.ratio * expf(e.z - sub) + a.re : 0.f; e.w = j + 3 < m ? a.ratio * expf(e.w - sub) + a.re : 0.f;
    *reinterpret_cast<float4*>(blk + (size_t)row * mp + j) = e;
  }
}

__global__ __launch_bounds__(256) void keys2_kernel(const Args a) { keys2_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void keys2_ragged_kernel(const Args a, const int32_t* lens) { keys2_body<true>(a, lens); }

// ---- query: one workgroup per (task, head, 16 query rows) -------------------------------------------------------------------
__global__ __launch_bounds__(256) void query_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ldf(MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * LDS_S], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, m = a.m, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp, LD = ldf(mp);
  // 1. c q into LDS, diag = 0.5 c^2 |q|^2: 16 threads per row
  {
    const int r = tid >> 4, n = n0 + r;
    const float* xrow = n < Nq ? a.x + (((size_t)t * Nq + n) * H + h) * d : nullptr;
    const float s = stage_row<16>(xrow, xs + r * LDX, d, tid & 15, a.c);
    if ((tid & 15) == 0) s_diag[r] = 0.5f * a.c * a.c * s;
  }
  __syncthreads();
  // 2. dd into LDS, row maxima: wave w takes the 64-feature groups w, w + 4, ..
  {
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int f0 = wv * WF; f0 < mp; f0 += 4 * WF) {
      f32x4_t acc[1][NT];
      dd_tiles<1>(xs, a.proj, d, m, f0, lr, lq, acc);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int fj = f0 + 16 * j + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (fj < mp) s_f[(4 * lq + r) * LD + fj] = fj < m ? acc[0][j][r] : 0.f;
          if (fj < m) best[r] = fmaxf(best[r], acc[0][j][r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) best[r] = fmaxf(best[r], __shfl_xor(best[r], off, 64));
      if (lr == 0) s_pm[wv][4 * lq + r] = best[r];
    }
  }
  __syncthreads();
  // 3. F_q = ratio exp(dd - diag - rowmax) + ratio 1e-4 in place, zeros at features >= m
  {
    const int q4 = mp / 4;
    for (int idx = tid; idx < QT * q4; idx += 256) {
      const int row = idx / q4, j = 4 * (idx - row * q4);
      const float sub = s_diag[row] + fmaxf(fmaxf(s_pm[0][row], s_pm[1][row]), fmaxf(s_pm[2][row], s_pm[3][row]));
      float4 e = *reinterpret_cast<const float4*>(s_f + row * LD + j);
      e.x = j < m ? a.ratio * expf(e.x - sub) + a.re : 0.f; e.y = j + 1 < m ? a.ratio * expf(e.y - sub) + a.re : 0.f;
      e.z = j + 2 < m ? a.ratio * expf(e.z - sub) + a.re : 0.f; e.w = j + 3 < m ? a.ratio * expf(e.w - sub) + a.re : 0.f;
      *reinterpret_cast<float4*>(s_f + row * LD + j) = e;
    }
  }
  __syncthreads();
  // 4. S = F_q F_k^T: wave w takes the 16-feature chunks w, w + 4, .. (four in flight), ascending; then the waves fold 0, 1, 2, 3
  {
    const int tk = (Nc + 15) / 16, nch16 = mp / 16;
    const float* krow[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + ((size_t)th * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
    f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int ch = wv; ch < nch16; ch += 16) {
      float4 fb[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          fb[u][jj] = (ch + 4 * u < nch16 && krow[jj]) ? *reinterpret_cast<const float4*>(krow[jj] + 16 * (ch + 4 * u)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ch + 4 * u >= nch16) break;
        const float4 fa = *reinterpret_cast<const float4*>(s_f + lr * LD + 16 * (ch + 4 * u) + 4 * lq);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          if (jj >= tk) continue;
          acc[jj] = mfma4(fa.x, fb[u][jj].x, acc[jj]); acc[jj] = mfma4(fa.y, fb[u][jj].y, acc[jj]);
          acc[jj] = mfma4(fa.z, fb[u][jj].z, acc[jj]); acc[jj] = mfma4(fa.w, fb[u][jj].w, acc[jj]);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) *reinterpret_cast<f32x4_t*>(red + ((wv * 2 + jj) * 64 + lane) * 4) = acc[jj];
  }
  __syncthreads();
  if (wv < 2) {
    const int jj = wv;
    f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4_t vv = *reinterpret_cast<const f32x4_t*>(red + ((k * 2 + jj) * 64 + lane) * 4);
      s[0] += vv[0]; s[1] += vv[1]; s[2] += vv[2]; s[3] += vv[3];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int np = 16 * jj + lr;
      if (np < Nc) s_S[(4 * lq + r) * LDS_S + np] = s[r];
    }
  }
  __syncthreads();
  if (tid < QT) {
    float s = 0.f;
    for (int np = 0; np < Nc; ++np) s += s_S[tid * LDS_S + np];
    s_D[tid] = s;
  }
  __syncthreads();
  // 5. out[t][n][e H + h] = sum_n' S[n][n'] v[(t, n', h)][e] / D[n]: wave = 16-channel tiles of e, K = 32 key slots (zeros beyond Nc)
  for (int et = wv; et * 16 < d; et += 4) {
    const int e = 16 * et + lr;
    float bv[MAXNC / 4];
#pragma unroll
    for (int ks = 0; ks < MAXNC / 4; ++ks) { const int np = 4 * ks + lq; bv[ks] = np < Nc ? a.v[((size_t)(t * Nc + np) * H + h) * d + e] : 0.f; }
    f32x4_t o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < MAXNC / 4; ++ks) {
      const int np = 4 * ks + lq;
      o = mfma4(np < Nc ? s_S[lr * LDS_S + np] : 0.f, bv[ks], o);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * lq + r;
      if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o[r] / s_D[4 * lq + r];
    }
  }
}

inline Args make_args(int T, int H, int Nq, int Nc, int d, int m, const State& st) {
  Args a{};
  a.T = T; a.H = H; a.Nq = Nq; a.Nc = Nc; a.d = d; a.m = m; a.mp = st.mp; a.nch = st.nch;
  a.fk = st.fk; a.fkw = st.fk; a.M = st.M; a.part = st.part;
  a.c = powf((float)d, -0.25f); a.ratio = 1.0f / sqrtf((float)m); a.re = a.ratio * 1e-4f;
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

#ifndef MLHOT_HOSTSIM
inline bool fc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
#endif

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
  if (!fc_aligned16(k) || !fc_aligned16(proj) || !fc_aligned16(state)) { set_error("%s: k, proj and state must be 16-byte aligned", what); return MLHOT_ERR_ARG; }
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

inline int favor_query_forward(const float* q, const void* state, const float* v, const float* proj, int T, int H, int Nq, int Nc, int d, int m,
                               float* out, void* ws, size_t ws_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !q || !state || !v || !proj || !out) { set_error("favor_query_fwd: bad argument"); return MLHOT_ERR_ARG; }
  if (!favor_cached_ok(T, H, Nc, d, m)) {
    set_error("favor_query_fwd serves Nc <= 32, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < favor_query_ws_need(T, H, Nq, Nc, d, m)) { set_error("favor_query_fwd: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fc::QT - 1) / fc::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("favor_query_fwd: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)"); return MLHOT_ERR_ARG; }
  if (!fc_aligned16(q) || !fc_aligned16(proj) || !fc_aligned16(state)) { set_error("favor_query_fwd: q, proj and state must be 16-byte aligned"); return MLHOT_ERR_ARG; }
  const fc::State st = fc::carve_state(T, H, Nc, m, const_cast<void*>(state));
  fc::Args a = fc::make_args(T, H, Nq, Nc, d, m, st);
  a.x = q; a.proj = proj; a.v = v; a.out = out; a.ntile = (int)ntile;
  ProfScope ps("favor.query", s);
  hipLaunchKernelGGL(fc::query_kernel, dim3((unsigned)(ntile * T * H)), dim3(256), 0, s, a);
  return check_launch("favor.query");
#endif
}

}  // namespace mlhot
