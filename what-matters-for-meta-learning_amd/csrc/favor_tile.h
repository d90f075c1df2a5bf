// The tile steps of the FAVOR+ inference kernels, each ONCE: favor_cached.h (keys, query), favor_summary.h (absorb, query),
// favor_prefix_long.h (dd, sweep), favor_linear.h (apply), favor_long.h (keys, query), np_query.h and np_prefix.h (the attention part) are sequences of these
// calls plus what is their own.  The bits of one kernel are defined as equal to another's (tests compare them with torch.equal):
// they are, because both run the same text here.  Every step keeps ONE order of its floating-point operations, a function of the
// dimensions alone; the __shared__ arrays stay declared in the kernels and are passed in.
// v_mfma_f32_16x16x4_f32: A lane l = A[l&15][l>>4], B lane l = B[l>>4][l&15], C/D lane l reg r = C[4*(l>>4)+r][l&15]; a float4 of 4
// consecutive k per lane feeds 4 MFMAs whose lane-group lq covers k0 + 4 lq + i - the same permutation on both operands.
// Lane names throughout: tid the thread, wv its wave (uniform), lane = tid & 63, lr = lane & 15, lq = lane >> 4.
#pragma once
#include "common.h"

#ifndef MLHOT_HOSTSIM
namespace mlhot {
namespace ft {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4_t mfma4(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int QT = 16;                    // query rows per workgroup
constexpr int MAXNC = 32, MIND = 16, MAXD = 256, MINM = 16, MAXM = 1536;
constexpr int NT = 4;                     // 16-feature tiles per wave and trip of the dd loop
constexpr int WF = 16 * NT;               // features per wave and trip
constexpr int KCH = 4 * WF;               // features per key-side workgroup
constexpr int LDX = MAXD + 8;             // LDS row stride of a [16 x d] tile: 8 mod 32, so a b128 read of lanes (lr, lq) is conflict-free
constexpr int ldf(int mp) { return (mp + 31) / 32 * 32 + 8; }      // LDS row stride of dd / F, 8 mod 32 as well
constexpr int LDS_S = MAXNC + 1;
constexpr int ldo(int d) { return d + 4; }  // row stride of a wave's partial [16 x d] tile in LDS
constexpr float EPS = 1e-4f;              // the feature's floor, relative to ratio (fast_attention.py:96-97)

struct Scales {                           // d^-1/4, m^-1/2, ratio * 1e-4
  float c, ratio, re;
  Scales() = default;
  Scales(int d, int m) : c(powf((float)d, -0.25f)), ratio(1.0f / sqrtf((float)m)), re(ratio * EPS) {}
};
inline bool dims_ok(int d, int m) { return d >= MIND && d % 16 == 0 && d <= MAXD && m >= MINM && m <= MAXM; }
// what every kernel here serves; the entries add their own terms (shot counts, grids)
inline bool envelope_ok(int T, int H, int d, int m) { return T >= 1 && H >= 1 && dims_ok(d, m) && (long long)T * H < (1 << 20); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lens[t] held to lo .. hi: the host checks the values; the clamp keeps every index in bounds whatever arrives.  NULL: hi
__device__ __forceinline__ int clamp_len(const int32_t* lens, int t, int lo, int hi) { return lens ? min(max((int)lens[t], lo), hi) : hi; }
__device__ __forceinline__ float max4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }
__device__ __forceinline__ float wave_max(float best) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  return best;
}
// s_w[wave] = the maximum of part[0 .. n) over this wave's share; after a barrier max4 of s_w is the workgroup's
__device__ __forceinline__ void part_max(const float* part, int n, float* s_w, int tid) {
  float best = -INFINITY;
  for (int i = tid; i < n; i += 256) best = fmaxf(best, part[i]);
  best = wave_max(best);
  if ((tid & 63) == 0) s_w[tid >> 6] = best;
}
// the feature of four neighbours from their dd: ratio exp(dd - sub) + re, zeros at features >= m (selected by index)
__device__ __forceinline__ float4 feature4(float4 e, float sub, int j, int m, const Scales& sc) {
  e.x = j < m ? sc.ratio * expf(e.x - sub) + sc.re : 0.f; e.y = j + 1 < m ? sc.ratio * expf(e.y - sub) + sc.re : 0.f;
  e.z = j + 2 < m ? sc.ratio * expf(e.z - sub) + sc.re : 0.f; e.w = j + 3 < m ? sc.ratio * expf(e.w - sub) + sc.re : 0.f;
  return e;
}
// the same without ratio and floor: exp(dd - sub), zeros at features >= m
__device__ __forceinline__ float4 exp4(float4 e, float sub, int j, int m) {
  e.x = j < m ? expf(e.x - sub) : 0.f; e.y = j + 1 < m ? expf(e.y - sub) : 0.f;
  e.z = j + 2 < m ? expf(e.z - sub) : 0.f; e.w = j + 3 < m ? expf(e.w - sub) : 0.f;
  return e;
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

// ---- key side ----------------------------------------------------------------------------------------------------------------------
// A wave's dd tiles into rows of ddb (row stride mp): rows >= len are not stored and enter no maximum, features in [m, mp) are
// zeros.  PERROW: best[i][r] is row 16 i + 4 lq + r's maximum over this lane's features; otherwise best[0][0] is the lane's.
template <int RTA, bool PERROW>
__device__ __forceinline__ void dd_store(const f32x4_t (&acc)[RTA][NT], float* ddb, int mp, int m, int f0, int lr, int lq, int len,
                                         float (&best)[PERROW ? 2 : 1][PERROW ? 4 : 1]) {
#pragma unroll
  for (int i = 0; i < RTA; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * i + 4 * lq + r;
      if (row >= len) continue;
      float* drow = ddb + (size_t)row * mp;
      float& b = best[PERROW ? i : 0][PERROW ? r : 0];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int fj = f0 + 16 * j + lr;
        if (fj < mp) drow[fj] = fj < m ? acc[i][j][r] : 0.f;
        if (fj < m) b = fmaxf(b, acc[i][j][r]);
      }
    }
}

// dd of up to 16 RT key rows for the feature chunk blockIdx.y (KCH features, WF per wave): krow(r) is row r's pointer, rows >= len
// are staged as zeros and never read - selected by row index, so a NaN there goes nowhere.  With at most 16 valid rows of 32 the
// second tile holds no shot: the first tile's chains alone, the same per element (len is one scalar per workgroup: wave-uniform).
// The maxima go to part: one float for the workgroup, or (PERROW) one per row, -inf where the row is behind len.
// MASKED == false: len is the caller's row count, at least 1 and above 16 where RT == 2 - the two tests on it fold away.
// LDS: xs [16 RT][LDX]; s_w [4], PERROW [4][32].
template <int RT, bool PERROW, bool MASKED, class Row>
__device__ __forceinline__ void keys_dd(Row krow, int len, const float* proj, float c, int d, int m, int mp, float* ddb, float* part, float* xs, float* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  for (int r = tid >> 3; r < 16 * RT; r += 32) stage_row<8>(r < len ? krow(r) : nullptr, xs + r * LDX, d, tid & 7, c);
  __syncthreads();
  const int f0 = blockIdx.y * KCH + wv * WF;
  float best[PERROW ? 2 : 1][PERROW ? 4 : 1];
#pragma unroll
  for (int i = 0; i < (PERROW ? 2 : 1); ++i)
#pragma unroll
    for (int r = 0; r < (PERROW ? 4 : 1); ++r) best[i][r] = -INFINITY;
  if (f0 < mp && (!MASKED || len > 0)) {
    if (MASKED && RT == 2 && len <= 16) {
      f32x4_t acc[1][NT];
      dd_tiles<1>(xs, proj, d, m, f0, lr, lq, acc);
      dd_store<1, PERROW>(acc, ddb, mp, m, f0, lr, lq, len, best);
    } else {
      f32x4_t acc[RT][NT];
      dd_tiles<RT>(xs, proj, d, m, f0, lr, lq, acc);
      dd_store<RT, PERROW>(acc, ddb, mp, m, f0, lr, lq, len, best);
    }
  }
  if constexpr (PERROW) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) best[i][r] = fmaxf(best[i][r], __shfl_xor(best[i][r], off, 64));
        if (lr == 0) s_w[wv * 32 + 16 * i + 4 * lq + r] = best[i][r];
      }
    __syncthreads();
    if (tid < 32) part[tid] = max4(s_w[tid], s_w[32 + tid], s_w[64 + tid], s_w[96 + tid]);
  } else {
    const float b = wave_max(best[0][0]);
    if (lane == 0) s_w[wv] = b;
    __syncthreads();
    if (tid == 0) part[0] = max4(s_w[0], s_w[1], s_w[2], s_w[3]);
  }
}

// diag = 0.5 c^2 |k|^2 of 32 key rows: 8 threads per row (thread tid's row is tid >> 3), every one of them returns it
__device__ __forceinline__ float key_diag(const float* xrow, int d, float c, int tid) {
  return 0.5f * c * c * stage_row<8>(xrow, nullptr, d, tid & 7, 0.f);
}

// ---- query side: F of 16 rows in LDS ---------------------------------------------------------------------------------------------------
// s_pm[wave][row] = the maximum over the 16 lanes that hold row 4 lq + r's elements of this wave
__device__ __forceinline__ void rowmax_fold(float (&best)[4], float (*s_pm)[QT], int wv, int lr, int lq) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) best[r] = fmaxf(best[r], __shfl_xor(best[r], off, 64));
    if (lr == 0) s_pm[wv][4 * lq + r] = best[r];
  }
}

// F = ratio exp(dd - diag - rowmax) + ratio 1e-4 in place (s_f, row stride LD), zeros at features >= m
__device__ __forceinline__ void features_inplace(float* s_f, int LD, int m, int mp, const float* s_diag, const float (*s_pm)[QT], const Scales& sc, int tid) {
  const int q4 = mp / 4;
  for (int idx = tid; idx < QT * q4; idx += 256) {
    const int row = idx / q4, j = 4 * (idx - row * q4);
    const float sub = s_diag[row] + max4(s_pm[0][row], s_pm[1][row], s_pm[2][row], s_pm[3][row]);
    float4* at = reinterpret_cast<float4*>(s_f + row * LD + j);
    *at = feature4(*at, sub, j, m, sc);
  }
}

// The front half of every query kernel, barriers included; qrow(r) is the tile's row r or nullptr (zeros):
//   1. c q into xs, diag = 0.5 c^2 |q|^2: 16 threads per row
//   2. dd into s_f (row stride ldf(mp)) with the row maxima: wave w takes the 64-feature groups w, w + 4, ..
//   3. F_q in place
template <class Row>
__device__ __forceinline__ void query_front(Row qrow, const float* proj, int d, int m, int mp, const Scales& sc, float* xs, float* s_f, float* s_diag,
                                            float (*s_pm)[QT]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int LD = ldf(mp);
  {
    const int r = tid >> 4;
    const float s = stage_row<16>(qrow(r), xs + r * LDX, d, tid & 15, sc.c);
    if ((tid & 15) == 0) s_diag[r] = 0.5f * sc.c * sc.c * s;
  }
  __syncthreads();
  {
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int f0 = wv * WF; f0 < mp; f0 += 4 * WF) {
      f32x4_t acc[1][NT];
      dd_tiles<1>(xs, proj, d, m, f0, lr, lq, acc);
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
    rowmax_fold(best, s_pm, wv, lr, lq);
  }
  __syncthreads();
  features_inplace(s_f, LD, m, mp, s_diag, s_pm, sc, tid);
  __syncthreads();
}

// N sums over a row's features at once: 16 threads per row, thread p calls term(j, s) for j = p, p + 16, .. in order, then a
// butterfly over the 16 lanes (commutative at every level: every lane ends with the same bits)
template <int N, class Term>
__device__ __forceinline__ void row_sums(int mp, int p, float (&s)[N], Term term) {
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = 0.f;
  for (int j = p; j < mp; j += 16) term(j, s);
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += __shfl_xor(s[i], off, 64);
}

// ---- S = F B^T against up to 32 rows of B ----------------------------------------------------------------------------------------------
// S[16][ncol] into s_S: brow[jj] = row 16 jj + lr of B at its element 4 lq (row stride irrelevant here; nullptr: zeros), tk the
// 16-row tiles of B in use, nch16 the 16-feature chunks.  Wave w takes the chunks w, w + 4, .. ascending (four in flight); the B
// operand of chunk feature f is bt(jj, f, on, the loaded float4); the partials go to red [4][2][64][4] and the waves fold 0, 1, 2, 3.
// Two barriers inside; s_S holds the columns < ncol behind the second.
struct BPlain { __device__ __forceinline__ float4 operator()(int, int, bool, float4 b) const { return b; } };
template <class BT>
__device__ __forceinline__ void s_tile(const float* s_f, int LD, const float* const (&brow)[2], int tk, int nch16, int ncol, BT bt, float* red, float* s_S) {
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  {
    f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int ch = wv; ch < nch16; ch += 16) {
      float4 fb[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          fb[u][jj] = (ch + 4 * u < nch16 && brow[jj]) ? *reinterpret_cast<const float4*>(brow[jj] + 16 * (ch + 4 * u)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ch + 4 * u >= nch16) break;
        const int j0 = 16 * (ch + 4 * u) + 4 * lq;
        const float4 fa = *reinterpret_cast<const float4*>(s_f + lr * LD + j0);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          if (jj >= tk) continue;
          const float4 b = bt(jj, j0, brow[jj] != nullptr, fb[u][jj]);
          acc[jj] = mfma4(fa.x, b.x, acc[jj]); acc[jj] = mfma4(fa.y, b.y, acc[jj]);
          acc[jj] = mfma4(fa.z, b.z, acc[jj]); acc[jj] = mfma4(fa.w, b.w, acc[jj]);
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
      if (np < ncol) s_S[(4 * lq + r) * LDS_S + np] = s[r];
    }
  }
  __syncthreads();
}

// D = rowsum(S): the Nc columns in order; one barrier behind it
__device__ __forceinline__ void s_rowsum(const float* s_S, int Nc, float* s_D) {
  const int tid = threadIdx.x;
  if (tid < QT) {
    float s = 0.f;
    for (int np = 0; np < Nc; ++np) s += s_S[tid * LDS_S + np];
    s_D[tid] = s;
  }
  __syncthreads();
}

// The value rows of channel e for this lane's key slots 4 ks + lq (v0 = slot 0's row, vld floats between slots; zeros from Nc on),
// and S[:, :cut] V as ONE chain over the 32 key slots (zeros from cut on, selected by index)
__device__ __forceinline__ void load_v(float (&bv)[MAXNC / 4], const float* v0, size_t vld, int Nc, int e, int lq, bool on = true) {
#pragma unroll
  for (int ks = 0; ks < MAXNC / 4; ++ks) { const int np = 4 * ks + lq; bv[ks] = on && np < Nc ? v0[np * vld + e] : 0.f; }
}
__device__ __forceinline__ f32x4_t sv_chain(const float* s_S, const float (&bv)[MAXNC / 4], int cut, int lr, int lq) {
  f32x4_t o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < MAXNC / 4; ++ks) {
    const int np = 4 * ks + lq;
    o = mfma4(np < cut ? s_S[lr * LDS_S + np] : 0.f, bv[ks], o);
  }
  return o;
}
// store(row, e, sum_n' S[row][n'] v[n'][e] / D[row]) for the tile's 16 rows: wave = the 16-channel tiles of e
template <class Store>
__device__ __forceinline__ void sv_tiles(const float* s_S, const float* s_D, const float* v0, size_t vld, int Nc, int d, int wv, int lr, int lq, Store store) {
  for (int et = wv; et * 16 < d; et += 4) {
    const int e = 16 * et + lr;
    float bv[MAXNC / 4];
    load_v(bv, v0, vld, Nc, e, lq);
    const f32x4_t o = sv_chain(s_S, bv, Nc, lr, lq);
#pragma unroll
    for (int r = 0; r < 4; ++r) store(4 * lq + r, e, o[r] / s_D[4 * lq + r]);
  }
}

// ---- the same three steps over a WIDE S tile: more than 32 key slots, walked in chunks of 32 (favor_long.h) -----------------------------
// s_S has row stride ld (odd, as LDS_S is).  Every sum keeps the order of its 32-slot twin above and carries on behind it: with at
// most 32 slots these run the twin's operations exactly.
// D = rowsum(S): the n columns in order; one barrier behind it
__device__ __forceinline__ void s_rowsum_wide(const float* s_S, int ld, int n, float* s_D) {
  const int tid = threadIdx.x;
  if (tid < QT) {
    float s = 0.f;
    for (int np = 0; np < n; ++np) s += s_S[tid * ld + np];
    s_D[tid] = s;
  }
  __syncthreads();
}
// load_v for the chunk of slots n0 .. n0 + 32 (zeros from n on)
__device__ __forceinline__ void load_v_at(float (&bv)[MAXNC / 4], const float* v0, size_t vld, int n0, int n, int e, int lq) {
#pragma unroll
  for (int ks = 0; ks < MAXNC / 4; ++ks) { const int np = n0 + 4 * ks + lq; bv[ks] = np < n ? v0[np * vld + e] : 0.f; }
}
// sv_chain continued: o carries the chain over the slots < n0, this adds the slots n0 .. n0 + 32 in order (zeros from cut on, by index)
__device__ __forceinline__ f32x4_t sv_chain_on(f32x4_t o, const float* s_S, int ld, const float (&bv)[MAXNC / 4], int n0, int cut, int lr, int lq) {
#pragma unroll
  for (int ks = 0; ks < MAXNC / 4; ++ks) {
    const int np = n0 + 4 * ks + lq;
    o = mfma4(np < cut ? s_S[lr * ld + np] : 0.f, bv[ks], o);
  }
  return o;
}
// sv_tiles over n slots: per element ONE chain over the slots in ascending order, the accumulator carried from chunk to chunk
template <class Store>
__device__ __forceinline__ void sv_tiles_wide(const float* s_S, int ld, const float* s_D, const float* v0, size_t vld, int n, int d, int wv, int lr, int lq, Store store) {
  for (int et = wv; et * 16 < d; et += 4) {
    const int e = 16 * et + lr;
    f32x4_t o = {0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < n; n0 += MAXNC) {
      float bv[MAXNC / 4];
      load_v_at(bv, v0, vld, n0, n, e, lq);
      o = sv_chain_on(o, s_S, ld, bv, n0, n, lr, lq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) store(4 * lq + r, e, o[r] / s_D[4 * lq + r]);
  }
}

// ---- the wide steps continued across PAGES of the wide tile (favor_paged.h) --------------------------------------------
// The wide tile holds one page of the slots at a time, its column 0 being slot p0.  D and the out chains carry on from page to page:
// each is still ONE chain over the slots in ascending order, so with a single page these run the wide steps' operations exactly.
// s_rowsum_wide continued: D = carry (nullptr: 0) + the page's n columns in order; carry may be s_D itself.  One barrier behind it
__device__ __forceinline__ void s_rowsum_page(const float* s_S, int ld, int n, float* s_D, const float* carry) {
  const int tid = threadIdx.x;
  if (tid < QT) {
    float s = carry ? carry[tid] : 0.f;
    for (int np = 0; np < n; ++np) s += s_S[tid * ld + np];
    s_D[tid] = s;
  }
  __syncthreads();
}
// sv_chain_on against a page: slot np is column np - p0 of s_S (zeros from cut on, by index)
__device__ __forceinline__ f32x4_t sv_chain_page(f32x4_t o, const float* s_S, int ld, const float (&bv)[MAXNC / 4], int n0, int p0, int cut, int lr, int lq) {
#pragma unroll
  for (int ks = 0; ks < MAXNC / 4; ++ks) {
    const int np = n0 + 4 * ks + lq;
    o = mfma4(np < cut ? s_S[lr * ld + np - p0] : 0.f, bv[ks], o);
  }
  return o;
}
// one channel tile's chain over the page's slots p0 .. pend (pend <= n, the task's slots): sv_tiles_wide's inner loop, o carried in
__device__ __forceinline__ f32x4_t sv_page(f32x4_t o, const float* s_S, int ld, const float* v0, size_t vld, int p0, int pend, int n, int e, int lr, int lq) {
  for (int n0 = p0; n0 < pend; n0 += MAXNC) {
    float bv[MAXNC / 4];
    load_v_at(bv, v0, vld, n0, n, e, lq);
    o = sv_chain_page(o, s_S, ld, bv, n0, p0, n, lr, lq);
  }
  return o;
}

// ---- masked read-outs: G groups of per-row context masks over ONE S tile -------------------------------------------
// s_Sm = S where the row's mask keeps the column, +0.0f elsewhere, over the first n columns (both tiles have row stride ld);
// word(row, c) is the row's mask word c - bit j = column 32 c + j - and 0 for a row that is not stored.  One barrier behind it.
// Every step above then runs on s_Sm unchanged: a masked sum IS the sum of the kept columns (a dropped one adds +0 in its place in
// the same order), never a difference; with every bit set s_Sm has S's bits and so has everything formed from it.
template <class Word>
__device__ __forceinline__ void s_mask(const float* s_S, float* s_Sm, int ld, int n, Word word) {
  const int nw = (n + 31) / 32 * 32;
  for (int idx = threadIdx.x; idx < QT * nw; idx += 256) {
    const int row = idx / nw, np = idx - row * nw;
    if (np < n) s_Sm[row * ld + np] = (word(row, np >> 5) >> (np & 31)) & 1u ? s_S[row * ld + np] : 0.f;
  }
  __syncthreads();
}
// x / D, and exact zero for a row whose mask kept no valid column (D == 0: every kept column of S is positive)
__device__ __forceinline__ float div_kept(float x, float D) { return D > 0.f ? x / D : 0.f; }

// ---- [16 x mp] [mp x d]: F in LDS against C streamed from memory -----------------------------------------------------------------------
// NG: 64-column groups of d.  A lane's float4 of C[j][64 g + 4 lr ..] serves four MFMAs whose 16 output columns are 64 g + 4 lr' + y.
// Wave w takes the 16-feature chunks w, w + 4, .. in ascending order for every column group; the next chunk's rows of C are in flight
// while this one's MFMAs run.  Then (two barriers) F is dead and its space takes the four partial tiles [wave][16][ldo(d)]; the
// caller folds them with fold_tiles and does its own epilogue.
template <int NG>
__device__ __forceinline__ void stream_product(float* s_f, int LD, const float* C, int mp, int d, int wv, int lr, int lq) {
  f32x4_t acc[NG][4];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[g][y] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  {
    const int nch16 = mp / 16;
    const float* Cb = C + 4 * lr;
    float4 cur[NG][4], nxt[NG][4];
    auto load = [&](float4 (&b)[NG][4], int ch) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int x = 0; x < 4; ++x)
          b[g][x] = (ch < nch16 && 64 * g + 4 * lr < d) ? *reinterpret_cast<const float4*>(Cb + (size_t)(16 * ch + 4 * lq + x) * d + 64 * g)
                                                        : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    load(cur, wv);
    for (int ch = wv; ch < nch16; ch += 4) {
      load(nxt, ch + 4);
      const float4 fa = *reinterpret_cast<const float4*>(s_f + lr * LD + 16 * ch + 4 * lq);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        acc[g][0] = mfma4(fa.x, cur[g][0].x, acc[g][0]); acc[g][1] = mfma4(fa.x, cur[g][0].y, acc[g][1]);
        acc[g][2] = mfma4(fa.x, cur[g][0].z, acc[g][2]); acc[g][3] = mfma4(fa.x, cur[g][0].w, acc[g][3]);
        acc[g][0] = mfma4(fa.y, cur[g][1].x, acc[g][0]); acc[g][1] = mfma4(fa.y, cur[g][1].y, acc[g][1]);
        acc[g][2] = mfma4(fa.y, cur[g][1].z, acc[g][2]); acc[g][3] = mfma4(fa.y, cur[g][1].w, acc[g][3]);
        acc[g][0] = mfma4(fa.z, cur[g][2].x, acc[g][0]); acc[g][1] = mfma4(fa.z, cur[g][2].y, acc[g][1]);
        acc[g][2] = mfma4(fa.z, cur[g][2].z, acc[g][2]); acc[g][3] = mfma4(fa.z, cur[g][2].w, acc[g][3]);
        acc[g][0] = mfma4(fa.w, cur[g][3].x, acc[g][0]); acc[g][1] = mfma4(fa.w, cur[g][3].y, acc[g][1]);
        acc[g][2] = mfma4(fa.w, cur[g][3].z, acc[g][2]); acc[g][3] = mfma4(fa.w, cur[g][3].w, acc[g][3]);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int x = 0; x < 4; ++x) cur[g][x] = nxt[g][x];
    }
  }
  __syncthreads();
  const int LDO = ldo(d);
#pragma unroll
  for (int g = 0; g < NG; ++g)
    if (64 * g + 4 * lr < d) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(s_f + (wv * QT + 4 * lq + r) * LDO + 64 * g + 4 * lr) = make_float4(acc[g][0][r], acc[g][1][r], acc[g][2][r], acc[g][3][r]);
    }
  __syncthreads();
}
// element (row, e) of the product: the waves' partial tiles folded 0, 1, 2, 3
__device__ __forceinline__ float fold_tiles(const float* red, int LDO, int row, int e) {
  return ((red[row * LDO + e] + red[(QT + row) * LDO + e]) + red[(2 * QT + row) * LDO + e]) + red[(3 * QT + row) * LDO + e];
}

}  // namespace ft
}  // namespace mlhot
#endif
