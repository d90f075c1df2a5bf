// Top-k attention read-out: per (task, head, target row) the k heaviest context slots of the read-out w = S / D of
// favor_cached.h / favor_long.h / favor_paged.h and their weights, selected INSIDE the query launch,
//     idx[t][h][n][j] = the j-th valid slot in the order (S[n][c] descending, c ascending),   wk[t][h][n][j] = S[n][idx] / D[n],
// without w [T][H][Nq][Nc] ever existing in memory.  Three query kernels, one per per-shot form; each IS its form's plain query - the
// same favor_tile.h steps in the same sequence, so out has that entry's bits - plus a selection behind each S tile.
//
// DEFINITION.  The ranked quantity is the UN-NORMALISED score S[n][c], the bits ft::s_tile leaves in the tile; D[n] > 0 is one number
// per row and IEEE division by it is monotone, so the order of S is an order of w (w may round two different S to one value: the
// VALUES of a top-k over w are these, the indices need not be).  Valid slots: c < lens[t] (long, paged); the keys entry takes no lens
// and a column whose S is exactly +0 - a zero row of F_k - is absent.  Ties go to the lower slot.  wk is the read-out's own single
// IEEE divide with the row's final D: the bits mlhot_favor_query_weights_fwd / _long_fwd / _paged_fwd store into w[t][h][n][idx].
// Entries j >= the number of valid slots: idx = -1, wk = +0.0f.
//
// SELECTION (no atomics, no workspace, no LDS of its own).  S >= 0, so its bit pattern compares as an unsigned integer; the key
//     key(c) = (bits(S[n][c]) << 32) | (0xFFFFFFFF - c)            (0: no candidate)
// is unique per slot and its unsigned order IS the ranking.  Wave w owns the tile's rows 4 w .. 4 w + 3 and works on the four at once
// (four independent chains).  A lane holds the keys of the columns lane, lane + 64, .. of the tile and, in lane j < k, the row's j-th
// best so far.  Round j is the wave-wide maximum over all keys strictly below round j - 1's: no marking, and since the order is
// total the result does not depend on how the slots are split into pages.  The rounds end early when nothing is left.
// PAGED FORM, ONE WALK: the selection runs on each page's S while it lies in the wide tile, before the barrier that hands the tile to
// the next page; the running k best are carried across the pages IN REGISTERS (lane j, four rows: 8 VGPRs - less than the 2 KiB of LDS
// a carried list would take), the divide by the final D follows the last page.  A page none of whose keys (in the wave's four rows)
// exceeds the carried k-th key is skipped after one compare and a ballot.  A state of at most 256 slots has one page: the long
// kernel's operations exactly; a long state of at most 32 slots selects among the same S bits as the keys kernel.
// The bits of a row depend neither on the other rows of the call nor on the capacity Nc the same shots are kept in.
// LDS: the form's own arrays, nothing more.
#pragma once
#include "common.h"
#include "favor_tile.h"
#include "favor_cached.h"
#include "favor_long.h"
#include "favor_paged.h"

namespace mlhot {

constexpr int FAVOR_TOPK_MAXK = 16;

#ifndef MLHOT_HOSTSIM
namespace ftk {

using ft::QT;
using fl2::LDW;
typedef unsigned long long key_t;

struct TopK {
  int k;
  int32_t* idx;         // [T H][Nq][k]
  float* wk;            // [T H][Nq][k]
};

// the running k best of the wave's four rows: best[r] of lane j < k is row 4 wv + r's j-th key, kth[r] (wave-uniform) its k-th
struct Sel {
  key_t best[4], kth[4];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int r = 0; r < 4; ++r) best[r] = kth[r] = 0;
  }
};

__device__ __forceinline__ key_t wave_max_key(key_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const key_t y = __shfl_xor(x, off, 64);
    x = y > x ? y : x;
  }
  return x;
}

// The tile s_P (row stride ld, column 0 = slot p0, pn columns in use) joins the running k best.  NC: columns per lane (64 NC >= pn).
// ZERO_ABSENT: a column whose S is +0 is no candidate (the keys form).  Reads LDS only; the callers' barrier stands before it.
template <int NC, bool ZERO_ABSENT>
__device__ __forceinline__ void select_tile(Sel& sl, const float* s_P, int ld, int p0, int pn, int k, int wv, int lane) {
  key_t cand[4][NC];
  bool any = false;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + 64 * i;
      key_t key = 0;
      if (c < pn) {
        const unsigned bits = __float_as_uint(s_P[(4 * wv + r) * ld + c]);
        if (!ZERO_ABSENT || bits != 0u) key = ((key_t)bits << 32) | (key_t)(0xFFFFFFFFu - (unsigned)(p0 + c));
      }
      cand[r][i] = key;
      any = any || key > sl.kth[r];
    }
  if (!__any(any)) return;                                                     // the page adds nothing to any of the four rows
  key_t prev[4], fresh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { prev[r] = ~(key_t)0; fresh[r] = 0; }
  for (int j = 0; j < k; ++j) {
    key_t left = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      key_t mx = sl.best[r] < prev[r] ? sl.best[r] : 0;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const key_t c = cand[r][i] < prev[r] ? cand[r][i] : 0;
        mx = c > mx ? c : mx;
      }
      mx = wave_max_key(mx);
      prev[r] = mx;
      if (lane == j) fresh[r] = mx;
      left |= mx;
    }
    if (left == 0) break;                                                      // wave-uniform: every row has run out of candidates
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) { sl.best[r] = fresh[r]; sl.kth[r] = __shfl(fresh[r], k - 1, 64); }
}

// idx and wk of the wave's rows from the final list and the final D: lane j stores entry j
__device__ __forceinline__ void store_topk(const Sel& sl, const TopK& tk, const float* s_D, size_t row0, int rows, int wv, int lane) {
  if (lane >= tk.k) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * wv + r;
    if (row >= rows) continue;
    const key_t key = sl.best[r];
    const size_t at = (row0 + row) * tk.k + lane;
    tk.idx[at] = key ? (int32_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
    tk.wk[at] = key ? __uint_as_float((unsigned)(key >> 32)) / s_D[row] : 0.f;
  }
}

// ---- keys form (Nc <= 32): fc::query_body's steps, the selection behind D --------------------------------------------------------
__global__ __launch_bounds__(256) void query_topk_kernel(const fc::Args a, const TopK tk) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int rows = min(QT, Nq - n0);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* krow[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + ((size_t)th * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
  ft::s_tile(s_f, ft::ldf(mp), krow, (Nc + 15) / 16, mp / 16, Nc, ft::BPlain{}, red, s_S);
  ft::s_rowsum(s_S, Nc, s_D);
  Sel sl;
  sl.clear();
  select_tile<1, true>(sl, s_S, ft::LDS_S, 0, Nc, tk.k, wv, lane);
  store_topk(sl, tk, s_D, (size_t)th * Nq + n0, rows, wv, lane);
  ft::sv_tiles(s_S, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, d, wv, lr, lq, [&](int row, int e, float o) {
    const int n = n0 + row;
    if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
  });
}

// ---- long form (Nc <= 256): fl2::query_body's steps, the selection behind D over the task's slots ----------------------------------
__global__ __launch_bounds__(256) void query_long_topk_kernel(const fl2::Args a, const TopK tk) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc), rows = min(QT, Nq - n0);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  fp2::s_page(a, th, 0, need, s_f, red, s_S, s_W, tid, lr, lq);          // fl2::query_body's chunk loop and its barrier
  ft::s_rowsum_wide(s_W, LDW, need, s_D);
  Sel sl;
  sl.clear();
  select_tile<4, false>(sl, s_W, LDW, 0, need, tk.k, wv, lane);
  store_topk(sl, tk, s_D, (size_t)th * Nq + n0, rows, wv, lane);
  ft::sv_tiles_wide(s_W, LDW, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, need, d, wv, lr, lq, [&](int row, int e, float o) {
    const int n = n0 + row;
    if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
  });
}

// ---- paged form (Nc <= 4096): fp2::paged_body's ONE walk; each page joins the carried k best while it lies in the wide tile --------
__global__ __launch_bounds__(256) void query_paged_topk_kernel(const fl2::Args a, const TopK tk) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT];
  constexpr int PAGE = fp2::PAGE;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc), rows = min(QT, Nq - n0);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* v0 = a.v + ((size_t)t * Nc * H + h) * d;
  ft::f32x4_t o[ft::MAXD / 64];
#pragma unroll
  for (int i = 0; i < ft::MAXD / 64; ++i) o[i] = ft::f32x4_t{0.f, 0.f, 0.f, 0.f};
  Sel sl;
  sl.clear();
  for (int p0 = 0; p0 < need; p0 += PAGE) {
    const int pn = min(PAGE, need - p0);
    fp2::s_page(a, th, p0, pn, s_f, red, s_S, s_W, tid, lr, lq);
    ft::s_rowsum_page(s_W, LDW, pn, s_D, p0 > 0 ? s_D : nullptr);
    select_tile<4, false>(sl, s_W, LDW, p0, pn, tk.k, wv, lane);
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
  store_topk(sl, tk, s_D, (size_t)th * Nq + n0, rows, wv, lane);              // D is final behind the last page
}

}  // namespace ftk
#endif

// form 0: mlhot_favor_query_topk_fwd (a keys / ragged state, no lens), 1: _long_topk_fwd, 2: _paged_topk_fwd.
inline int favor_query_topk_launch(const char* what, int form, const float* q, const void* state, const float* v, const float* proj, const int32_t* lens,
                                   int T, int H, int Nq, int Nc, int d, int m, float* out, int k, int32_t* idx, float* wk, void* ws, size_t ws_bytes,
                                   hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !q || !state || !v || !proj || !out || !idx || !wk || k < 1 || k > FAVOR_TOPK_MAXK) {
    set_error("%s: bad argument (1 <= k <= %d, idx and wk not NULL)", what, FAVOR_TOPK_MAXK);
    return MLHOT_ERR_ARG;
  }
  const bool ok = form == 0 ? favor_cached_ok(T, H, Nc, d, m) : form == 1 ? favor_long_ok(T, H, Nc, d, m) : favor_paged_ok(T, H, Nc, d, m);
  if (!ok) {
    set_error("%s serves Nc <= %d, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what,
              form == 0 ? 32 : form == 1 ? FAVOR_LONG_MAXNC : FAVOR_PAGED_MAXNC, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < 256) { set_error("%s: workspace too small (%zu < 256)", what, ws_bytes); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + ftk::QT - 1) / ftk::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return form == 0 ? MLHOT_ERR_ARG : MLHOT_ERR_UNSUPPORTED; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) {
    set_error("%s: q, proj and state must be 16-byte aligned", what);
    return form == 0 ? MLHOT_ERR_ARG : MLHOT_ERR_UNSUPPORTED;
  }
  if (((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(wk)) & 3) != 0) { set_error("%s: idx and wk must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  const ftk::TopK tk{k, idx, wk};
  const dim3 grid((unsigned)(ntile * T * H));
  const char* label = form == 0 ? "favor.querytopk" : form == 1 ? "favor.lquerytopk" : "favor.pquerytopk";
  {
    ProfScope ps(label, s);
    if (form == 0) {
      const fc::State st = fc::carve_state(T, H, Nc, m, const_cast<void*>(state));
      fc::Args a = fc::make_args(T, H, Nq, Nc, d, m, st);
      a.x = q; a.proj = proj; a.v = v; a.out = out; a.ntile = (int)ntile;
      hipLaunchKernelGGL(ftk::query_topk_kernel, grid, dim3(256), 0, s, a, tk);
    } else {
      const fl2::State st = fl2::carve_state(T, H, Nc, m, const_cast<void*>(state));
      fl2::Args a = fl2::make_args(T, H, Nq, Nc, d, m, st, lens);
      a.x = q; a.proj = proj; a.v = v; a.out = out; a.w = nullptr; a.ntile = (int)ntile;
      if (form == 1) hipLaunchKernelGGL(ftk::query_long_topk_kernel, grid, dim3(256), 0, s, a, tk);
      else hipLaunchKernelGGL(ftk::query_paged_topk_kernel, grid, dim3(256), 0, s, a, tk);
    }
  }
  return check_launch(label);
#endif
}

}  // namespace mlhot
