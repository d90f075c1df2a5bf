// Attention mass per context slot: the read-out w = S / D of favor_cached.h / favor_long.h / favor_paged.h reduced
// over the target rows INSIDE the query launch,
//     mass[t][h][c] = sum_n tw[t][n] * w[t][h][n][c]          (tw == nullptr: the plain column sum)
// without w [T][H][Nq][Nc] ever existing in memory.  Three query kernels, one per per-shot form; each IS its form's plain query - the
// same favor_tile.h steps in the same sequence, so out has that entry's bits - plus one more store behind D, as w was in 6c-5.
//
// SUMMATION ORDER (no atomics; a function of Nq alone):
//   1. a (task, head, 16-row tile) workgroup adds its rows' terms per column in ASCENDING ROW order, starting from +0.0f, into the
//      tile partial part[t][h][tile][c] - thread c owns column c (of the page, for the paged form);
//   2. fold_kernel adds the tile partials per column in ASCENDING TILE order, starting from +0.0f.
//   A term is w = S / D, the read-out's own expression and its one divide; with tw it is tw * w - ONE rounded multiply - and every
//   addition is ONE rounded add: NO FMA CONTRACTION.  hipcc contracts a * b + c by default (and HIP's __fmul_rn / __fadd_rn are
//   plain operators in its headers, contracted like any other - measured: they fused here), so the two functions that add are
//   compiled under `#pragma clang fp contract(off)` and the product passes through an empty asm, which makes it a value of its
//   own.  So with tw == nullptr mass is the fp32 fold, in that order, of the very bits mlhot_favor_query_weights_fwd / _long_fwd /
//   _paged_fwd store into w.
//   Tiles are 16 target rows from row 0 on: a caller that splits the targets at multiples of 16 gets the same tile partials from
//   the pieces (row invariance of S and D), and one fold over all of them gives the single call's bits.
// Columns c >= lens[t]: exactly 0.0f (long / paged: selected by index; keys form: S's column of a zero row of F_k is +0).
//
// PAGED FORM, TWO WALKS: D[n] is final only behind the last page.  Walk 1 is favor_paged.h's own loop (S per page, D and the out
// chains carried on).  Behind it the LAST page's S is still in the wide tile: its columns are reduced straight from LDS.  Walk 2
// forms S of every earlier page AGAIN (ft::s_tile is a function of its operands: the same bits) and reduces it with the final D.
// A state of at most 256 slots has one page and no second walk: the long kernel's operations exactly.
// MEMORY: the tile partials, T H ceil(Nq / 16) Nc floats - 1/16 of w - are all this path writes beside out and mass; D stays in LDS.
// LDS: the form's own arrays plus the 16 target weights.
#pragma once
#include "common.h"
#include "favor_tile.h"
#include "favor_cached.h"
#include "favor_long.h"
#include "favor_paged.h"

namespace mlhot {

#ifndef MLHOT_HOSTSIM
namespace fm {

using ft::QT;
using fl2::LDW;

struct Mass {
  const float* tw;      // [T][Nq] target weights, or nullptr
  float* part;          // [T H][ntile][Nc] tile partials
};

// the tile's target weights into s_tw (rows >= `rows`: unused); no barrier - the callers have one before the first read
__device__ __forceinline__ void stage_tw(const Mass& ms, int t, int Nq, int n0, int rows, float* s_tw, int tid) {
  if (ms.tw && tid < rows) s_tw[tid] = ms.tw[(size_t)t * Nq + n0 + tid];
}

// part[p0 + c] for the pn columns of the tile s_P (row stride ld, column 0 = slot p0): thread c adds rows 0 .. rows - 1 in order
template <bool TW>
__device__ __forceinline__ void mass_cols(const float* s_P, int ld, const float* s_D, const float* s_tw, int rows, int p0, int pn, float* part, int tid) {
#pragma clang fp contract(off)
  if (tid < pn) {
    float acc = 0.f;
    for (int row = 0; row < rows; ++row) {
      float term = s_P[row * ld + tid] / s_D[row];
      if (TW) {
        term = s_tw[row] * term;
        asm volatile("" : "+v"(term));                 // the rounded product is a value of its own: nothing fuses across this
      }
      acc = acc + term;
    }
    part[p0 + tid] = acc;
  }
}
__device__ __forceinline__ void mass_step(const Mass& ms, const float* s_P, int ld, const float* s_D, const float* s_tw, int rows, int p0, int pn, float* part, int tid) {
  if (ms.tw) mass_cols<true>(s_P, ld, s_D, s_tw, rows, p0, pn, part, tid);
  else mass_cols<false>(s_P, ld, s_D, s_tw, rows, p0, pn, part, tid);
}

// ---- keys form (Nc <= 32): fc::query_body's steps, the tile partial behind D ------------------------------------------------------
__global__ __launch_bounds__(256) void query_mass_kernel(const fc::Args a, const Mass ms) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_D[QT], s_diag[QT], s_pm[4][QT], s_tw[QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int rows = min(QT, Nq - n0);
  stage_tw(ms, t, Nq, n0, rows, s_tw, tid);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* krow[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + ((size_t)th * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
  ft::s_tile(s_f, ft::ldf(mp), krow, (Nc + 15) / 16, mp / 16, Nc, ft::BPlain{}, red, s_S);
  ft::s_rowsum(s_S, Nc, s_D);
  mass_step(ms, s_S, ft::LDS_S, s_D, s_tw, rows, 0, Nc, ms.part + (size_t)blockIdx.x * Nc, tid);
  ft::sv_tiles(s_S, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, d, wv, lr, lq, [&](int row, int e, float o) {
    const int n = n0 + row;
    if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
  });
}

// ---- long form (Nc <= 256): fl2::query_body's steps, the tile partial behind D; zeros behind the task's slots ------------------------
__global__ __launch_bounds__(256) void query_long_mass_kernel(const fl2::Args a, const Mass ms) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT], s_tw[QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc), rows = min(QT, Nq - n0);
  stage_tw(ms, t, Nq, n0, rows, s_tw, tid);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  fp2::s_page(a, th, 0, need, s_f, red, s_S, s_W, tid, lr, lq);          // fl2::query_body's chunk loop and its barrier
  ft::s_rowsum_wide(s_W, LDW, need, s_D);
  float* part = ms.part + (size_t)blockIdx.x * Nc;
  mass_step(ms, s_W, LDW, s_D, s_tw, rows, 0, need, part, tid);
  for (int np = need + tid; np < Nc; np += 256) part[np] = 0.f;
  ft::sv_tiles_wide(s_W, LDW, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, need, d, wv, lr, lq, [&](int row, int e, float o) {
    const int n = n0 + row;
    if (n < Nq) a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = o;
  });
}

// ---- paged form (Nc <= 4096): fp2::paged_body's walk, then the column sums with the final D - the last page from LDS, the earlier
// pages formed again -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void query_paged_mass_kernel(const fl2::Args a, const Mass ms) {
  __shared__ __attribute__((aligned(16))) float s_f[QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[QT * ft::LDS_S], s_W[QT * LDW], s_D[QT], s_diag[QT], s_pm[4][QT], s_tw[QT];
  constexpr int PAGE = fp2::PAGE;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * QT;
  const int d = a.d, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp;
  const int need = ft::clamp_len(a.lens, t, 1, Nc), rows = min(QT, Nq - n0);
  stage_tw(ms, t, Nq, n0, rows, s_tw, tid);
  ft::query_front([&](int r) { return n0 + r < Nq ? a.x + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  const float* v0 = a.v + ((size_t)t * Nc * H + h) * d;
  // walk 1: fp2::paged_body's loop
  {
    ft::f32x4_t o[ft::MAXD / 64];
#pragma unroll
    for (int i = 0; i < ft::MAXD / 64; ++i) o[i] = ft::f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int p0 = 0; p0 < need; p0 += PAGE) {
      const int pn = min(PAGE, need - p0);
      fp2::s_page(a, th, p0, pn, s_f, red, s_S, s_W, tid, lr, lq);
      ft::s_rowsum_page(s_W, LDW, pn, s_D, p0 > 0 ? s_D : nullptr);
#pragma unroll
      for (int i = 0; i < ft::MAXD / 64; ++i) {
        const int et = wv + 4 * i;
        if (et * 16 < d) o[i] = ft::sv_page(o[i], s_W, LDW, v0, (size_t)H * d, p0, p0 + pn, need, 16 * et + lr, lr, lq);
      }
      if (p0 + PAGE < need) __syncthreads();                                   // the wide tile is the next page's; the last page stays
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
  // the last page: still in the wide tile, D final
  float* part = ms.part + (size_t)blockIdx.x * Nc;
  const int plast = (need - 1) / PAGE * PAGE;
  mass_step(ms, s_W, LDW, s_D, s_tw, rows, plast, need - plast, part, tid);
  for (int np = need + tid; np < Nc; np += 256) part[np] = 0.f;
  // walk 2: the earlier pages again
  for (int p0 = 0; p0 < plast; p0 += PAGE) {
    __syncthreads();                                                           // every column sum of the tile before is done
    fp2::s_page(a, th, p0, PAGE, s_f, red, s_S, s_W, tid, lr, lq);
    mass_step(ms, s_W, LDW, s_D, s_tw, rows, p0, PAGE, part, tid);
  }
}

// ---- fold: mass[th][c] = the tile partials of column c in ascending tile order ------------------------------------------------------
__global__ __launch_bounds__(256) void fold_kernel(const float* part, int ntile, int Nc, float* mass) {
#pragma clang fp contract(off)
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= Nc) return;
  const float* p = part + (size_t)blockIdx.x * ntile * Nc + c;
  float acc = 0.f;
  for (int i = 0; i < ntile; ++i) acc = acc + p[(size_t)i * Nc];
  mass[(size_t)blockIdx.x * Nc + c] = acc;
}

}  // namespace fm
#endif

// workspace of the three mass entries: the tile partials, T H ceil(Nq / 16) Nc floats (at least favor_query_fwd's token block).
// This is the path's whole footprint beside out and mass: 1/16 of w [T][H][Nq][Nc], rounded up to a tile.  0: shape not served.
inline size_t favor_query_mass_ws_need(int T, int H, int Nq, int Nc, int d, int m) {
#ifndef MLHOT_HOSTSIM
  if (favor_paged_ok(T, H, Nc, d, m) && Nq >= 1) {
    const size_t b = (size_t)T * H * (((size_t)Nq + 15) / 16) * Nc * sizeof(float);
    return b > 256 ? align_up(b, (size_t)256) : 256;
  }
#endif
  (void)T; (void)H; (void)Nq; (void)Nc; (void)d; (void)m; return 0;
}

// mlhot_favor_mass_fold: part [TH][ntile][Nc] -> mass [TH][Nc]
inline int favor_mass_fold(const float* part, int TH, int ntile, int Nc, float* mass, hipStream_t s) {
  const char* what = "favor_mass_fold";
  if (TH <= 0 || ntile <= 0 || Nc <= 0 || !part || !mass) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
#ifdef MLHOT_HOSTSIM
  (void)s; set_error("%s: GPU build only", what); return MLHOT_ERR_UNSUPPORTED;
#else
  if (TH >= (1 << 20) || Nc > FAVOR_PAGED_MAXNC) { set_error("%s serves T H < 2^20 and Nc <= 4096 (got T H=%d Nc=%d)", what, TH, Nc); return MLHOT_ERR_UNSUPPORTED; }
  if (((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(mass)) & 3) != 0) { set_error("%s: part and mass must be 4-byte aligned", what); return MLHOT_ERR_ARG; }
  ProfScope ps("favor.massfold", s);
  hipLaunchKernelGGL(fm::fold_kernel, dim3(TH, (Nc + 255) / 256), dim3(256), 0, s, part, ntile, Nc, mass);
  return check_launch("favor.massfold");
#endif
}

// form 0: mlhot_favor_query_mass_fwd (a keys / ragged state, no lens), 1: _long_mass_fwd, 2: _paged_mass_fwd.
// fold != 0: mass [T][H][Nc], the tile partials in ws (favor_query_mass_ws_need bytes).  fold == 0: mass IS the tile partials
// [T][H][ceil(Nq / 16)][Nc] and ws is the token block.
inline int favor_query_mass_launch(const char* what, int form, const float* q, const void* state, const float* v, const float* proj, const int32_t* lens,
                                   const float* tw, int T, int H, int Nq, int Nc, int d, int m, float* out, float* mass, int fold, void* ws, size_t ws_bytes,
                                   hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || !q || !state || !v || !proj || !out || !mass) { set_error("%s: bad argument", what); return MLHOT_ERR_ARG; }
  const bool ok = form == 0 ? favor_cached_ok(T, H, Nc, d, m) : form == 1 ? favor_long_ok(T, H, Nc, d, m) : favor_paged_ok(T, H, Nc, d, m);
  if (!ok) {
    set_error("%s serves Nc <= %d, d %% 16 == 0, d <= 256, 16 <= m <= 1536 on the GPU build (got Nc=%d d=%d m=%d)", what,
              form == 0 ? 32 : form == 1 ? FAVOR_LONG_MAXNC : FAVOR_PAGED_MAXNC, Nc, d, m);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)tw; (void)fold; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const size_t need = fold ? favor_query_mass_ws_need(T, H, Nq, Nc, d, m) : 256;
  if (ws == nullptr || ws_bytes < need) { set_error("%s: workspace too small (%zu < %zu)", what, ws_bytes, need); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + fm::QT - 1) / fm::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("%s: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)", what); return form == 0 ? MLHOT_ERR_ARG : MLHOT_ERR_UNSUPPORTED; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) {
    set_error("%s: q, proj and state must be 16-byte aligned", what);
    return form == 0 ? MLHOT_ERR_ARG : MLHOT_ERR_UNSUPPORTED;
  }
  if (((reinterpret_cast<uintptr_t>(mass) | reinterpret_cast<uintptr_t>(tw) | reinterpret_cast<uintptr_t>(ws)) & 3) != 0) {
    set_error("%s: tw, mass and ws must be 4-byte aligned", what);
    return MLHOT_ERR_ARG;
  }
  fm::Mass ms{tw, fold ? (float*)ws : mass};
  const dim3 grid((unsigned)(ntile * T * H));
  const char* label = form == 0 ? "favor.querymass" : form == 1 ? "favor.lquerymass" : "favor.pquerymass";
  {
    ProfScope ps(label, s);
    if (form == 0) {
      const fc::State st = fc::carve_state(T, H, Nc, m, const_cast<void*>(state));
      fc::Args a = fc::make_args(T, H, Nq, Nc, d, m, st);
      a.x = q; a.proj = proj; a.v = v; a.out = out; a.ntile = (int)ntile;
      hipLaunchKernelGGL(fm::query_mass_kernel, grid, dim3(256), 0, s, a, ms);
    } else {
      const fl2::State st = fl2::carve_state(T, H, Nc, m, const_cast<void*>(state));
      fl2::Args a = fl2::make_args(T, H, Nq, Nc, d, m, st, lens);
      a.x = q; a.proj = proj; a.v = v; a.out = out; a.w = nullptr; a.ntile = (int)ntile;
      if (form == 1) hipLaunchKernelGGL(fm::query_long_mass_kernel, grid, dim3(256), 0, s, a, ms);
      else hipLaunchKernelGGL(fm::query_paged_mass_kernel, grid, dim3(256), 0, s, a, ms);
    }
  }
  MLHOT_TRY(check_launch(label));
  return fold ? favor_mass_fold(ms.part, T * H, (int)ntile, Nc, mass, s) : MLHOT_OK;
#endif
}

}  // namespace mlhot
