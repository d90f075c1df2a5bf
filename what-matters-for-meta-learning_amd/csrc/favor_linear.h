// FAVOR+ forward and backward in LINEAR form, for more than 32 shots on either side.  Option "favor_linear".
//
// favor.h's chain forms S = Q' K'^T entry by entry: right while Nc <= 30 << m, quadratic in the shot counts above.  Here the context
// enters only through [m, d] sums, as fast_attention.py:151-156 writes it.  Notation favor.h's: E = ratio exp(dd - diag - stab),
// F = E + re, re = ratio 1e-4; per (task, head), with the centre c[e] = v[first shot, e] (favor2.h B1: out is a convex combination
// of the value rows, and sums over v itself lose the digits the rows share):
//   forward   ksum[j] = sum_n F_k[n,j]                    Ctx[j,e] = sum_n F_k[n,j] (v[n,e] - c[e])
//             D[q]    = sum_j F_q[q,j] ksum[j]            out[q,e] = c[e] + (sum_j F_q[q,j] Ctx[j,e]) / D[q]
//   backward  g[q,e]  = dO[q,e] / D[q]                    w[q]     = sum_e g[q,e] (out[q,e] - c[e])
//             dF_q[q,j] = sum_e g[q,e] Ctx[j,e] - w[q] ksum[j]
//             dCtx[j,e] = sum_q F_q[q,j] g[q,e]           dks[j]   = - sum_q F_q[q,j] w[q]
//             dF_k[n,j] = sum_e dCtx[j,e] (v[n,e] - c[e]) + dks[j]          dv[n,e] = sum_j F_k[n,j] dCtx[j,e]
//             G = dF . E   (c's own gradient is identically zero: sum_j F_q ksum = D)
// The feature front (dd, diag, maxima, E) and the back (row sums of G, the stabiliser's gradient, dx) are favor.h's own launches
// on favor.h's buffers, row stride m: the kernels here read E with scalar loads (a float4 would be misaligned on odd rows at odd m).
// Ctx / dCtx have mp = m rounded up to 16 rows of d floats (float4 loads); rows >= m are written as exact zeros.
//
//   sum    grid (task x head, 64-feature chunk), a wave owns 16 features: the shots are walked in 16-row tiles, F^T B on the matrix
//          core (K = the 16 shot slots, rows past N skipped), one more accumulator against a column of x[n] for the [m] vector.
//          forward: F_k, B = v - c, x = 1 -> Ctx, ksum;  backward: F_q, B = g, x = -w -> dCtx, dks.
//   apply  grid (task x head x 16-row tile): F of the tile in LDS, [16 x mp] [mp x d] against Ctx / dCtx streamed from memory
//          (fsum::query_kernel's step 5: wave w takes the 16-feature chunks w, w + 4, .., the four partial tiles fold 0, 1, 2, 3).
//          forward: F_q, Ctx -> D, out;  backward: F_k, dCtx -> dv.
//   gw     grid (task x head x 16-row tile): g = dO / D in token-major rows, -w.
//   grad   grid (task x head x 16-row tile): A = g or v - c in LDS, dF = A C^T over the d channels on the matrix core, wave w takes
//          the feature tiles w, w + 4, ..; G = (dF + x[row] s[j]) E into favor.h's G buffers.
// No atomics; every sum has one order that is a function of the dimensions alone.  v_mfma_f32_16x16x4_f32 operand layout: favor2.h.
#pragma once
#include "common.h"
#include "favor.h"
#include "options.h"
#include "favor_tile.h"

#ifndef MLHOT_HOSTSIM
namespace mlhot {
namespace fl {

using ft::f32x4_t;
using ft::mfma4;
using ft::LDX;
using ft::ldf;
using ft::ldo;

constexpr int MINN = 32;                  // the route serves max(Nq, Nc) > MINN: up to there favor2.h's two launches do
constexpr int MIND = 16; constexpr int MAXD = 256; constexpr int MINM = 16; constexpr int MAXM = 1536;      // a CPU test reads these and applies()
static_assert(MIND == ft::MIND && MAXD == ft::MAXD && MINM == ft::MINM && MAXM == ft::MAXM, "favor_tile.h's envelope");
constexpr int RT = ft::QT;                // rows per workgroup of apply / gw / grad
constexpr int FC = 64;                    // features per sum workgroup: 16 per wave
constexpr int MSMALL = 320;               // apply: F's LDS tile is sized for mp <= MSMALL or for MAXM

// blockIdx.x = (task x head) x 16-row tile, and favor.h's launches count rows in an int
inline bool grid_ok(const FavorDims& f) {
  const long long n = f.Nq > f.Nc ? f.Nq : f.Nc;
  return (long long)f.T * f.H * ((n + RT - 1) / RT) < (1ll << 31) && (long long)f.T * f.H * n < (1ll << 31);
}

inline bool applies(const FavorDims& f) { return (f.Nq > MINN || f.Nc > MINN) && f.Nq >= 1 && f.Nc >= 1 && f.d % 16 == 0 && f.d >= MIND && f.d <= MAXD && f.m >= MINM && f.m <= MAXM && grid_ok(f); }

struct Ws {
  FavorWs w;                              // what favor.h's front and back work on (S and dS stay null: nothing here forms them)
  float *ctx, *ksum, *dctx, *dks;         // [T H][mp][d], [T H][mp]
  float *g, *nw;                          // dO / D in token-major rows [rows_q][d]; -w [rows_q]
  int mp;
  bool ok;
};
inline Ws carve(const FavorDims& f, void* ws, size_t bytes, size_t* need = nullptr) {
  Arena a(ws, bytes);
  Ws r{};
  FavorWs& w = r.w;
  r.mp = (f.m + 15) / 16 * 16;
  const size_t rq = f.rows_q(), rk = f.rows_k(), th = (size_t)f.T * f.H;
  w.pc = a.take<float>((size_t)f.m * f.d);
  w.qf = a.take<float>(rq * f.m);
  w.kf = a.take<float>(rk * f.m);
  w.diag_q = a.take<float>(rq); w.diag_k = a.take<float>(rk);
  w.max_q = a.take<float>(rq);  w.max_k = a.take<float>(rk);
  w.arg_q = a.take<int>(rq);    w.arg_k = a.take<int>(rk);
  w.gmax = a.take<float>(4);    w.gpos = a.take<int>(4);
  w.D = a.take<float>(rq);      // per query ROW (t, n, h) here, not favor.h's [t][h][n]
  w.Gq = a.take<float>(rq * f.m);
  w.Gk = a.take<float>(rk * f.m);
  w.rsum_q = a.take<float>(rq); w.rsum_k = a.take<float>(rk);
  w.gtotal = a.take<float>(4);
  r.ctx = a.take<float>(th * r.mp * f.d);  r.ksum = a.take<float>(th * r.mp);
  r.dctx = a.take<float>(th * r.mp * f.d); r.dks = a.take<float>(th * r.mp);
  r.g = a.take<float>(rq * f.d);           r.nw = a.take<float>(rq);
  w.ok = r.ok = a.ok;
  if (need) *need = a.off + 256;
  return r;
}

// ---- sum: C[j, e] = sum_n F[n, j] (B[n, e] - c[e]),  cs[j] = sum_n F[n, j] x[n] -------------------------------------------------
struct SumArgs {
  const float *F, *B, *x;                 // E rows [rows][m]; token-major rows [rows][d]; per row, or null = 1
  float *C, *cs;                          // [T H][mp][d], [T H][mp]
  int H, N, d, m, mp, centre;             // N rows per task; centre: c = the task's first row of B, else 0
  float re;
};

template <int NG>
__global__ __launch_bounds__(256) void sum_kernel(const SumArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x, t = th / a.H, h = th % a.H;
  const int d = a.d, N = a.N, H = a.H;
  const int jw = blockIdx.y * FC + 16 * wv;
  if (jw >= a.mp) return;                  // whole waves leave; the kernel has no barrier
  const int j = jw + lr;
  const bool jin = j < a.m;
  float cv[4 * NG];
  f32x4_t acc[4 * NG], accx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int et = 0; et < 4 * NG; ++et) {
    acc[et] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    cv[et] = (a.centre && 16 * et < d) ? a.B[((size_t)t * N * H + h) * d + 16 * et + lr] : 0.f;
  }
  for (int n0 = 0; n0 < N; n0 += 16) {
    const int nks = min(4, (N - n0 + 3) / 4);        // shot slots behind N are zeros: their MFMAs add +0 and are skipped
    float ea[4], xa[4];
    size_t row[4];
    bool in[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int n = n0 + 4 * ks + lq;
      in[ks] = n < N;
      row[ks] = ((size_t)t * N + (in[ks] ? n : 0)) * H + h;
      ea[ks] = (in[ks] && jin) ? a.F[row[ks] * a.m + j] + a.re : 0.f;
      xa[ks] = in[ks] ? (a.x ? a.x[row[ks]] : 1.f) : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      if (ks < nks) accx = mfma4(ea[ks], xa[ks], accx);
#pragma unroll
    for (int et = 0; et < 4 * NG; ++et) {
      if (16 * et >= d) continue;
      float bv[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bv[ks] = in[ks] ? a.B[row[ks] * d + 16 * et + lr] - cv[et] : 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        if (ks < nks) acc[et] = mfma4(ea[ks], bv[ks], acc[et]);
    }
  }
  float* Cb = a.C + ((size_t)th * a.mp + jw) * d;
#pragma unroll
  for (int et = 0; et < 4 * NG; ++et) {
    if (16 * et >= d) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) Cb[(size_t)(4 * lq + r) * d + 16 * et + lr] = acc[et][r];
  }
  if (lr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a.cs[(size_t)th * a.mp + jw + 4 * lq + r] = accx[r];
  }
}

// ---- apply: forward D[row] = F . cs, out = c + F C / D (merged order);  backward dv = F C (token-major rows) --------------------
struct ApplyArgs {
  const float *F, *C, *cs, *v;            // E rows [rows][m]; [T H][mp][d]; [T H][mp] (forward); the values (forward: the centre)
  float *out, *D;                         // forward: out [T][Nq][d H], D [rows]; backward: out = dv [rows][d], D null
  int H, N, Nc, d, m, mp, ntile, fwd;
  float re;
};

constexpr int apply_lds(int ng, int mcap) { return RT * ldf(mcap) > 4 * RT * ldo(64 * ng) ? RT * ldf(mcap) : 4 * RT * ldo(64 * ng); }

template <int NG, int MCAP>
__global__ __launch_bounds__(256) void apply_kernel(const ApplyArgs a) {
  __shared__ __attribute__((aligned(16))) float s_f[apply_lds(NG, MCAP)];
  __shared__ float s_den[RT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * RT;
  const int d = a.d, m = a.m, N = a.N, H = a.H, mp = a.mp, LD = ldf(mp);
  // 1. F of the tile: rows >= N and features >= m are zeros, selected by index
  for (int idx = tid; idx < RT * mp; idx += 256) {
    const int row = idx / mp, j = idx - row * mp, n = n0 + row;
    s_f[row * LD + j] = (n < N && j < m) ? a.F[(((size_t)t * N + n) * H + h) * m + j] + a.re : 0.f;
  }
  __syncthreads();
  // 2. forward: D = sum_j F[j] cs[j]
  if (a.fwd) {
    const int row = tid >> 4, p = tid & 15;
    const float* cs = a.cs + (size_t)th * mp;
    float den[1];
    ft::row_sums(mp, p, den, [&](int j, float (&u)[1]) { u[0] += s_f[row * LD + j] * cs[j]; });
    if (p == 0) {
      s_den[row] = den[0];
      if (n0 + row < N) a.D[((size_t)t * N + n0 + row) * H + h] = den[0];
    }
  }
  // 3. F C into the four partial tiles (fsum::query_kernel's step 5)
  ft::stream_product<NG>(s_f, LD, a.C + (size_t)th * mp * d, mp, d, wv, lr, lq);
  // 4. fold the waves 0, 1, 2, 3; forward: divide, add the centre, store in mlhot_favor_fwd's merged order
  const float* cen = a.fwd ? a.v + ((size_t)t * a.Nc * H + h) * d : nullptr;
  for (int idx = tid; idx < RT * d; idx += 256) {
    const int row = idx / d, e = idx - row * d, n = n0 + row;
    if (n >= N) continue;
    const float s = ft::fold_tiles(s_f, ldo(d), row, e);
    if (a.fwd) a.out[((size_t)t * N + n) * ((size_t)d * H) + (size_t)e * H + h] = cen[e] + s / s_den[row];
    else a.out[(((size_t)t * N + n) * H + h) * d + e] = s;
  }
}

// ---- gw: g = dO / D in token-major rows, nw = - sum_e g (out - c) ------------------------------------------------------------------
struct GwArgs {
  const float *dout, *out, *D, *v;
  float *g, *nw;
  int H, Nq, Nc, d, ntile;
};

__global__ __launch_bounds__(256) void gw_kernel(const GwArgs a) {
  const int tid = threadIdx.x, row = tid >> 4, p = tid & 15;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n = tile * RT + row;
  const int d = a.d, H = a.H;
  float w = 0.f;
  if (n < a.Nq) {                           // a row's 16 lanes enter or stay out together: the shuffles below see their own row only
    const size_t gr = ((size_t)t * a.Nq + n) * H + h, ob = ((size_t)t * a.Nq + n) * ((size_t)d * H) + h;
    const float* cen = a.v + ((size_t)t * a.Nc * H + h) * d;
    const float den = a.D[gr];
    for (int e = p; e < d; e += 16) {
      const float gv = a.dout[ob + (size_t)e * H] / den;
      a.g[gr * d + e] = gv;
      w = fmaf(gv, a.out[ob + (size_t)e * H] - cen[e], w);
    }
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) w += __shfl_xor(w, off, 64);
  if (p == 0 && n < a.Nq) a.nw[((size_t)t * a.Nq + n) * H + h] = -w;
}

// ---- grad: G[row, j] = (sum_e (A[row, e] - c[e]) C[j, e] + x[row] cs[j]) E[row, j] -------------------------------------------------
struct GradArgs {
  const float *A, *C, *cs, *x, *E;        // token-major rows [rows][d]; [T H][mp][d]; [T H][mp]; per row or null = 1; E rows [rows][m]
  float* G;                               // [rows][m]
  int H, N, d, m, mp, ntile, centre;
};

__global__ __launch_bounds__(256) void grad_kernel(const GradArgs a) {
  __shared__ __attribute__((aligned(16))) float s_a[RT * LDX];
  __shared__ float s_x[RT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * RT;
  const int d = a.d, m = a.m, N = a.N, H = a.H, mp = a.mp;
  const float* cen = a.centre ? a.A + ((size_t)t * N * H + h) * d : nullptr;
  for (int idx = tid; idx < RT * d; idx += 256) {
    const int row = idx / d, e = idx - row * d, n = n0 + row;
    s_a[row * LDX + e] = n < N ? a.A[(((size_t)t * N + n) * H + h) * d + e] - (cen ? cen[e] : 0.f) : 0.f;
  }
  if (tid < RT) s_x[tid] = n0 + tid < N ? (a.x ? a.x[((size_t)t * N + n0 + tid) * H + h] : 1.f) : 0.f;
  __syncthreads();
  const float* cs = a.cs + (size_t)th * mp;
  for (int jt = wv; 16 * jt < mp; jt += 4) {
    const float* Cr = a.C + ((size_t)th * mp + 16 * jt + lr) * d + 4 * lq;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < d; c0 += 64) {       // four 16-deep chunks per trip, their loads in flight together; chunks past d add +0
      float4 av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool kin = c0 + 16 * u < d;
        av[u] = kin ? *reinterpret_cast<const float4*>(s_a + lr * LDX + c0 + 16 * u + 4 * lq) : make_float4(0.f, 0.f, 0.f, 0.f);
        bv[u] = kin ? *reinterpret_cast<const float4*>(Cr + c0 + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = mfma4(av[u].x, bv[u].x, acc); acc = mfma4(av[u].y, bv[u].y, acc);
        acc = mfma4(av[u].z, bv[u].z, acc); acc = mfma4(av[u].w, bv[u].w, acc);
      }
    }
    const int j = 16 * jt + lr;
    if (j >= m) continue;
    const float sj = cs[j];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 4 * lq + r;
      if (n >= N) continue;
      const size_t at = (((size_t)t * N + n) * H + h) * m + j;
      a.G[at] = (acc[r] + s_x[4 * lq + r] * sj) * a.E[at];
    }
  }
}

template <int MCAP>
inline void launch_apply(const ApplyArgs& a, dim3 grid, hipStream_t s) {
  switch ((a.d + 63) / 64) {
    case 1: hipLaunchKernelGGL((apply_kernel<1, MCAP>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((apply_kernel<2, MCAP>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((apply_kernel<3, MCAP>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((apply_kernel<4, MCAP>), grid, dim3(256), 0, s, a); break;
  }
}
inline int run_apply(const ApplyArgs& a, int th, hipStream_t s, const char* what) {
  ProfScope ps(what, s);
  const dim3 grid((unsigned)(th * a.ntile));
  if (a.mp <= MSMALL) launch_apply<MSMALL>(a, grid, s);
  else launch_apply<MAXM>(a, grid, s);
  return check_launch(what);
}
inline int run_sum(const SumArgs& a, int th, hipStream_t s, const char* what) {
  ProfScope ps(what, s);
  const dim3 grid((unsigned)th, (unsigned)((a.mp + FC - 1) / FC));
  switch ((a.d + 63) / 64) {
    case 1: hipLaunchKernelGGL((sum_kernel<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((sum_kernel<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((sum_kernel<3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((sum_kernel<4>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch(what);
}
inline int run_grad(const GradArgs& a, int th, hipStream_t s, const char* what) {
  ProfScope ps(what, s);
  hipLaunchKernelGGL(grad_kernel, dim3((unsigned)(th * a.ntile)), dim3(256), 0, s, a);
  return check_launch(what);
}

inline int forward(const FavorDims& f, const float* q, const float* k, const float* v, const float* proj, float* out, void* ws, size_t ws_bytes,
                   hipStream_t s) {
  const Ws r = carve(f, ws, ws_bytes);
  if (!r.ok) { set_error("favor_fwd: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  const ft::Scales sc(f.d, f.m);
  const int th = f.T * f.H;
  MLHOT_TRY(favor_front_dd(f, r.w, q, k, proj, sc.c, s));
  MLHOT_TRY(favor_front_feat(f, r.w, sc.ratio, s));
  MLHOT_TRY(run_sum(SumArgs{r.w.kf, v, nullptr, r.ctx, r.ksum, f.H, f.Nc, f.d, f.m, r.mp, 1, sc.re}, th, s, "favor.lin.ctx"));
  return run_apply(ApplyArgs{r.w.qf, r.ctx, r.ksum, v, out, r.w.D, f.H, f.Nq, f.Nc, f.d, f.m, r.mp, (f.Nq + RT - 1) / RT, 1, sc.re}, th, s, "favor.lin.out");
}

inline int backward(const FavorDims& f, const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk,
                    float* dv, void* ws, size_t ws_bytes, hipStream_t s) {
  const Ws r = carve(f, ws, ws_bytes);
  if (!r.ok) { set_error("favor_bwd: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  const ft::Scales sc(f.d, f.m);
  const int th = f.T * f.H, ntq = (f.Nq + RT - 1) / RT, ntk = (f.Nc + RT - 1) / RT;
  {
    ProfScope ps("favor.lin.bwd.gw", s);
    hipLaunchKernelGGL(gw_kernel, dim3((unsigned)(th * ntq)), dim3(256), 0, s, GwArgs{dout, out, r.w.D, v, r.g, r.nw, f.H, f.Nq, f.Nc, f.d, ntq});
  }
  MLHOT_TRY(check_launch("favor.lin.bwd.gw"));
  MLHOT_TRY(run_sum(SumArgs{r.w.qf, r.g, r.nw, r.dctx, r.dks, f.H, f.Nq, f.d, f.m, r.mp, 0, sc.re}, th, s, "favor.lin.bwd.dctx"));
  MLHOT_TRY(run_grad(GradArgs{r.g, r.ctx, r.ksum, r.nw, r.w.qf, r.w.Gq, f.H, f.Nq, f.d, f.m, r.mp, ntq, 0}, th, s, "favor.lin.bwd.Gq"));
  MLHOT_TRY(run_grad(GradArgs{v, r.dctx, r.dks, nullptr, r.w.kf, r.w.Gk, f.H, f.Nc, f.d, f.m, r.mp, ntk, 1}, th, s, "favor.lin.bwd.Gk"));
  MLHOT_TRY(run_apply(ApplyArgs{r.w.kf, r.dctx, nullptr, v, dv, nullptr, f.H, f.Nc, f.Nc, f.d, f.m, r.mp, ntk, 0, sc.re}, th, s, "favor.lin.bwd.dv"));
  MLHOT_TRY(favor_back_sums(f, r.w, s));
  return favor_back_dx(f, r.w, q, k, sc.c, dq, dk, s);
}

}  // namespace fl
}  // namespace mlhot
#endif

namespace mlhot {
// The envelope of the linear route (mlhot_favor_linear_supported): the dimensions alone, not the option.
inline bool favor_linear_ok(const FavorDims& f) {
#ifndef MLHOT_HOSTSIM
  return f.T >= 1 && f.H >= 1 && fl::applies(f);
#else
  (void)f; return false;
#endif
}
}  // namespace mlhot
