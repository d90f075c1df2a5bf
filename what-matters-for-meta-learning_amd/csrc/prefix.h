// Forward-only operators over EVERY context prefix 1..Nc of one batch (the evaluator's loss-versus-context-size sweep:
// networks/_resnet_np.py forward_prefixes).  Row k-1 of each output is what the plain operator returns for the first k shots.
//   agg     mean / max / baco of ops_direct.h as running sums / maxima in shot order: one pass over rs, the same operations in the
//           same order as AggFwd on rs[:, :k], so the rows agree with it bit for bit.
//   FAVOR+  favor2.h's arithmetic.  Nothing on the query side depends on the prefix; on the key side only the batch-global
//           stabiliser does: for k shots it is M_k = max of dd over all tasks, heads, features and the FIRST k shots.  Launches:
//     F1      favor2.h's projection kernel, unchanged: dd = (c x) P^T for query and key rows, partial query row maxima.
//     keymax  one wave per key row: its maximum over the m features.
//     sweep   grid (task x head).  M_1..M_Nc from the key row maxima (every workgroup folds the same T H Nc values).  The
//             prefixes are cut into groups whose M_k lie within SPAN of the group's largest, L.  Per group ONE feature pass
//             A[n][j] = sum_m F_q[n][m] ratio exp(dd_k[j][m] - (diag_j + L)) on the matrix core (and once Q[n] = sum_m
//             F_q[n][m]); every prefix of the group is then S_k[n][j] = s_jk A[n][j] + ratio 1e-4 Q[n] for j < k with
//             s_jk = exp((diag_j + L) - (diag_j + M_k)), D_k = rowsum, out_k = S_k V / D_k: O(Nq k d) per prefix.
//             s_jk is 1 when M_k = L.  Within a group exp(. - L) >= exp(. - M_k) e^-SPAN: whatever underflows against L is below
//             e^-55 against M_k, nothing beside the 1e-4 every feature carries; s_jk <= e^SPAN cannot overflow.  Batches whose
//             running maximum climbs by more than SPAN take one feature pass per such step - the cost of the plain loop at worst.
#pragma once
#include "common.h"
#include "foreach.h"
#include "ops_direct.h"
#include "favor2.h"

namespace mlhot {

struct AggPrefixFwd {
  int mode, T, Nc, R;
  const float* rs; const float* lv; float* r; float* sigma;      // r, sigma: [Nc][T][R]; sigma may be null
  MLHOT_HD void operator()(size_t i) const {
    const int j = (int)(i % R); const size_t t = i / R;
    const float* src = rs + t * Nc * R + j;
    const size_t step = (size_t)T * R;
    float* dst = r + i;
    if (mode == 0) {
      float s = 0.f;
      for (int n = 0; n < Nc; ++n) { s += src[(size_t)n * R]; dst[n * step] = s / (float)(n + 1); }
    } else if (mode == 1) {
      float best = src[0];
      dst[0] = best;
      for (int n = 1; n < Nc; ++n) { const float v = src[(size_t)n * R]; if (v > best) best = v; dst[n * step] = best; }
    } else {
      const float* lsrc = lv + t * Nc * R + j;
      float s1 = 1.f, s2 = 0.f;   // prior: mu_z = 0, sigma_z = 1, as AggFwd
      for (int n = 0; n < Nc; ++n) {
        const float iv = 1.f / (1e-5f + softplus_f(lsrc[(size_t)n * R]));
        s1 += iv; s2 += iv * src[(size_t)n * R];
        const float sz = 1.f / s1;
        if (sigma) sigma[i + n * step] = sz;
        dst[n * step] = sz * s2;
      }
    }
  }
};

#ifndef MLHOT_HOSTSIM
namespace fp {
using fv::f32x4_t;
using fv::mfma4;
using fv::MAXN;
using fv::NPMAX;
constexpr int NT = 1024, NW = NT / 64;
constexpr int NPART = NT / MAXN;      // threads per shot in the fold of the key row maxima
constexpr float SPAN = 32.f;          // prefixes share a feature pass while their stabilisers lie this close (header comment)
static_assert(MAXN == 32 && NT == MAXN * MAXN, "the sweep kernel builds S with one thread per (n, j)");

struct Ws { fv::Ws w; float* kmax; bool ok; };     // w: only what F1 writes (dd, partial maxima); kmax [T Nc H]
inline Ws carve(const FavorDims& f, void* ws, size_t bytes, size_t* need = nullptr) {
  Arena a(ws, bytes);
  Ws p{};
  fv::Ws& w = p.w;
  w.mp = (f.m + 15) / 16 * 16; w.nch = (f.m + fv::FCH - 1) / fv::FCH; w.npart = w.nch * 4;
  const size_t rq = f.rows_q(), rk = f.rows_k(), th = (size_t)f.T * f.H;
  w.eq = a.take<float>(rq * w.mp); w.ek = a.take<float>(rk * w.mp);
  w.pm_v = a.take<float>(rq * w.npart); w.pm_i = a.take<int>(rq * w.npart);
  w.wg_v = a.take<float>(th * w.nch); w.wg_row = a.take<int>(th * w.nch); w.wg_j = a.take<int>(th * w.nch);
  p.kmax = a.take<float>(rk);
  p.ok = w.ok = a.ok;
  if (need) *need = a.off + 256;
  return p;
}

__global__ __launch_bounds__(256) void keymax_kernel(const float* ek, int rows, int m, int mp, float* kmax) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = ek + (size_t)row * mp;
  float best = -INFINITY;
  for (int j = 4 * lane; j < mp; j += 256) {
    const float4 u = *reinterpret_cast<const float4*>(p + j);
    if (j < m) best = fmaxf(best, u.x);
    if (j + 1 < m) best = fmaxf(best, u.y);
    if (j + 2 < m) best = fmaxf(best, u.z);
    if (j + 3 < m) best = fmaxf(best, u.w);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if (lane == 0) kmax[row] = best;
}

// a.out: [Nc][T][Nq][d H]
__global__ __launch_bounds__(NT) void sweep_kernel(const fv::Args a, const float* kmax) {
  __shared__ float s_mx[MAXN], s_diag[2 * MAXN], s_A[MAXN * (MAXN + 1)], s_S[2][MAXN * (MAXN + 1)], s_D[2][MAXN], s_Q[MAXN];
  __shared__ float s_pm[NPART][MAXN + 1], s_M[MAXN], s_L[MAXN], red[NW * 4 * 64 * 4];
  __shared__ int s_grp[MAXN], s_ng;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x, t = th / a.f.H, h = th % a.f.H;
  const int d = a.f.d, m = a.f.m, Nq = a.f.Nq, Nc = a.f.Nc, H = a.f.H, T = a.f.T, mp = a.w.mp;
  // query row maxima from F1's partials (as favor2.h's F2)
  if (tid < Nq) {
    const size_t grow = (size_t)(t * Nq + tid) * H + h;
    float pv[NPMAX];
#pragma unroll
    for (int p = 0; p < NPMAX; ++p) pv[p] = p < a.w.npart ? a.w.pm_v[grow * a.w.npart + p] : -INFINITY;
    float best = -INFINITY;
#pragma unroll
    for (int p = 0; p < NPMAX; ++p) best = fmaxf(best, pv[p]);
    s_mx[tid] = best;
  }
  // per shot: the maximum over every task and head, NPART threads per shot
  {
    const int n = tid & (MAXN - 1), part = tid / MAXN;
    float best = -INFINITY;
    if (n < Nc)
      for (int b = part; b < T * H; b += NPART) best = fmaxf(best, kmax[((size_t)(b / H) * Nc + n) * H + b % H]);
    s_pm[part][n] = best;
  }
  // diag = 0.5 c^2 |x|^2 of the block's rows: 4 threads per row (the first 256 threads)
  {
    const int r = tid >> 2, part = tid & 3;
    float s = 0.f;
    const float* xp = r < 2 * MAXN ? fv::block_row(a, t, h, r) : nullptr;
    if (xp) {
      float4 u[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) { const int e = 4 * part + 16 * k; u[k] = e < d ? *reinterpret_cast<const float4*>(xp + e) : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
      for (int k = 0; k < 16; ++k) s += (u[k].x * u[k].x + u[k].y * u[k].y) + (u[k].z * u[k].z + u[k].w * u[k].w);
    }
    s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
    if (xp && part == 0) s_diag[r] = 0.5f * a.c * a.c * s;
  }
  __syncthreads();
  if (tid < Nc) {
    float best = -INFINITY;
#pragma unroll
    for (int p = 0; p < NPART; ++p) best = fmaxf(best, s_pm[p][tid]);
    s_M[tid] = best;
  }
  __syncthreads();
  if (tid == 0) {
    // running maxima M_1..M_Nc, then the groups from the largest prefix down
    float run = -INFINITY;
    for (int n = 0; n < Nc; ++n) { run = fmaxf(run, s_M[n]); s_M[n] = run; }
    int g = 0; float L = s_M[Nc - 1];
    s_L[0] = L;
    for (int k = Nc - 1; k >= 0; --k) {
      if (L - s_M[k] > SPAN) { ++g; L = s_M[k]; s_L[g] = L; }
      s_grp[k] = g;
    }
    s_ng = g + 1;
  }
  __syncthreads();
  // Q[n] = sum_m F_q[n][m], 32 threads per query row (its own small pass: as two more accumulators of the feature pass below it
  // pushed that loop over the 128 registers a 1024-thread workgroup has)
  {
    const int n = tid / MAXN, part = tid & (MAXN - 1);
    float sq = 0.f;
    if (n < Nq) {
      const float* row = a.w.eq + ((size_t)(t * Nq + n) * H + h) * mp;
      const float sub = s_diag[n] + s_mx[n];
      for (int j = part; j < m; j += MAXN) sq += a.ratio * expf(row[j] - sub) + a.re;
    }
#pragma unroll
    for (int off = MAXN / 2; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if (part == 0) s_Q[n] = sq;
  }
  const bool has_tile = 16 * wv < d;        // this wave's 16 channels of out = S V (d <= 256: at most one tile per wave)
  const int tq = (Nq + 15) / 16;
  const int ng = s_ng;
  int it = 0;
  for (int g = 0; g < ng; ++g) {
    const float L = s_L[g];
    int klo = Nc, khi = -1;
    for (int k = 0; k < Nc; ++k)
      if (s_grp[k] == g) { klo = min(klo, k); khi = max(khi, k); }
    const int tk = (khi + 16) / 16;          // key tiles that hold a shot of this group's prefixes
    // rows as 32-bit element offsets from the feature buffers (NONE: no such row) - as pointers they were eight registers of the loop
    constexpr unsigned NONE = 0xffffffffu;
    unsigned qrow[2], krow[2]; float qsub[2], ksub[2];
    // opaque, so that the rows' addresses are formed here, per group, and not kept from before the loop.  Steers register allocation
    // only: with it (and the one behind the feature pass) the kernel takes 120 VGPRs and no scratch, -Rpass-analysis=kernel-resource-usage;
    // a compiler that ignores it gives the same results with spills
    int lr_g = lr;
    asm volatile("" : "+v"(lr_g));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = 16 * i + lr_g;
      qrow[i] = r < Nq ? (unsigned)(((t * Nq + r) * H + h) * mp) : NONE;
      krow[i] = r <= khi ? (unsigned)(((t * Nc + r) * H + h) * mp) : NONE;      // later shots may lie above L: not exponentiated
      qsub[i] = r < Nq ? s_diag[r] + s_mx[r] : 0.f;
      ksub[i] = r <= khi ? s_diag[Nq + r] + L : 0.f;
    }
    f32x4_t acc[2][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
    auto ldd = [&](const float* base, unsigned row, int j) { return (row != NONE && j < mp) ? *reinterpret_cast<const float4*>(base + row + j) : make_float4(0.f, 0.f, 0.f, 0.f); };
    auto feat = [&](unsigned row, int j, float sub, float add, const float4 dd) {      // ratio exp(dd - sub) + add, 0 beyond m
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row == NONE || j >= mp) return f;
      f.x = j < m ? a.ratio * expf(dd.x - sub) + add : 0.f; f.y = j + 1 < m ? a.ratio * expf(dd.y - sub) + add : 0.f;
      f.z = j + 2 < m ? a.ratio * expf(dd.z - sub) + add : 0.f; f.w = j + 3 < m ? a.ratio * expf(dd.w - sub) + add : 0.f;
      return f;
    };
    // two 16-feature chunks per trip, the dd of trip + 1 requested before the exponentials of this trip (as F2)
    float4 dq[2][2], dk[2][2];
    auto fetch = [&](int jb) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = jb + 16 * NW * u + 4 * lq;
#pragma unroll
        for (int i = 0; i < 2; ++i) { dq[u][i] = ldd(a.w.eq, qrow[i], j); dk[u][i] = ldd(a.w.ek, krow[i], j); }
      }
    };
    fetch(16 * wv);
    for (int jb = 16 * wv; jb < mp; jb += 32 * NW) {
      float4 cq[2][2], ck[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) { cq[u][i] = dq[u][i]; ck[u][i] = dk[u][i]; }
      if (jb + 32 * NW < mp) fetch(jb + 32 * NW);
      float4 fa[2][2], fb[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = jb + 16 * NW * u + 4 * lq;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[u][i] = feat(qrow[i], j, qsub[i], a.re, cq[u][i]);
          fb[u][i] = feat(krow[i], j, ksub[i], 0.f, ck[u][i]);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            if (i >= tq || jj >= tk) continue;
            acc[i][jj] = mfma4(fa[u][i].x, fb[u][jj].x, acc[i][jj]); acc[i][jj] = mfma4(fa[u][i].y, fb[u][jj].y, acc[i][jj]);
            acc[i][jj] = mfma4(fa[u][i].z, fb[u][jj].z, acc[i][jj]); acc[i][jj] = mfma4(fa[u][i].w, fb[u][jj].w, acc[i][jj]);
          }
    }
    // fold the sixteen waves: A[n][j] (C layout: n = 16 i + 4 lq + r, j = 16 jj + lr)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) *reinterpret_cast<f32x4_t*>(red + (((wv * 2 + i) * 2 + jj) * 64 + lane) * 4) = acc[i][jj];
    __syncthreads();
    if (wv < 4) {
      const int i = wv >> 1, jj = wv & 1;            // wave wv folds tile (i, jj), in a fixed order
      f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const f32x4_t vv = *reinterpret_cast<const f32x4_t*>(red + (((k * 2 + i) * 2 + jj) * 64 + lane) * 4);
        s[0] += vv[0]; s[1] += vv[1]; s[2] += vv[2]; s[3] += vv[3];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s_A[(16 * i + 4 * lq + r) * (MAXN + 1) + 16 * jj + lr] = s[r];
    }
    __syncthreads();
    // Everything per lane below is derived from a lane id the compiler cannot see through: hoisted out of the group loop as
    // loop-invariant, the out phase's sixteen addresses stayed live across the feature pass and went to scratch around it.
    // (120 VGPRs and no scratch with it, 128 and 196 bytes of scratch per lane without.)
    int tid_o = tid;
    asm volatile("" : "+v"(tid_o));
    const int lane_o = tid_o & 63, lr = lane_o & 15, lq = lane_o >> 4, e = 16 * wv + lr;
    // the value rows of this wave's channels, B operand of out = S V (loaded behind the feature pass: its registers are the loop's)
    float bv[MAXN / 4];
#pragma unroll
    for (int ks = 0; ks < MAXN / 4; ++ks) { const int np = 4 * ks + lq; bv[ks] = (has_tile && np <= khi) ? a.v[((size_t)(t * Nc + np) * H + h) * d + e] : 0.f; }
    // the prefixes of this group: kk + 1 shots
    for (int kk = klo; kk <= khi; ++kk, ++it) {
      const int buf = it & 1;
      {
        const int n = tid_o / MAXN, j = tid_o & (MAXN - 1);
        float sv = 0.f;
        if (n < Nq && j <= kk) {
          const float dg = s_diag[Nq + j];
          sv = expf((dg + L) - (dg + s_M[kk])) * s_A[n * (MAXN + 1) + j] + a.re * s_Q[n];
        }
        s_S[buf][n * (MAXN + 1) + j] = sv;
#pragma unroll
        for (int off = MAXN / 2; off > 0; off >>= 1) sv += __shfl_xor(sv, off, 64);
        if (j == 0) s_D[buf][n] = sv;
      }
      __syncthreads();        // one barrier per prefix: S / D alternate between two buffers
      if (has_tile) {
        f32x4_t o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < MAXN / 4; ++ks) {
          if (4 * ks > kk) continue;
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (i < tq) o[i] = mfma4(s_S[buf][(16 * i + lr) * (MAXN + 1) + 4 * ks + lq], bv[ks], o[i]);
        }
        float* ob = a.out + ((size_t)kk * T + t) * Nq * ((size_t)d * H) + (size_t)e * H + h;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int nn = 16 * i + 4 * lq + r;
            if (nn < Nq) ob[(size_t)nn * ((size_t)d * H)] = o[i][r] / s_D[buf][nn];
          }
      }
    }
  }
}

// favor2.h's shapes, and feature buffers below 2^31 elements: the sweep kernel addresses their rows by 32-bit offsets
inline bool applies(const FavorDims& f) {
  const size_t mp = (size_t)(f.m + 15) / 16 * 16;
  return fv::applies(f) && f.rows_q() * mp <= 0x7fffffffu && f.rows_k() * mp <= 0x7fffffffu;
}
inline size_t ws_need(const FavorDims& f) {
  if (!applies(f)) return 0;
  size_t n = 0;
  carve(f, nullptr, 0, &n);
  return n;
}
inline int forward(const FavorDims& f, const float* q, const float* k, const float* v, const float* proj, float* out, void* ws, size_t ws_bytes,
                   hipStream_t s) {
  if (!applies(f)) {
    set_error("favor_prefix_fwd: Nq, Nc <= %d, d %% 16 == 0, d <= 256, 16 <= m <= %d, T N H m < 2^31 only (got Nq=%d Nc=%d d=%d m=%d): loop mlhot_favor_fwd over the prefixes",
              MAXN, fv::FCH * NPMAX / 4, f.Nq, f.Nc, f.d, f.m);
    return MLHOT_ERR_UNSUPPORTED;
  }
  const Ws p = carve(f, ws, ws_bytes);
  if (!p.ok) { set_error("favor_prefix_fwd: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  fv::Args a = fv::make_args(f, p.w, q, k, v, proj);
  a.out = out;
  const int th = f.T * f.H, R = f.Nq + f.Nc, rk = (int)f.rows_k();
  {
    ProfScope ps("favor_prefix.f1", s);
    if (R <= 32) hipLaunchKernelGGL((fv::f1_kernel<2>), dim3(th, p.w.nch), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((fv::f1_kernel<4>), dim3(th, p.w.nch), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor_prefix.f1"));
  {
    ProfScope ps("favor_prefix.keymax", s);
    hipLaunchKernelGGL(keymax_kernel, dim3((rk + 3) / 4), dim3(256), 0, s, (const float*)p.w.ek, rk, f.m, p.w.mp, p.kmax);
  }
  MLHOT_TRY(check_launch("favor_prefix.keymax"));
  {
    ProfScope ps("favor_prefix.sweep", s);
    hipLaunchKernelGGL(sweep_kernel, dim3(th), dim3(NT), 0, s, a, (const float*)p.kmax);
  }
  return check_launch("favor_prefix.sweep");
}

}  // namespace fp
#endif
}  // namespace mlhot
