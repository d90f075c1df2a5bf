// nn.Linear forward for THOUSANDS of rows with a ROW-INVARIANCE guarantee (the prefix sweep's folded Linears):
//
//   y[M][N] = act([src_0 | src_1][M][K0 + K1] w[N][K0 + K1]^T + b)
//
// The bits of output row i depend on the input rows that map to it, on w, b, K0, K1, N and act - not on M, not on the row's index
// or its place in a tile, not on the grid, not on which rows share the launch.  mlhot_linear_fwd picks its kernel by M (few-row
// kernel, 16- and 64-row tiles); here there is ONE kernel and nothing in it looks at M except the masks:
//   * every output element is one accumulator chain of v_mfma_f32_16x16x4_f32 over k = 0, 4, 8, .. in chunks of KC = 32: the
//     order is a function of K0 + K1 alone; no split-K, no atomics, no fold between waves;
//   * rows >= M are read as zeros and never stored, columns >= N are read as zeros and never stored, the k tail past K is zero
//     for every row alike;
//   * the operands go through LDS in MFMA lane order (linear_skinny.h's: lane (lr, lq) holds 4 consecutive k of its row, MFMA i
//     of the four that consume them pairs element i of A with element i of B), so a row's products are the same whatever lr it
//     lands on.  That an fp32 MFMA computes an output element the same way at every position of the tile is the one assumption;
//     tests/test_linear_rows_gpu.py measures it (permuted rows, shifted rows).
// Row maps: output row i reads source row (i / rep) % period (period == 0: no wrap), per source - the decoder features of one
// batch serve every prefix (period = T * Nq), a per-task vector serves its Nq targets (rep = Nq); nothing is materialised.
//
// Workgroup: 256 threads, 64 rows x 64 columns; wave (wr, wc) owns 32 x 32 = 2 x 2 MFMA tiles.  x and w chunks [64][32] are staged
// through LDS with a row stride of 40 floats: the ds_read_b128 of lane (lr, lq) is at dword 40 lr + 4 lq (+ 16 per k step), and
// 40 lr mod 64 takes 8 distinct multiples of 8 over any 8 consecutive lr, so the 16-lane groups of a b128 read ({0-3, 12-15,
// 20-27}, ..) touch 16 distinct 4-bank slots - conflict-free; the ds_write_b128 of 8 consecutive threads covers one row's 32
// dwords.  The next chunk's global loads are issued before the current chunk's MFMAs.
#pragma once
#include "common.h"
#include "linear_skinny.h"
#include "../../include/mlhot.h"

#ifndef MLHOT_HOSTSIM
namespace mlhot {
namespace lr {

constexpr int TM = 64, TN = 64, KC = 32, LDS_LD = 40;

struct Src { const float* x; long long ld; int rep, period; };
struct Args {
  Src s0, s1;
  const float* w; const float* b; float* y;
  long long ldy;
  int M, N, K0, K, act;
};

__device__ __forceinline__ long long src_row(const Src& s, int i) {
  const int r = s.rep > 1 ? i / s.rep : i;
  return s.period > 0 ? r % s.period : r;
}

__global__ __launch_bounds__(256) void fwd_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float xs[TM * LDS_LD];
  __shared__ __attribute__((aligned(16))) float ws[TN * LDS_LD];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int wr = wv >> 1, wc = wv & 1;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  // staging: thread t carries k offset 4 (t & 7) of rows (t >> 3) and (t >> 3) + 32, of x and of w
  const int sk = 4 * (tid & 7), sr = tid >> 3;
  const float* px0[2]; const float* px1[2]; const float* pw[2];
  bool okx[2], okw[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int m = m0 + sr + 32 * h, n = n0 + sr + 32 * h;
    okx[h] = m < a.M; okw[h] = n < a.N;
    const int mm = okx[h] ? m : 0;
    px0[h] = a.s0.x + (size_t)src_row(a.s0, mm) * a.s0.ld;
    px1[h] = a.s1.x ? a.s1.x + (size_t)src_row(a.s1, mm) * a.s1.ld - a.K0 : px0[h];      // indexed by the layer's k as well
    pw[h] = a.w + (size_t)(okw[h] ? n : 0) * a.K;
  }
  float4 gx[2], gw[2];
  auto fetch = [&](int kb) {
    const int k = kb + sk;
    const bool kin = k < a.K, first = k < a.K0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      gx[h] = sk::ld4((first ? px0[h] : px1[h]) + k, kin && okx[h]);
      gw[h] = sk::ld4(pw[h] + k, kin && okw[h]);
    }
  };
  // which of the wave's two column tiles hold a column < N (wave-uniform; a skipped tile's MFMAs would only produce masked columns)
  const bool nt_on[2] = {n0 + 32 * wc < a.N, n0 + 32 * wc + 16 < a.N};
  sk::f32x4_t acc[2][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
  const float* xa = xs + (32 * wr + lr) * LDS_LD + 4 * lq;
  const float* wb = ws + (32 * wc + lr) * LDS_LD + 4 * lq;
  fetch(0);
  for (int kb = 0; kb < a.K; kb += KC) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<float4*>(xs + (sr + 32 * h) * LDS_LD + sk) = gx[h];
      *reinterpret_cast<float4*>(ws + (sr + 32 * h) * LDS_LD + sk) = gw[h];
    }
    __syncthreads();
    if (kb + KC < a.K) fetch(kb + KC);
#pragma unroll
    for (int s = 0; s < KC / 16; ++s) {
      const float4 a0 = *reinterpret_cast<const float4*>(xa + 16 * s), a1 = *reinterpret_cast<const float4*>(xa + 16 * LDS_LD + 16 * s);
      const float4 b0 = *reinterpret_cast<const float4*>(wb + 16 * s), b1 = *reinterpret_cast<const float4*>(wb + 16 * LDS_LD + 16 * s);
      if (nt_on[0]) {
        acc[0][0] = sk::mfma4(a0.x, b0.x, acc[0][0]); acc[1][0] = sk::mfma4(a1.x, b0.x, acc[1][0]);
        acc[0][0] = sk::mfma4(a0.y, b0.y, acc[0][0]); acc[1][0] = sk::mfma4(a1.y, b0.y, acc[1][0]);
        acc[0][0] = sk::mfma4(a0.z, b0.z, acc[0][0]); acc[1][0] = sk::mfma4(a1.z, b0.z, acc[1][0]);
        acc[0][0] = sk::mfma4(a0.w, b0.w, acc[0][0]); acc[1][0] = sk::mfma4(a1.w, b0.w, acc[1][0]);
      }
      if (nt_on[1]) {
        acc[0][1] = sk::mfma4(a0.x, b1.x, acc[0][1]); acc[1][1] = sk::mfma4(a1.x, b1.x, acc[1][1]);
        acc[0][1] = sk::mfma4(a0.y, b1.y, acc[0][1]); acc[1][1] = sk::mfma4(a1.y, b1.y, acc[1][1]);
        acc[0][1] = sk::mfma4(a0.z, b1.z, acc[0][1]); acc[1][1] = sk::mfma4(a1.z, b1.z, acc[1][1]);
        acc[0][1] = sk::mfma4(a0.w, b1.w, acc[0][1]); acc[1][1] = sk::mfma4(a1.w, b1.w, acc[1][1]);
      }
    }
    __syncthreads();
  }
  // C lane (lr, lq) reg r = C[row 4 lq + r][col lr]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + 32 * wc + 16 * j + lr;
    if (n >= a.N) continue;
    const float bn = a.b ? a.b[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 32 * wr + 16 * i + 4 * lq + r;
        if (m < a.M) a.y[(size_t)m * a.ldy + n] = act_apply(a.act, acc[i][j][r] + bn);
      }
  }
}

}  // namespace lr
}  // namespace mlhot
#endif

namespace mlhot {

// the shapes the kernel serves (k ranges in float4 steps); pointers and leading dimensions are checked per call
inline bool linear_rows_shape_ok(int k0, int k1, int N) {
#ifdef MLHOT_HOSTSIM
  (void)k0; (void)k1; (void)N; return false;
#else
  return k0 > 0 && k0 % 4 == 0 && k1 >= 0 && k1 % 4 == 0 && N >= 1 && (long long)k0 + k1 < (1 << 30);
#endif
}

inline int linear_rows_forward(const mlhot_rows_src* src, int n_src, const float* w, const float* b, float* y, int ldy, int M, int N, int act,
                               hipStream_t stream) {
  if (!src || (n_src != 1 && n_src != 2) || !w || !y || M < 1 || N < 1 || ldy < N) { set_error("linear_rows_fwd: bad argument"); return MLHOT_ERR_ARG; }
  for (int i = 0; i < n_src; ++i)
    if (!src[i].x || src[i].rep < 1 || src[i].period < 0 || src[i].k < 0) { set_error("linear_rows_fwd: bad source %d (x, rep >= 1, period >= 0)", i); return MLHOT_ERR_ARG; }
#ifdef MLHOT_HOSTSIM
  (void)b; (void)act; (void)stream; set_error("linear_rows: GPU build only"); return MLHOT_ERR_ARG;
#else
  const int k0 = src[0].k, k1 = n_src == 2 ? src[1].k : 0;
  bool ok = linear_rows_shape_ok(k0, k1, N) && act >= 0 && act <= 2 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  for (int i = 0; ok && i < n_src; ++i) ok = src[i].k == 0 || sk::aligned4(src[i].x, src[i].ld);
  if (!ok) {
    set_error("linear_rows_fwd: needs K0 > 0, K0 %% 4 == 0, K1 %% 4 == 0, 16-byte aligned source rows and weights, act in 0..2 (K0=%d K1=%d N=%d act=%d)",
              k0, k1, N, act);
    return MLHOT_ERR_UNSUPPORTED;
  }
  lr::Args a{};
  a.s0 = lr::Src{src[0].x, src[0].ld, src[0].rep, src[0].period};
  a.s1 = k1 > 0 ? lr::Src{src[1].x, src[1].ld, src[1].rep, src[1].period} : lr::Src{nullptr, 0, 1, 0};
  a.w = w; a.b = b; a.y = y; a.ldy = ldy; a.M = M; a.N = N; a.K0 = k0; a.K = k0 + k1; a.act = act;
  ProfScope ps("linear_rows", stream);
  hipLaunchKernelGGL(lr::fwd_kernel, dim3((unsigned)((M + lr::TM - 1) / lr::TM), (unsigned)((N + lr::TN - 1) / lr::TN)), dim3(256), 0, stream, a);
  return check_launch("linear_rows_fwd");
#endif
}

}  // namespace mlhot
