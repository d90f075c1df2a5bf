// The query tail of the vanilla CNP / ANP family in ONE launch: everything of the test-mode forward behind the
// encoder that sees the targets, against a conditioned context.
//
//   attention  x [T*Nq, dw] (the encoder's target rows), the key state of mlhot_favor_keys_fwd (F_k with ratio, + 1e-4 and the
//              batch-global stabiliser already in it), vh [T, Nc, 8, d]:
//              per head h: q_h = x Wq_h^T + b, dd_q = (c q_h) P^T, row maxima, F_q, S = F_q F_k^T, D = rowsum(S), out_h = S V_h / D
//              into the merged tile (order e * 8 + h); then r = merged Wo^T + b, z = r_to_z(r), mu = decoder0([x | z])
//   latent     z [T, dim_z] (the aggregated context, or zeros without a context shot): mu = decoder0([x | z[t]])
// The training tail cannot be one launch - its key stabiliser is a maximum over the whole batch.  Here that maximum sits in the key
// state, so no workgroup depends on another: grid (task x 16-row target tile), 256 threads, no workspace, no atomics.
//
// ROW INVARIANCE, as for linear_rows.h and favor_cached.h: the bits of mu[t, n, :] depend on x[t, n], the state, the parameters and
// the dimensions - not on Nq, on n, on the row's place in its tile or on the other rows.  What makes it so:
//   * a workgroup owns 16 rows and everything of them; rows >= Nq are read as zeros and never stored, and no sum mixes rows;
//   * every matrix product is v_mfma_f32_16x16x4_f32 with ONE accumulator chain per output element over k = 0, 16, 32, .. (each
//     step four MFMAs that pair element i of the lanes' float4s; k past K reads zeros on both sides) - an order that is a function
//     of K alone; the one exception is S, favor_cached.h's: wave w takes the 16-feature chunks w, w + 4, .., the four partial
//     results are folded 0, 1, 2, 3 - a function of m alone; D adds the Nc columns in order;
//   * |c q|^2 is one float4 per lane and a butterfly over the row's 16 lanes (commutative at every level);
//   * an fp32 MFMA computes an output element the same way at every row of its tile - linear_rows.h's one assumption.
// LDS (attention): [x | z] 8.5 KB, c q_h / r 4.5 KB, dd / F_q 18.5 KB (the decoder's two hidden tiles later), the merged tile
// 32.5 KB, S's fold buffer 8 KB, S 2 KB: 76 KB, two workgroups per CU.  Every row stride is 8 mod 32 dwords, so the b128 operand
// reads of lanes (lr, lq) at [lr][4 lq] are conflict-free.
#pragma once
#include "common.h"
#include "linear_skinny.h"
#include "favor_cached.h"
#include "../../include/mlhot.h"

namespace mlhot {

inline bool np_query_attends(const mlhot_np_dims& d) { return d.agg_mode == MLHOT_AGG_ATTENTION && d.Nc > 0; }

// the dimensions the kernel serves (d.Nq is not looked at); pointers are checked per call
inline bool np_query_ok(const mlhot_np_dims& d) {
#ifdef MLHOT_HOSTSIM
  (void)d; return false;
#else
  if (d.T < 1 || d.Nc < 0 || d.agg_mode < 0 || d.agg_mode > 3) return false;
  if (d.dim_w < 16 || d.dim_w % 16 || d.dim_w > 64 || d.dim_z < 4 || d.dim_z % 4 || d.dim_z > 64) return false;
  if (d.dec_hidden < 4 || d.dec_hidden % 4 || d.dec_hidden > 128 || d.y_dim < 1 || d.y_dim > 16) return false;
  if (np_query_attends(d))
    return d.dim_r == d.dim_w && d.Nc <= 32 && d.m_feat >= 16 && d.m_feat <= 272 && favor_cached_ok(d.T, MLHOT_HEADS, d.Nc, d.dim_w, d.m_feat);
  return true;
#endif
}

#ifndef MLHOT_HOSTSIM
namespace nq {

using sk::f32x4_t;
using sk::ld4;
using sk::mfma4;

constexpr int QT = 16, H = MLHOT_HEADS;
constexpr int MAXD = 64, MAXZ = 64, MAXH = 128, MAXNC = 32, MAXM = 272;
constexpr int LDXZ = MAXD + MAXZ + 8;      // [x | z]
constexpr int LDQ = MAXD + 8;              // c q_h, later r
constexpr int LDF = ft::ldf(MAXM);         // dd / F_q
constexpr int LDM = H * MAXD + 8;          // the merged tile
constexpr int LDH = MAXH + 8;              // the decoder's hidden tiles (they lie in the dd buffer)
constexpr int LDS_S = ft::LDS_S;
static_assert(LDXZ % 32 == 8 && LDQ % 32 == 8 && LDF % 32 == 8 && LDM % 32 == 8 && LDH % 32 == 8, "row strides are 8 mod 32 dwords");
static_assert(QT * LDF >= 2 * QT * LDH, "the hidden tiles fit the dd buffer");

struct Args {
  const float* x; float* mu;
  const float *fk, *v, *z, *proj;
  const float *wq_w[H], *wq_b[H];
  const float *wo_w, *wo_b, *r2z_w, *r2z_b, *dec_w[3], *dec_b[3];
  int T, Nq, Nc, ntile, dw, dz, dh, y, m, mp, out_act;
  ft::Scales sc;
};
// SUMMARY (np_query_summary.h) reads favor_summary.h's state through the three context pointers, so that the
// argument block - and with it the per-shot kernels' code - stays what it was: fk = A [T][8][mp][d], v = a [T][8][mp],
// z = vs [T][8][d]; cnt [T][8] (int32) lies 16 floats (M's block) behind vs in that state, which the entry checks.
__device__ __forceinline__ const int32_t* summary_cnt(const Args& a) { return reinterpret_cast<const int32_t*>(a.z + (size_t)a.T * H * a.dw + 16); }

// acc[j] += A[16][K] (LDS; arow = this lane's row + 4 lq) x B_j[16][K]^T (global; brow[j] = this lane's row + 4 lq, nullptr: zeros)
// for the tiles with on[j]: per element one chain over k = 0, 16, 32, ..; the B loads of 64 k are in flight together.
template <int NT>
__device__ __forceinline__ void mm_tiles(const float* arow, const float* const (&brow)[NT], const bool (&on)[NT], int K, int lq, f32x4_t (&acc)[NT]) {
  constexpr int UF = 4;
  for (int c0 = 0; c0 < K; c0 += 16 * UF) {
    float4 bv[UF][NT];
#pragma unroll
    for (int u = 0; u < UF; ++u)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        bv[u][j] = ld4(brow[j] + c0 + 16 * u, brow[j] != nullptr && c0 + 16 * u + 4 * lq < K);
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int k0 = c0 + 16 * u;
      if (k0 >= K) break;
      const float4 av = k0 + 4 * lq < K ? *reinterpret_cast<const float4*>(arow + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (!on[j]) continue;
        acc[j] = mfma4(av.x, bv[u][j].x, acc[j]); acc[j] = mfma4(av.y, bv[u][j].y, acc[j]);
        acc[j] = mfma4(av.z, bv[u][j].z, acc[j]); acc[j] = mfma4(av.w, bv[u][j].w, acc[j]);
      }
    }
  }
}

// store(r, row, n, A[row] . W[n] + b[n]) for the tile's 16 rows and every n < N: wave w takes the 16-column tiles w, w + 4, ..,
// NT of them at a time.  A [16][K] in LDS (stride lda), W [N][K] and b [N] (or nullptr) in global memory, K % 4 == 0.
template <int NT, class Store>
__device__ __forceinline__ void tile_linear(const float* A, int lda, const float* W, const float* b, int K, int N, int wv, int lr, int lq, Store store) {
  const int ntile = (N + 15) / 16;
  for (int t0 = wv; t0 < ntile; t0 += 4 * NT) {
    const float* brow[NT]; bool on[NT]; f32x4_t acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = 16 * (t0 + 4 * j) + lr;
      on[j] = t0 + 4 * j < ntile;
      brow[j] = n < N ? W + (size_t)n * K + 4 * lq : nullptr;
      acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    mm_tiles<NT>(A + lr * lda + 4 * lq, brow, on, K, lq, acc);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = 16 * (t0 + 4 * j) + lr;
      if (!on[j] || n >= N) continue;
      const float bn = b ? b[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) store(r, 4 * lq + r, n, acc[j][r] + bn);      // C lane (lr, lq) reg r = C[row 4 lq + r][col lr]
    }
  }
}

// SUMMARY (with ATTN): the context is favor_summary.h's fixed-size state instead of per-shot key features - steps 4
// and 5 of a head change, everything else is this text for both.
template <bool ATTN, bool SUMMARY = false>
__global__ __launch_bounds__(256) void query_kernel(const Args a) {
  static_assert(ATTN || !SUMMARY, "a summary state belongs to the attention");
  static_assert(4 * QT * ft::ldo(MAXD) <= QT * LDF, "the four partial tiles of F_q A fit into F_q's space");
  __shared__ __attribute__((aligned(16))) float s_xz[QT * LDXZ];
  __shared__ __attribute__((aligned(16))) float s_f[ATTN ? QT * LDF : 2 * QT * LDH];
  __shared__ __attribute__((aligned(16))) float s_q[ATTN ? QT * LDQ : 4];
  __shared__ __attribute__((aligned(16))) float s_mg[ATTN ? QT * LDM : 4];
  __shared__ __attribute__((aligned(16))) float s_red[ATTN && !SUMMARY ? 4 * 2 * 64 * 4 : 4];
  __shared__ float s_S[ATTN && !SUMMARY ? QT * LDS_S : 1], s_D[QT], s_diag[QT], s_pm[4][QT], s_fs[SUMMARY ? QT : 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int t = blockIdx.x / a.ntile, n0 = (blockIdx.x % a.ntile) * QT;
  const int Nq = a.Nq, dw = a.dw, dz = a.dz;
  // the x tile (rows >= Nq: zeros), and in latent mode the task's z behind every row: 16 threads per row, one float4 each
  {
    const int r = tid >> 4, n = n0 + r, e = 4 * (tid & 15);
    if (e < dw) *reinterpret_cast<float4*>(s_xz + r * LDXZ + e) = ld4(a.x + ((size_t)t * Nq + (n < Nq ? n : 0)) * dw + e, n < Nq);
    if (!ATTN && e < dz) *reinterpret_cast<float4*>(s_xz + r * LDXZ + dw + e) = *reinterpret_cast<const float4*>(a.z + (size_t)t * dz + e);
  }
  __syncthreads();
  if constexpr (ATTN) {
    const int d = dw, m = a.m, mp = a.mp, Nc = a.Nc;
    for (int h = 0; h < H; ++h) {
      // 1. c q_h into LDS
      tile_linear<1>(s_xz, LDXZ, a.wq_w[h], a.wq_b[h], d, d, wv, lr, lq, [&](int, int row, int n, float v) { s_q[row * LDQ + n] = a.sc.c * v; });
      __syncthreads();
      // 2. diag = 0.5 |c q|^2; dd = (c q) P^T into LDS with the row maxima
      {
        const int r = tid >> 4, e = 4 * (tid & 15);
        float s = 0.f;
        if (e < d) { const float4 u = *reinterpret_cast<const float4*>(s_q + r * LDQ + e); s = (u.x * u.x + u.y * u.y) + (u.z * u.z + u.w * u.w); }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
        if ((tid & 15) == 0) s_diag[r] = 0.5f * s;
      }
      {
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        tile_linear<4>(s_q, LDQ, a.proj, nullptr, d, m, wv, lr, lq, [&](int r, int row, int n, float v) { s_f[row * LDF + n] = v; best[r] = fmaxf(best[r], v); });
        ft::rowmax_fold(best, s_pm, wv, lr, lq);
      }
      __syncthreads();
      // 3. F_q = ratio exp(dd - diag - rowmax) + ratio 1e-4 in place, zeros at features >= m
      ft::features_inplace(s_f, LDF, m, mp, s_diag, s_pm, a.sc, tid);
      __syncthreads();
      if constexpr (SUMMARY) {
        const size_t th = (size_t)t * H + h;
        // 4. per row: fs = sum_j F_q[j], and the denominator D = sum_j F_q[j] a[j] + eps cnt fs (fsum::query_kernel's step 4)
        {
          const int row = tid >> 4, p = tid & 15;
          const float* av = a.v + th * mp;
          float s[2];
          ft::row_sums(mp, p, s, [&](int j, float (&u)[2]) { const float f = s_f[row * LDF + j]; u[0] += f; u[1] += f * av[j]; });
          if (p == 0) { s_fs[row] = s[0]; s_D[row] = s[1] + (ft::EPS * (float)summary_cnt(a)[th]) * s[0]; }
        }
        // 5. F_q A[t, h], A streamed from memory: wave w takes the 16-feature chunks w, w + 4, .., the four partial tiles go where F_q
        // was (two barriers inside) and fold 0, 1, 2, 3; merged[row][e H + h] = (F_q A + eps vs[e] fs) / D.  The next head writes
        // s_f behind its first barrier.
        ft::stream_product<1>(s_f, LDF, a.fk + th * mp * d, mp, d, wv, lr, lq);
        const float* vs = a.z + th * d;
        for (int idx = tid; idx < QT * d; idx += 256) {
          const int row = idx / d, e = idx - row * d;
          const float s = ft::fold_tiles(s_f, ft::ldo(d), row, e);
          s_mg[row * LDM + e * H + h] = (s + (ft::EPS * vs[e]) * s_fs[row]) / s_D[row];
        }
        continue;
      }
      // 4. S = F_q F_k^T (favor_cached.h's chunk order and fold), D = rowsum(S)
      const float* krow[2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) krow[jj] = 16 * jj + lr < Nc ? a.fk + (((size_t)t * H + h) * Nc + 16 * jj + lr) * mp + 4 * lq : nullptr;
      ft::s_tile(s_f, LDF, krow, (Nc + 15) / 16, mp / 16, Nc, ft::BPlain{}, s_red, s_S);
      ft::s_rowsum(s_S, Nc, s_D);
      // 5. merged[row][e H + h] = sum_n' S[row][n'] v[(t, n', h)][e] / D[row]
      ft::sv_tiles(s_S, s_D, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, d, wv, lr, lq, [&](int row, int e, float o) { s_mg[row * LDM + e * H + h] = o; });
    }
    __syncthreads();
    // r = merged Wo^T + b (dim_r == dw), then z = r_to_z(r) behind x
    tile_linear<1>(s_mg, LDM, a.wo_w, a.wo_b, H * d, dw, wv, lr, lq, [&](int, int row, int n, float v) { s_q[row * LDQ + n] = v; });
    __syncthreads();
    tile_linear<1>(s_q, LDQ, a.r2z_w, a.r2z_b, dw, dz, wv, lr, lq, [&](int, int row, int n, float v) { s_xz[row * LDXZ + dw + n] = v; });
    __syncthreads();
  }
  // decoder0([x | z]): Linear + ReLU, Linear + ReLU, Linear (+ tanh)
  float* h1 = s_f;
  float* h2 = s_f + QT * LDH;
  tile_linear<2>(s_xz, LDXZ, a.dec_w[0], a.dec_b[0], dw + dz, a.dh, wv, lr, lq, [&](int, int row, int n, float v) { h1[row * LDH + n] = v > 0.f ? v : 0.f; });
  __syncthreads();
  tile_linear<2>(h1, LDH, a.dec_w[1], a.dec_b[1], a.dh, a.dh, wv, lr, lq, [&](int, int row, int n, float v) { h2[row * LDH + n] = v > 0.f ? v : 0.f; });
  __syncthreads();
  tile_linear<1>(h2, LDH, a.dec_w[2], a.dec_b[2], a.dh, a.y, wv, lr, lq, [&](int, int row, int n, float v) {
    if (n0 + row < Nq) a.mu[((size_t)t * Nq + n0 + row) * a.y + n] = act_apply(a.out_act, v);
  });
}

using ft::aligned16;

}  // namespace nq
#endif

// x_qry [T*Nq, dim_w] -> mu [T*Nq, y_dim] against a conditioned context: key_state (mlhot_favor_keys_fwd's, for T, 8 heads, d.Nc,
// dim_w, m_feat) and vh [T, Nc, 8, dim_w] for an attention model with Nc > 0, z [T, dim_z] otherwise.  d.Nq is ignored.
inline int np_query_forward(const mlhot_np_dims& d, const mlhot_np_params& p, const float* x_qry, int Nq, const void* key_state, const float* vh,
                            const float* z, float* mu, hipStream_t s) {
  if (Nq < 1 || !x_qry || !mu) { set_error("np_query_fwd: bad argument"); return MLHOT_ERR_ARG; }
  if (!np_query_ok(d)) {
    set_error("np_query_fwd serves dim_w %% 16 == 0, dim_w <= 64, dim_z %% 4 == 0, dim_z <= 64, dec_hidden %% 4 == 0, dec_hidden <= 128, y_dim <= 16 and, "
              "for the attention, dim_r == dim_w, Nc <= 32, 16 <= m <= 272 on the GPU build (got dim_w=%d dim_r=%d dim_z=%d dec_hidden=%d y_dim=%d Nc=%d m=%d)",
              d.dim_w, d.dim_r, d.dim_z, d.dec_hidden, d.y_dim, d.Nc, d.m_feat);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)p; (void)key_state; (void)vh; (void)z; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const bool attn = np_query_attends(d);
  bool have = p.r2z_w || !attn, al = nq::aligned16(x_qry);
  for (int i = 0; i < 3; ++i) { have = have && p.dec_w[i] && p.dec_b[i]; al = al && nq::aligned16(p.dec_w[i]); }
  if (attn) {
    have = have && key_state && vh && p.r2z_b && p.wo_w && p.wo_b && p.proj;
    al = al && nq::aligned16(key_state) && nq::aligned16(vh) && nq::aligned16(p.r2z_w) && nq::aligned16(p.wo_w) && nq::aligned16(p.proj);
    for (int h = 0; h < MLHOT_HEADS; ++h) { have = have && p.wq_w[h] && p.wq_b[h]; al = al && nq::aligned16(p.wq_w[h]); }
  } else {
    have = have && z; al = al && nq::aligned16(z);
  }
  if (!have) { set_error("np_query_fwd: a null pointer among the state and the parameters this mode reads"); return MLHOT_ERR_ARG; }
  if (!al) { set_error("np_query_fwd: x_qry, the state and the weights must be 16-byte aligned"); return MLHOT_ERR_UNSUPPORTED; }
  const long long ntile = ((long long)Nq + nq::QT - 1) / nq::QT;
  if (ntile * d.T >= (1ll << 31)) { set_error("np_query_fwd: T ceil(Nq / 16) must stay below 2^31 (chunk the targets)"); return MLHOT_ERR_ARG; }
  nq::Args a{};
  a.x = x_qry; a.mu = mu; a.z = z; a.v = vh; a.proj = p.proj;
  for (int h = 0; h < MLHOT_HEADS; ++h) { a.wq_w[h] = p.wq_w[h]; a.wq_b[h] = p.wq_b[h]; }
  a.wo_w = p.wo_w; a.wo_b = p.wo_b; a.r2z_w = p.r2z_w; a.r2z_b = p.r2z_b;
  for (int i = 0; i < 3; ++i) { a.dec_w[i] = p.dec_w[i]; a.dec_b[i] = p.dec_b[i]; }
  a.T = d.T; a.Nq = Nq; a.Nc = d.Nc; a.ntile = (int)ntile; a.dw = d.dim_w; a.dz = d.dim_z; a.dh = d.dec_hidden; a.y = d.y_dim;
  a.out_act = d.out_tanh ? ACT_TANH : ACT_NONE;
  ProfScope ps("np.query", s);
  if (attn) {
    const fc::State st = fc::carve_state(d.T, MLHOT_HEADS, d.Nc, d.m_feat, const_cast<void*>(key_state));
    a.fk = st.fk; a.m = d.m_feat; a.mp = st.mp;
    a.sc = ft::Scales(d.dim_w, d.m_feat);
    hipLaunchKernelGGL(nq::query_kernel<true>, dim3((unsigned)(ntile * d.T)), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(nq::query_kernel<false>, dim3((unsigned)(ntile * d.T)), dim3(256), 0, s, a);
  }
  return check_launch("np.query");
#endif
}

}  // namespace mlhot
