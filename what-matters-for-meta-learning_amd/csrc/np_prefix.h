// The query tail of the vanilla CNP / ANP family for a whole PREFIX SWEEP in one launch: mu[i] is np_query.h's
// tail against the first ks[i] context shots of every task, for K strictly increasing prefix lengths, test mode, forward only.
//
//   latent     z [K, T, dz] (agg_prefixes' rows at ks through r_to_z): mu_i = decoder0([x | z_i[t]]).  The x half of decoder layer 1
//              is the head of that layer's accumulator chain and does not see the prefix: it is computed once per tile (s_hx) and
//              every prefix continues the chain from it over the z half - the bits of np_query.h's one chain over [x | z].
//   attention  kh, vh [T, Nc, 8, d] (the head projections of all Nc shots).  The key features of prefix k are
//              F_k[j] = ratio (exp(dd_k[j] - diag_k[j] - M_k) + 1e-4) for j < k, M_k = the maximum of dd_k over all tasks, heads,
//              features and the first k shots: the prefix enters through the scalar M_k and the column count alone.  Key side, two
//              launches into the workspace: favor_cached.h's K1 (dd_k, unmasked - one chain per element, so a row's bits are those
//              of the masked launch) and np.prefix_keys (per (task, head, shot): the maximum over the features, and diag_k).  The
//              sweep kernel folds the shot maxima into the running maxima M_1 .. M_Nc (a maximum is exact in any order).
//              Per head h, ONCE for all prefixes of the workgroup: q_h, dd_q, the row maxima, F_q (np_query.h's steps 1 - 3, with
//              diag_q formed as favor_cached.h's query kernel forms it, 0.5 c^2 |q|^2 from the unscaled q) and the value rows in
//              registers.  Then the prefixes in ascending order; while M_k stays what it was, S = F_q F_k^T is kept (the M_k
//              GROUPING: exact - M_k is a running maximum, so equal values are neighbours and there are at most K groups; a new
//              value builds F_k from dd_k on the fly and S over the columns j < the largest k here).  A prefix is then column sums
//              in shot order: D_k = S[:, 0] + .. + S[:, k - 1] (one running sum per row, kept for every k) and
//              out_h = S[:, :k] V[:k] / D_k (columns >= k enter the chain as zeros, as a masked state's do) into the prefix's
//              merged tile (order e * 8 + h).  Behind the heads, per prefix: r = merged Wo^T + b as ONE chain over e * 8 + h -
//              linear_rows' order, so the launch follows the composed route's arithmetic step by step -, z = r_to_z(r) behind x,
//              and the decoder as in the latent kind.
// Grid (task x 16-row target tile, chunk of prefixes), 256 threads, no atomics, plain vector stores; a workgroup depends on no
// other.  A merged tile is 32.5 KB, so an attention workgroup takes 2 prefixes (a latent one 8): the query side of a tile is
// computed ceil(K / 2) times for a sweep.  The sweep's grid is below the CU count at the shapes it is used at, where the chunks run
// side by side and a smaller chunk is a shorter launch.
//
// INVARIANCE.  The bits of mu[i, t, n, :] depend only on x[t, n], the first ks[i] shots of the batch, the parameters and the
// dimensions - not on Nq, on n's place in its tile, on the other target rows, or on which other prefixes were requested:
//   * a workgroup owns 16 rows and everything of them; rows >= Nq are read as zeros and never stored, and no sum mixes rows;
//   * np_query.h's rules for the accumulator chains: every product is v_mfma_f32_16x16x4_f32 with ONE chain per output element
//     over k = 0, 16, 32, ..; S is four chains (wave w takes the 16-feature chunks w, w + 4, ..) folded 0, 1, 2, 3;
//   * what a prefix reads of the key side is dd_k and diag_k of its own shots (a row's bits do not depend on the other rows) and
//     M_k, a maximum over its own shots; S's column j is a function of F_q, row j and M_k alone, so whether S was kept from the
//     previous prefix or rebuilt - that is, which other prefixes share the workgroup - does not change a bit; columns >= k are
//     masked by index, never by value, so what they hold (an Inf where a later shot towers over M_k) goes nowhere;
//   * D_k adds the columns 0 .. k - 1 in order; the out chain runs over the 32 key slots with zeros from k on; r_k is one chain over
//     the merged tile; all of it a function of k and the dimensions.
// LDS (attention): [x | z] 8.5 KB, c q_h / r 4.5 KB, the unscaled q_h 4.5 KB, dd / F_q 18.5 KB (the decoder's two hidden tiles
// later), the merged tiles of 2 prefixes 65 KB, the x half of decoder layer 1 8.5 KB, S's fold buffer 8 KB, S and its running sums
// 4.2 KB, the maxima 1.2 KB: 123 KB, one workgroup per CU.  Row strides are 8 mod 32 dwords as in np_query.h.
#pragma once
#include "common.h"
#include "np_query.h"

namespace mlhot {

constexpr int NP_PREFIX_MAXK = 32;

inline bool np_prefix_ok(const mlhot_np_dims& d, int K) {
#ifdef MLHOT_HOSTSIM
  (void)d; (void)K; return false;
#else
  return K >= 1 && K <= NP_PREFIX_MAXK && d.Nc >= 1 && d.Nc <= 32 && np_query_ok(d);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace npx {

using nq::f32x4_t;
using nq::ld4;
using nq::mfma4;
using nq::QT;
using nq::H;
using nq::LDXZ;
using nq::LDQ;
using nq::LDF;
using nq::LDH;
using nq::LDS_S;
using nq::MAXNC;

using nq::LDM;
constexpr int pc(bool attn) { return attn ? 2 : 8; }      // prefixes per workgroup: a merged tile each in the attention kernel

struct Args {
  nq::Args q;                              // np_query.h's: q.v = vh, q.z = z [K, T, dz], q.Nc = all the shots, q.mu [K, T, Nq, y]
  const float *dd, *diag, *pmax;           // the key side in the workspace: dd_k [T][H][Nc][mp], diag_k and the shot maxima [T][H][Nc]
  int K, ks[NP_PREFIX_MAXK];
};

struct Ws { float *dd, *diag, *pmax; fc::State st; size_t floats; };
inline Ws carve_ws(int T, int Nc, int m, void* ws) {
  Ws w{};
  w.st = fc::carve_state(T, H, Nc, m, ws);
  const size_t n = align_up((size_t)T * H * Nc, 64);
  w.dd = w.st.fk; w.diag = w.st.fk + w.st.floats; w.pmax = w.diag + n;
  w.floats = w.st.floats + 2 * n;
  return w;
}

// ---- key side, launch 2: per (task, head, shot) the maximum of dd_k over the features, and diag_k as favor_cached.h's K2 has it ----
__global__ __launch_bounds__(256) void keys_kernel(const fc::Args a, float* diag, float* pmax) {
  const int tid = threadIdx.x, th = blockIdx.x, t = th / a.H, h = th % a.H;
  const int r = tid >> 3, part = tid & 7;          // 32 rows x 8 threads
  const float dg = ft::key_diag(r < a.Nc ? a.x + ((size_t)(t * a.Nc + r) * a.H + h) * a.d : nullptr, a.d, a.sc.c, tid);
  float best = -INFINITY;
  if (r < a.Nc)
    for (int f = part; f < a.m; f += 8) best = fmaxf(best, a.fk[((size_t)th * a.Nc + r) * a.mp + f]);
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if (r < a.Nc && part == 0) { diag[(size_t)th * a.Nc + r] = dg; pmax[(size_t)th * a.Nc + r] = best; }
}

// nq::tile_linear with a row stride of W of its own (ldw) and the chain's start value: store(r, row, n, chain from init(row, n) + b[n])
template <int NT, class Init, class Store>
__device__ __forceinline__ void tile_linear_from(const float* A, int lda, const float* W, int ldw, const float* b, int K, int N, int wv, int lr, int lq,
                                                 Init init, Store store) {
  const int ntile = (N + 15) / 16;
  for (int t0 = wv; t0 < ntile; t0 += 4 * NT) {
    const float* brow[NT]; bool on[NT]; f32x4_t acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = 16 * (t0 + 4 * j) + lr;
      on[j] = t0 + 4 * j < ntile;
      brow[j] = n < N ? W + (size_t)n * ldw + 4 * lq : nullptr;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][r] = on[j] && n < N ? init(4 * lq + r, n) : 0.f;
    }
    nq::mm_tiles<NT>(A + lr * lda + 4 * lq, brow, on, K, lq, acc);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = 16 * (t0 + 4 * j) + lr;
      if (!on[j] || n >= N) continue;
      const float bn = b ? b[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) store(r, 4 * lq + r, n, acc[j][r] + bn);
    }
  }
}

template <bool ATTN>
__global__ __launch_bounds__(256) void sweep_kernel(const Args pa) {
  constexpr int PC = pc(ATTN);
  const nq::Args& a = pa.q;
  __shared__ __attribute__((aligned(16))) float s_xz[QT * LDXZ];
  __shared__ __attribute__((aligned(16))) float s_hx[QT * LDH];
  __shared__ __attribute__((aligned(16))) float s_f[ATTN ? QT * LDF : 2 * QT * LDH];
  __shared__ __attribute__((aligned(16))) float s_q[ATTN ? QT * LDQ : 4];
  __shared__ __attribute__((aligned(16))) float s_o[ATTN ? QT * LDQ : 4];
  __shared__ __attribute__((aligned(16))) float s_mg[ATTN ? PC * QT * LDM : 4];
  __shared__ __attribute__((aligned(16))) float s_red[ATTN ? 4 * 2 * 64 * 4 : 4];
  __shared__ float s_S[ATTN ? QT * LDS_S : 1], s_Dc[ATTN ? QT * LDS_S : 1], s_cm[ATTN ? 8 * MAXNC : 1], s_M[MAXNC], s_diag[QT], s_pm[4][QT];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int t = blockIdx.x / a.ntile, n0 = (blockIdx.x % a.ntile) * QT;
  const int p0 = blockIdx.y * PC, npre = min(PC, pa.K - p0);
  const int Nq = a.Nq, dw = a.dw, dz = a.dz, T = a.T;
  {
    const int r = tid >> 4, n = n0 + r, e = 4 * (tid & 15);
    if (e < dw) *reinterpret_cast<float4*>(s_xz + r * LDXZ + e) = ld4(a.x + ((size_t)t * Nq + (n < Nq ? n : 0)) * dw + e, n < Nq);
  }
  if constexpr (ATTN) {
    // the shot maxima over all tasks and heads: thread (slice, shot) folds every eighth (task, head), then the running maxima
    const int Nc = a.Nc, j = tid & 31, sl = tid >> 5;
    float best = -INFINITY;
    if (j < Nc)
      for (int th = sl; th < T * H; th += 8) best = fmaxf(best, pa.pmax[(size_t)th * Nc + j]);
    s_cm[sl * MAXNC + j] = best;
  }
  __syncthreads();
  if constexpr (ATTN) {
    if (tid == 0) {
      float run = -INFINITY;
      for (int j = 0; j < a.Nc; ++j) {
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) run = fmaxf(run, s_cm[sl * MAXNC + j]);
        s_M[j] = run;
      }
    }
  }
  // the x half of decoder layer 1: the head of its chain, without the bias
  tile_linear_from<2>(s_xz, LDXZ, a.dec_w[0], dw + dz, nullptr, dw, a.dh, wv, lr, lq, [](int, int) { return 0.f; },
                      [&](int, int row, int n, float v) { s_hx[row * LDH + n] = v; });
  __syncthreads();
  if constexpr (ATTN) {
    const int d = dw, m = a.m, mp = a.mp, Nc = a.Nc;
    const int khi = pa.ks[p0 + npre - 1];                    // the largest prefix of this workgroup: S's columns
    for (int h = 0; h < H; ++h) {
      const size_t th = (size_t)t * H + h;
      // 1. - 3. of np_query.h: c q_h (and q_h itself for diag), dd_q with the row maxima, F_q in place
      nq::tile_linear<1>(s_xz, LDXZ, a.wq_w[h], a.wq_b[h], d, d, wv, lr, lq, [&](int, int row, int n, float v) { s_q[row * LDQ + n] = a.sc.c * v; s_o[row * LDQ + n] = v; });
      __syncthreads();
      {
        const int r = tid >> 4;
        const float s = ft::stage_row<16>(s_o + r * LDQ, nullptr, d, tid & 15, 0.f);      // fc::query_kernel's diag: its sum, then its scale
        if ((tid & 15) == 0) s_diag[r] = 0.5f * a.sc.c * a.sc.c * s;
      }
      {
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        nq::tile_linear<4>(s_q, LDQ, a.proj, nullptr, d, m, wv, lr, lq, [&](int r, int row, int n, float v) { s_f[row * LDF + n] = v; best[r] = fmaxf(best[r], v); });
        ft::rowmax_fold(best, s_pm, wv, lr, lq);
      }
      __syncthreads();
      ft::features_inplace(s_f, LDF, m, mp, s_diag, s_pm, a.sc, tid);
      // head h's value rows (wave = the 16-channel tile of e) in registers
      const bool mine = 16 * wv < d;
      float bv[MAXNC / 4];
      ft::load_v(bv, a.v + ((size_t)t * Nc * H + h) * d, (size_t)H * d, Nc, 16 * wv + lr, lq, mine);
      __syncthreads();
      int Mprev = 0;
      for (int pi = 0; pi < npre; ++pi) {
        const int k = pa.ks[p0 + pi];
        const int Mbits = __builtin_amdgcn_readfirstlane(__float_as_int(s_M[k - 1]));
        if (pi == 0 || Mbits != Mprev) {
          // 4. S = F_q F_k^T with F_k built from dd_k for this M_k (favor_cached.h's K2 formula), np_query.h's chunk order and fold
          Mprev = Mbits;
          const float Mk = __int_as_float(Mbits);
          const float* krow[2]; float sub[2];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int np = 16 * jj + lr;
            krow[jj] = np < khi ? pa.dd + (th * Nc + np) * mp + 4 * lq : nullptr;
            sub[jj] = np < khi ? pa.diag[th * Nc + np] + Mk : 0.f;
          }
          ft::s_tile(s_f, LDF, krow, (khi + 15) / 16, mp / 16, Nc,
                     [&](int jj, int f, bool on, float4 b) { return on ? ft::feature4(b, sub[jj], f, m, a.sc) : make_float4(0.f, 0.f, 0.f, 0.f); }, s_red, s_S);
          if (tid < QT) {                                      // D of every prefix: the running sum over the columns, in shot order
            float s = 0.f;
            for (int np = 0; np < Nc; ++np) { s += s_S[tid * LDS_S + np]; s_Dc[tid * LDS_S + np] = s; }
          }
          __syncthreads();
        }
        // 5. out_h = S[:, :k] V_h[:k] / D_k into prefix pi's merged tile: one chain over the 32 key slots, zeros from k on
        if (mine) {
          const f32x4_t o = ft::sv_chain(s_S, bv, k, lr, lq);
#pragma unroll
          for (int r = 0; r < 4; ++r) s_mg[(pi * QT + 4 * lq + r) * LDM + (16 * wv + lr) * H + h] = o[r] / s_Dc[(4 * lq + r) * LDS_S + k - 1];
        }
      }
    }
    __syncthreads();
  }
  float* h1 = s_f;
  float* h2 = s_f + QT * LDH;
  for (int pi = 0; pi < npre; ++pi) {
    const size_t pt = (size_t)(p0 + pi) * T + t;
    if constexpr (ATTN) {
      // r = merged Wo^T + b (dim_r == dw): one chain over e * 8 + h, then z = r_to_z(r) behind x
      nq::tile_linear<1>(s_mg + pi * QT * LDM, LDM, a.wo_w, a.wo_b, H * dw, dw, wv, lr, lq, [&](int, int row, int n, float v) { s_q[row * LDQ + n] = v; });
      __syncthreads();
      nq::tile_linear<1>(s_q, LDQ, a.r2z_w, a.r2z_b, dw, dz, wv, lr, lq, [&](int, int row, int n, float v) { s_xz[row * LDXZ + dw + n] = v; });
    } else {
      const int r = tid >> 4, e = 4 * (tid & 15);
      if (e < dz) *reinterpret_cast<float4*>(s_xz + r * LDXZ + dw + e) = *reinterpret_cast<const float4*>(a.z + pt * dz + e);
    }
    __syncthreads();
    // decoder0([x | z_k]): layer 1 continues the x half's chain over z
    tile_linear_from<2>(s_xz + dw, LDXZ, a.dec_w[0] + dw, dw + dz, a.dec_b[0], dz, a.dh, wv, lr, lq, [&](int row, int n) { return s_hx[row * LDH + n]; },
                        [&](int, int row, int n, float v) { h1[row * LDH + n] = v > 0.f ? v : 0.f; });
    __syncthreads();
    nq::tile_linear<2>(h1, LDH, a.dec_w[1], a.dec_b[1], a.dh, a.dh, wv, lr, lq, [&](int, int row, int n, float v) { h2[row * LDH + n] = v > 0.f ? v : 0.f; });
    __syncthreads();
    nq::tile_linear<1>(h2, LDH, a.dec_w[2], a.dec_b[2], a.dh, a.y, wv, lr, lq, [&](int, int row, int n, float v) {
      if (n0 + row < Nq) a.mu[(pt * Nq + n0 + row) * a.y + n] = act_apply(a.out_act, v);
    });
  }
}

}  // namespace npx
#endif

inline size_t np_prefix_ws_need(const mlhot_np_dims& d, int K) {
#ifndef MLHOT_HOSTSIM
  if (np_prefix_ok(d, K) && np_query_attends(d)) return npx::carve_ws(d.T, d.Nc, d.m_feat, nullptr).floats * sizeof(float);
#endif
  (void)d; (void)K; return 0;
}

// x_qry [T*Nq, dim_w] -> mu [K, T, Nq, y_dim]: row i against the first ks[i] of the d.Nc context shots.  ks: K HOST ints, strictly
// increasing in 1 .. d.Nc.  Attention: kh, vh [T, Nc, 8, dim_w] and ws (np_prefix_ws_need bytes); otherwise z [K, T, dim_z].
inline int np_prefix_forward(const mlhot_np_dims& d, const mlhot_np_params& p, const float* x_qry, int Nq, const int32_t* ks, int K, const float* kh,
                             const float* vh, const float* z, float* mu, void* ws, size_t ws_bytes, hipStream_t s) {
  if (Nq < 1 || !x_qry || !mu || !ks) { set_error("np_prefix_fwd: bad argument"); return MLHOT_ERR_ARG; }
  if (!np_prefix_ok(d, K)) {
    set_error("np_prefix_fwd serves 1 <= K <= 32 prefixes of 1 <= Nc <= 32 shots within np_query_fwd's envelope (dim_w %% 16 == 0, dim_w <= 64, dim_z %% 4 == 0, "
              "dim_z <= 64, dec_hidden %% 4 == 0, dec_hidden <= 128, y_dim <= 16; attention: dim_r == dim_w, 16 <= m <= 272) on the GPU build "
              "(got K=%d dim_w=%d dim_r=%d dim_z=%d dec_hidden=%d y_dim=%d Nc=%d m=%d)", K, d.dim_w, d.dim_r, d.dim_z, d.dec_hidden, d.y_dim, d.Nc, d.m_feat);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)p; (void)kh; (void)vh; (void)z; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  for (int i = 0; i < K; ++i)
    if (ks[i] < 1 || ks[i] > d.Nc || (i && ks[i] <= ks[i - 1])) { set_error("np_prefix_fwd: ks must be strictly increasing in 1 .. Nc = %d (ks[%d] = %d)", d.Nc, i, ks[i]); return MLHOT_ERR_ARG; }
  const bool attn = np_query_attends(d);
  bool have = p.r2z_w || !attn, al = nq::aligned16(x_qry);
  for (int i = 0; i < 3; ++i) { have = have && p.dec_w[i] && p.dec_b[i]; al = al && nq::aligned16(p.dec_w[i]); }
  if (attn) {
    have = have && kh && vh && p.r2z_b && p.wo_w && p.wo_b && p.proj;
    al = al && nq::aligned16(kh) && nq::aligned16(vh) && nq::aligned16(p.r2z_w) && nq::aligned16(p.wo_w) && nq::aligned16(p.proj) && nq::aligned16(ws);
    for (int h = 0; h < MLHOT_HEADS; ++h) { have = have && p.wq_w[h] && p.wq_b[h]; al = al && nq::aligned16(p.wq_w[h]); }
  } else {
    have = have && z; al = al && nq::aligned16(z);
  }
  if (!have) { set_error("np_prefix_fwd: a null pointer among the context rows and the parameters this mode reads"); return MLHOT_ERR_ARG; }
  if (!al) { set_error("np_prefix_fwd: x_qry, the context rows, the workspace and the weights must be 16-byte aligned"); return MLHOT_ERR_UNSUPPORTED; }
  const long long ntile = ((long long)Nq + nq::QT - 1) / nq::QT;
  if (ntile * d.T >= (1ll << 31)) { set_error("np_prefix_fwd: T ceil(Nq / 16) must stay below 2^31 (chunk the targets)"); return MLHOT_ERR_ARG; }
  npx::Args pa{};
  nq::Args& a = pa.q;
  a.x = x_qry; a.mu = mu; a.z = z; a.v = vh; a.proj = p.proj;
  for (int h = 0; h < MLHOT_HEADS; ++h) { a.wq_w[h] = p.wq_w[h]; a.wq_b[h] = p.wq_b[h]; }
  a.wo_w = p.wo_w; a.wo_b = p.wo_b; a.r2z_w = p.r2z_w; a.r2z_b = p.r2z_b;
  for (int i = 0; i < 3; ++i) { a.dec_w[i] = p.dec_w[i]; a.dec_b[i] = p.dec_b[i]; }
  a.T = d.T; a.Nq = Nq; a.Nc = d.Nc; a.ntile = (int)ntile; a.dw = d.dim_w; a.dz = d.dim_z; a.dh = d.dec_hidden; a.y = d.y_dim;
  a.out_act = d.out_tanh ? ACT_TANH : ACT_NONE;
  pa.K = K;
  for (int i = 0; i < K; ++i) pa.ks[i] = ks[i];
  const int PC = npx::pc(np_query_attends(d));
  const dim3 grid((unsigned)(ntile * d.T), (unsigned)((K + PC - 1) / PC));
  if (attn) {
    const npx::Ws w = npx::carve_ws(d.T, d.Nc, d.m_feat, ws);
    if (!ws || ws_bytes < w.floats * sizeof(float)) { set_error("np_prefix_fwd: workspace too small (%zu < %zu)", ws_bytes, w.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
    fc::Args ka = fc::make_args(d.T, MLHOT_HEADS, 0, d.Nc, d.dim_w, d.m_feat, w.st);
    ka.x = kh; ka.proj = p.proj;
    {
      ProfScope ps("favor.keys1", s);
      if (d.Nc <= 16) hipLaunchKernelGGL((fc::keys1_kernel<1>), dim3(d.T * MLHOT_HEADS, w.st.nch), dim3(256), 0, s, ka);
      else hipLaunchKernelGGL((fc::keys1_kernel<2>), dim3(d.T * MLHOT_HEADS, w.st.nch), dim3(256), 0, s, ka);
    }
    MLHOT_TRY(check_launch("favor.keys1"));
    {
      ProfScope ps("np.prefix_keys", s);
      hipLaunchKernelGGL(npx::keys_kernel, dim3(d.T * MLHOT_HEADS), dim3(256), 0, s, ka, w.diag, w.pmax);
    }
    MLHOT_TRY(check_launch("np.prefix_keys"));
    pa.dd = w.dd; pa.diag = w.diag; pa.pmax = w.pmax;
    a.m = d.m_feat; a.mp = w.st.mp;
    a.sc = ft::Scales(d.dim_w, d.m_feat);
    ProfScope ps("np.prefix", s);
    hipLaunchKernelGGL(npx::sweep_kernel<true>, grid, dim3(256), 0, s, pa);
  } else {
    ProfScope ps("np.prefix", s);
    hipLaunchKernelGGL(npx::sweep_kernel<false>, grid, dim3(256), 0, s, pa);
  }
  return check_launch("np.prefix");
#endif
}

}  // namespace mlhot
