// FAVOR+ for K context prefixes of any length: chunked running prefixes, no [mp x d] state.
//
// The targets are the same for every context size, so F_q is computed once; the prefix results are running sums over the shots,
//   F_q A_K = sum_{n < K} (F_q . e_n) v_n^T,   e_n[j] = exp(dd[n, j] - diag[n] - M),
// the per-shot form of favor_cached.h carried across chunks of 32 shots.  Prefix k (the first ks[k] shots; task t's first
// min(ks[k], lens[t])) uses the reference's stabiliser M_k = the maximum of dd over the valid shots < ks[k] of ALL tasks, heads and
// features (fast_attention.py:96-97 on that batch), and the key feature's +1e-4 floor relative to M_k.  The feature's ratio cancels:
//   out_k[q, e] = sum_n (S_k[q, n] + eps fs[q]) v[n, e] / sum_n (S_k[q, n] + eps fs[q]),   S_k[q, n] = sum_j F_q[q, j] exp(dd[n, j] - diag[n] - M_k),
// fs = rowsum(F_q): the numerator is  P_k + eps fs vs_k,  the denominator  p_k + eps fs cnt_k  of favor_summary.h, shot by shot.
//
//   D  grid (task x head x 32-shot chunk, 256-feature chunk): dd of the chunk's shots through ft::keys_dd - the bits favor_keys
//      gives an element - into the workspace, and per shot the maximum over the workgroup's features
//   X  grid (256 shots): smax[n] = the maximum over tasks, heads and feature chunks of shot n's maxima.  M_k is a running maximum
//      of smax, which the sweep takes as it walks.  (A fold inside D needs an atomic or a last-workgroup flag, a fold inside S
//      re-reads T H ceil(mp / 256) floats per shot in every workgroup: a third, tiny launch is the cheaper form.)
//   S  grid (task x head x 16-row target tile): ft::query_front (F_q in LDS once, fc::query_kernel's), then the shots in
//      chunks of 32, ascending.  Per chunk: diag of its keys, the running maxima Mref[n] = max(smax[0 .. n]),
//      S[q, n] = sum_j F_q[q, j] exp(dd[n, j] - diag[n] - Mref[n])  (every exponent <= 0) on the matrix core - wave w takes the
//      16-feature chunks w, w + 4, .. ascending, the waves fold 0, 1, 2, 3 - and the chunk's 32 rows of v in registers.  A member
//      ks[k] inside the chunk: column n < ks[k] is weighted exp(Mref[n] - M_k) <= 1 (1 where equal), gets + eps fs[q] and all later
//      columns are zeros BY INDEX; one MFMA chain over the 32 shot slots against v gives the chunk's part of the numerator, one
//      against ones the denominator's; the carried sums of the earlier chunks enter as exp(M_prev - M_k) P + eps fs vs (p, cnt
//      likewise).  At the end of a chunk the carried P, p (no eps, relative to the chunk's last Mref), vs and cnt take the chunk.
//      No factor ever exceeds 1 and no 0 x inf is formed: a weight is selected, never multiplied in, where a shot is masked.
// Masked rows (n >= lens[t]) of k AND v are never read, nor is their dd (never written).  No atomics; every sum has one order, a
// function of the dimensions and of the member's position alone - so out[k] has the same bits whichever other members are asked for.
// ROW INVARIANCE as in favor_cached.h: a workgroup owns 16 target rows and every feature of them, rows >= Nq are zeros and never
// stored, and every per-row sum is an MFMA chain or a 16-lane butterfly laid out the same way at every row of the tile.
#pragma once
#include "common.h"
#include "favor_cached.h"

namespace mlhot {

constexpr int FAVOR_PREFIX_LONG_MAXK = 64;

inline bool favor_prefix_long_ok(int T, int H, int Nq, int Nc, int d, int m, int K) {
#ifdef MLHOT_HOSTSIM
  (void)T; (void)H; (void)Nq; (void)Nc; (void)d; (void)m; (void)K; return false;
#else
  return Nq >= 1 && Nc >= 1 && K >= 1 && K <= FAVOR_PREFIX_LONG_MAXK && ft::envelope_ok(T, H, d, m) &&
         (long long)T * H * ((Nc + 31) / 32) < (1ll << 31) && (long long)T * H * (((long long)Nq + 15) / 16) < (1ll << 31);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace fpl {

using ft::f32x4_t;
using ft::mfma4;
using ft::EPS;

constexpr int CH = 32;                    // shots per chunk

struct Ws { float *dd, *part, *smax; int Ncp, nch, mp; size_t floats; };
inline Ws carve_ws(int T, int H, int Nc, int m, void* ws) {
  Ws w{};
  w.mp = (m + 15) / 16 * 16; w.nch = (w.mp + ft::KCH - 1) / ft::KCH; w.Ncp = (Nc + CH - 1) / CH * CH;
  const size_t th = (size_t)T * H;
  w.dd = (float*)ws; w.part = w.dd + th * w.Ncp * w.mp; w.smax = w.part + th * w.nch * w.Ncp;
  w.floats = th * w.Ncp * w.mp + th * w.nch * w.Ncp + w.Ncp;
  return w;
}

struct Args {
  const float *q, *k, *v, *proj;
  const int32_t* lens;
  float* out;
  Ws ws;
  int T, H, Nq, Nc, d, m, mp, ntile, K, nsc;      // nsc: the chunks that hold a shot < ks[K - 1]
  ft::Scales sc;
  int ks[FAVOR_PREFIX_LONG_MAXK];
};

// lens[t] held to 0 .. Nc (the host checks 1 .. Nc; the clamp keeps every index in bounds whatever arrives); NULL: all Nc
__device__ __forceinline__ int task_len(const int32_t* lens, int t, int Nc) { return ft::clamp_len(lens, t, 0, Nc); }

// ---- D: dd of one chunk's shots into the workspace, per shot the maximum over this workgroup's features ----------------------
__global__ __launch_bounds__(256) void dd_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float xs[CH * ft::LDX];
  __shared__ float s_w[4 * CH];
  const int th = blockIdx.x / a.nsc, sc = blockIdx.x % a.nsc, t = th / a.H, h = th % a.H, n0 = CH * sc;
  const int ll = min(max(task_len(a.lens, t, a.Nc) - n0, 0), CH);        // the chunk's valid shots; a shot behind lens[t] leaves -inf
  ft::keys_dd<2, true, true>([&](int r) { return a.k + (((size_t)t * a.Nc + n0 + r) * a.H + h) * a.d; }, ll, a.proj, a.sc.c, a.d, a.m, a.mp,
                       a.ws.dd + ((size_t)th * a.ws.Ncp + n0) * a.mp, a.ws.part + ((size_t)th * a.ws.nch + blockIdx.y) * a.ws.Ncp + n0, xs, s_w);
}

// ---- X: per shot the maximum over every task, head and feature chunk ----------------------------------------------------------
__global__ __launch_bounds__(256) void smax_kernel(const Args a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= CH * a.nsc) return;
  const size_t rows = (size_t)a.T * a.H * a.ws.nch;
  float best = -INFINITY;
  for (size_t i = 0; i < rows; ++i) best = fmaxf(best, a.ws.part[i * a.ws.Ncp + n]);
  a.ws.smax[n] = best;
}

// ---- S: one workgroup per (task, head, 16 target rows) walks the shots ---------------------------------------------------------
// NG: the 16-column tiles of d a wave owns (tile wv + 4 i)
template <int NG>
__global__ __launch_bounds__(256) void sweep_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float s_f[ft::QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[ft::QT * ft::LDX];
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * 64 * 4];
  __shared__ float s_S[ft::QT * ft::LDS_S], s_diag[ft::QT], s_pm[4][ft::QT], s_fs[ft::QT], s_kd[CH], s_sm[CH], s_mref[CH];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, q0 = tile * ft::QT;
  const int d = a.d, m = a.m, Nq = a.Nq, Nc = a.Nc, H = a.H, mp = a.mp, LD = ft::ldf(mp);
  // 1. - 3. c q and diag, dd and the row maxima, F_q in place
  ft::query_front([&](int r) { return q0 + r < Nq ? a.q + (((size_t)t * Nq + q0 + r) * H + h) * d : nullptr; }, a.proj, d, m, mp, a.sc, xs, s_f, s_diag, s_pm);
  // 4. fs = rowsum(F_q)
  {
    const int row = tid >> 4, p = tid & 15;
    float fs[1];
    ft::row_sums(mp, p, fs, [&](int j, float (&u)[1]) { u[0] += s_f[row * LD + j]; });
    if (p == 0) s_fs[row] = fs[0];
  }
  // 5. the walk.  Carried, relative to Mprev = the running maximum at the end of the last chunk: P (this wave's NG tiles of the
  //    [16 x d] numerator, rows 4 lq + r, column 16 (wv + 4 i) + lr), p (rows 4 lq + r), vs (this lane's columns) and cnt
  const int len = task_len(a.lens, t, Nc);
  f32x4_t Pc[NG], pc = {0.f, 0.f, 0.f, 0.f};
  float vsc[NG], cntc = 0.f, Mprev = -INFINITY;
#pragma unroll
  for (int i = 0; i < NG; ++i) { Pc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f}; vsc[i] = 0.f; }
  int ki = 0;
  for (int sc = 0; sc < a.nsc; ++sc) {
    const int n0 = CH * sc, ll = min(max(len - n0, 0), CH);
    __syncthreads();                            // the last chunk's members have read s_S, s_mref (and, first, s_fs is written)
    {
      const int r = tid >> 3;
      const float dg = ft::key_diag(r < ll ? a.k + (((size_t)t * Nc + n0 + r) * H + h) * d : nullptr, d, a.sc.c, tid);
      if ((tid & 7) == 0) s_kd[r] = dg;
    }
    if (tid < CH) s_sm[tid] = a.ws.smax[n0 + tid];
    // the chunk's rows of v for this lane's columns: slot 4 s8 + lq, zeros behind lens[t] (never read)
    float bv[NG][CH / 4];
#pragma unroll
    for (int i = 0; i < NG; ++i)
#pragma unroll
      for (int s8 = 0; s8 < CH / 4; ++s8) {
        const int np = 4 * s8 + lq, e = 16 * (wv + 4 * i) + lr;
        bv[i][s8] = (e < d && np < ll) ? a.v[(((size_t)t * Nc + n0 + np) * H + h) * d + e] : 0.f;
      }
    __syncthreads();
    if (tid < CH) {
      float mm = Mprev;
      for (int i = 0; i <= tid; ++i) mm = fmaxf(mm, s_sm[i]);
      s_mref[tid] = mm;
    }
    __syncthreads();
    // S[q, n] = sum_j F_q[q, j] exp(dd[n, j] - diag[n] - Mref[n]); features >= m and shots behind lens[t] are zeros by index
    {
      const float* drow[2];
      float sub[2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int n = 16 * jj + lr;
        drow[jj] = n < ll ? a.ws.dd + ((size_t)th * a.ws.Ncp + n0 + n) * mp + 4 * lq : nullptr;
        sub[jj] = s_kd[n] + s_mref[n];
      }
      ft::s_tile(s_f, LD, drow, (ll + 15) / 16, ll > 0 ? mp / 16 : 0, CH,
                 [&](int jj, int j0, bool on, float4 b) { return on ? ft::exp4(b, sub[jj], j0, m) : make_float4(0.f, 0.f, 0.f, 0.f); }, red, s_S);
    }
    // the chunk's part of a prefix that ends p shots into it, relative to Mk: one chain over the shot slots per tile, one against
    // ones for the denominator; slots at or behind min(p, ll) are zeros by index, their MFMAs (which would add +0) are skipped
    auto product = [&](int p, float Mk, float eps, f32x4_t (&o)[NG], f32x4_t& od) {
      const int cut = min(p, ll);
      float av[CH / 4];
#pragma unroll
      for (int s8 = 0; s8 < CH / 4; ++s8) {
        const int np = 4 * s8 + lq;
        const float mr = s_mref[np];
        const float w = mr == Mk ? 1.f : expf(mr - Mk);
        av[s8] = np < cut ? s_S[lr * ft::LDS_S + np] * w + eps * s_fs[lr] : 0.f;
      }
      od = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NG; ++i) o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s8 = 0; s8 < CH / 4; ++s8)
        if (4 * s8 < cut) {
          od = mfma4(av[s8], 1.f, od);
#pragma unroll
          for (int i = 0; i < NG; ++i) o[i] = mfma4(av[s8], bv[i][s8], o[i]);
        }
    };
    float fsr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) fsr[r] = s_fs[4 * lq + r];
    for (; ki < a.K && a.ks[ki] <= n0 + CH; ++ki) {
      const int p = a.ks[ki] - n0;
      const float Mk = s_mref[p - 1];
      const float g = Mk == Mprev ? 1.f : expf(Mprev - Mk);          // <= 1; the first chunk carries zeros
      f32x4_t o[NG], od;
      product(p, Mk, EPS, o, od);
      float den[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) den[r] = (g * pc[r] + (EPS * cntc) * fsr[r]) + od[r];
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const int e = 16 * (wv + 4 * i) + lr;
        if (e >= d) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = q0 + 4 * lq + r;
          if (n < Nq) a.out[(((size_t)ki * a.T + t) * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = ((g * Pc[i][r] + (EPS * vsc[i]) * fsr[r]) + o[i][r]) / den[r];
        }
      }
    }
    const float Mend = s_mref[CH - 1];
    if (sc + 1 < a.nsc) {                       // the chunk joins the carried sums, relative to its last running maximum
      const float g = Mend == Mprev ? 1.f : expf(Mprev - Mend);
      f32x4_t o[NG], od;
      product(CH, Mend, 0.f, o, od);
#pragma unroll
      for (int r = 0; r < 4; ++r) pc[r] = g * pc[r] + od[r];
#pragma unroll
      for (int i = 0; i < NG; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Pc[i][r] = g * Pc[i][r] + o[i][r];
        f32x4_t ov = {0.f, 0.f, 0.f, 0.f};      // the column sums of the chunk's v: a chain against ones, every row the same
#pragma unroll
        for (int s8 = 0; s8 < CH / 4; ++s8)
          if (4 * s8 < ll) ov = mfma4(4 * s8 + lq < ll ? 1.f : 0.f, bv[i][s8], ov);
        vsc[i] += ov[0];
      }
      cntc += (float)ll;
    }
    Mprev = Mend;
  }
}

inline size_t ws_need(int T, int H, int Nc, int m) { return carve_ws(T, H, Nc, m, nullptr).floats * sizeof(float); }

}  // namespace fpl
#endif

inline size_t favor_prefix_long_ws_need(int T, int H, int Nq, int Nc, int d, int m, int K) {
#ifndef MLHOT_HOSTSIM
  if (favor_prefix_long_ok(T, H, Nq, Nc, d, m, K)) return fpl::ws_need(T, H, Nc, m);
#endif
  (void)T; (void)H; (void)Nq; (void)Nc; (void)d; (void)m; (void)K; return 0;
}

// ks[K]: HOST ints, strictly increasing, 1 <= ks[i] <= Nc; lens[T]: int32 on the DEVICE (read there) or NULL
inline int favor_prefix_long_forward(const float* q, const float* k, const float* v, const float* proj, const int32_t* ks, int K,
                                     const int32_t* lens, int T, int H, int Nq, int Nc, int d, int m, float* out, void* ws, size_t ws_bytes,
                                     hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || Nc <= 0 || d <= 0 || m <= 0 || K <= 0 || !q || !k || !v || !proj || !ks || !out) {
    set_error("favor_prefix_long_fwd: bad argument"); return MLHOT_ERR_ARG;
  }
  if (!favor_prefix_long_ok(T, H, Nq, Nc, d, m, K)) {
    set_error("favor_prefix_long_fwd serves d %% 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, 1 <= K <= 64 on the GPU build (got d=%d m=%d K=%d)", d, m, K);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  for (int i = 0; i < K; ++i)
    if (ks[i] < 1 || ks[i] > Nc || (i > 0 && ks[i] <= ks[i - 1])) {
      set_error("favor_prefix_long_fwd: ks must be strictly increasing context sizes in 1..%d (ks[%d] = %d)", Nc, i, (int)ks[i]); return MLHOT_ERR_ARG;
    }
  fpl::Args a{};
  a.ws = fpl::carve_ws(T, H, Nc, m, ws);
  if (!ws || ws_bytes < a.ws.floats * sizeof(float)) { set_error("favor_prefix_long_fwd: workspace too small (%zu < %zu)", ws_bytes, a.ws.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(q) || !ft::aligned16(k) || !ft::aligned16(v) || !ft::aligned16(proj) || !ft::aligned16(ws)) {
    set_error("favor_prefix_long_fwd: q, k, v, proj and ws must be 16-byte aligned"); return MLHOT_ERR_ARG;
  }
  a.q = q; a.k = k; a.v = v; a.proj = proj; a.lens = lens; a.out = out;
  a.T = T; a.H = H; a.Nq = Nq; a.Nc = Nc; a.d = d; a.m = m; a.mp = a.ws.mp; a.K = K;
  a.ntile = (Nq + ft::QT - 1) / ft::QT;
  a.nsc = (ks[K - 1] + fpl::CH - 1) / fpl::CH;
  a.sc = ft::Scales(d, m);
  for (int i = 0; i < K; ++i) a.ks[i] = ks[i];
  {
    ProfScope ps("favor.plong_dd", s);
    hipLaunchKernelGGL(fpl::dd_kernel, dim3((unsigned)(T * H * a.nsc), a.ws.nch), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor.plong_dd"));
  {
    ProfScope ps("favor.plong_max", s);
    hipLaunchKernelGGL(fpl::smax_kernel, dim3((fpl::CH * a.nsc + 255) / 256), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor.plong_max"));
  ProfScope ps("favor.plong_sweep", s);
  const dim3 grid((unsigned)(a.ntile * T * H));
  switch ((d + 63) / 64) {
    case 1: hipLaunchKernelGGL((fpl::sweep_kernel<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((fpl::sweep_kernel<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((fpl::sweep_kernel<3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((fpl::sweep_kernel<4>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch("favor.plong_sweep");
#endif
}

}  // namespace mlhot
