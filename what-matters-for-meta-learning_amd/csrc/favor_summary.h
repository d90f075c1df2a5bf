// FAVOR+ context as a fixed-size summary: absorb shots without a capacity, query against [m, d] numbers.
//
// FAVOR+ is a linear attention: the context enters out only through  sum_n F_k[n]^T v[n]  and  sum_n F_k[n].  With the key feature
// F_k[n, j] = ratio (exp(dd[n, j] - diag[n] - M) + eps) the ratio cancels between numerator and denominator and the eps floor
// separates, so per (task, head) the state is, relative to its stabiliser M (ONE per state: the maximum of dd over every valid shot
// of all tasks, heads and features absorbed so far - fast_attention.py:96-97's batch-global rule):
//   A[j, e] = sum_n exp(dd[n, j] - diag[n] - M) v[n, e]   [mp, d]      a[j] = sum_n exp(dd[n, j] - diag[n] - M)   [mp]
//   vs[e]   = sum_n v[n, e]                                [d]          cnt  = the number of shots
//   out[q, e] = sum_j F_q[q, j] (A[j, e] + eps vs[e]) / sum_j F_q[q, j] (a[j] + eps cnt),   F_q exactly fc::query_kernel's (ft::query_front).
// State (floats): A [T][H][mp][d], a [T][H][mp], vs [T][H][d], M (one float in a block of 16), cnt [T][H] (int32), mp = m rounded
// up to 16; features >= m are exact zeros.  A fresh state has M = -inf and everything else 0.
//
//   absorb A1 grid (task x head, 256-feature chunk): dd of the NEW shots (<= 32 per task) on the matrix core into the workspace -
//             ft::keys_dd, so an element has the bits favor_keys gives it - and the workgroup's maximum; one workgroup copies the
//             state's M into the workspace, so that no workgroup of A2 reads what another one writes (state_in may be state_out)
//          A2 grid (task x head, 64-feature chunk): M' = max(M, the maxima), s = exp(M - M') (1 where M' == M, so a fresh state's
//             -inf - -inf never forms), e[n, j] = exp(dd - diag - M') in LDS (0 behind lens[t] and at features >= m - selected by
//             index, never by a product), then A <- s A + e^T v on the matrix core (K = the 32 shot slots), a <- s a + the row sums of
//             e^T; chunk 0 of a (task, head) adds vs and cnt, chunk 0 of (0, 0) writes M'
//   retract R1 = A1 as it is, R2 grid as A2: M stays, e = exp(min(dd - M, 0) - diag), A <- A - e^T v, a <- max(a - rowsum e, 0), vs and
//             cnt go down (fsum::retract2_kernel below)
//   query  grid (task x head x 16-row query tile), ONE launch for any Nq: F_q in LDS (ft::query_front), then
//             [16 x mp] [mp x d] against A streamed from memory: wave w takes the 16-feature chunks w, w + 4, .. in ascending order
//             for all d columns, the four partial tiles fold 0, 1, 2, 3 through LDS (F_q's space, dead by then); the row sums of
//             F_q and of F_q a give the eps terms and the denominator.
//   merge  grid (512 float4 slots of the state), ONE launch: n <= 8 states absorbed apart -> one, X' = sum_i exp(M_i - M') X_i
//             (fsum::merge_kernel below)
//   gather grid (512 float4 slots of the OUTPUT state), ONE launch: task t of the output = the sum of up to 8 (state, task) parts named
//             by a table on the device - merge with a row per task (fsum::gather_kernel below)
// No atomics; every sum has one order that depends on the dimensions alone.  ROW INVARIANCE of the query launch as in
// favor_cached.h: a workgroup owns 16 rows and every feature of them, rows >= Nq are zeros and never stored, and every per-row sum
// is laid out the same way at every row of a tile.
#pragma once
#include "common.h"
#include "favor_cached.h"

namespace mlhot {

inline bool favor_summary_ok(int T, int H, int d, int m) {
#ifdef MLHOT_HOSTSIM
  (void)T; (void)H; (void)d; (void)m; return false;
#else
  return ft::envelope_ok(T, H, d, m);
#endif
}

#ifndef MLHOT_HOSTSIM
namespace fsum {

using ft::f32x4_t;
using ft::mfma4;
using ft::EPS;

constexpr int MAXN = 32;                  // new shots per task and absorb call
constexpr int FC = 64;                    // features per A2 workgroup: 16 per wave
constexpr int LDE = FC + 8;               // LDS row stride of e

struct State { float *A, *a, *vs, *M; int32_t* cnt; int mp; size_t floats; };
inline State carve_state(int T, int H, int d, int m, void* state) {
  State s{};
  s.mp = (m + 15) / 16 * 16;
  const size_t th = (size_t)T * H;
  s.A = (float*)state; s.a = s.A + th * s.mp * d; s.vs = s.a + th * s.mp; s.M = s.vs + th * d;
  s.cnt = (int32_t*)(s.M + 16);
  s.floats = th * s.mp * d + th * s.mp + th * d + 16 + align_up(th, 16);
  return s;
}

struct Ws { float *dd, *part, *Mold; int nch; size_t floats; };
inline Ws carve_ws(int T, int H, int n, int mp, void* ws) {
  Ws w{};
  const size_t th = (size_t)T * H;
  w.nch = (mp + ft::KCH - 1) / ft::KCH;
  w.dd = (float*)ws; w.part = w.dd + th * n * mp; w.Mold = w.part + align_up(th * w.nch, 64);
  w.floats = th * n * mp + align_up(th * w.nch, 64) + 64;
  return w;
}

struct AbsorbArgs {
  const float *k, *v, *proj;
  const int32_t* lens;
  State in, out;
  Ws ws;
  int T, H, n, d, m, mp;
  float c;
};

// lens[t] held to 0 .. n; NULL: every one of the n rows is a shot
__device__ __forceinline__ int new_len(const int32_t* lens, int t, int n) { return ft::clamp_len(lens, t, 0, n); }

__global__ __launch_bounds__(256) void init_kernel(float* st, size_t floats, size_t m_at) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < floats; i += (size_t)gridDim.x * 256) st[i] = i == m_at ? -INFINITY : 0.f;
}

// ---- absorb, launch 1: dd of the new shots into the workspace, the workgroup's maximum ---------------------------------------
template <int RT>
__global__ __launch_bounds__(256) void absorb1_kernel(const AbsorbArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[16 * RT * ft::LDX];
  __shared__ float s_w[4];
  const int th = blockIdx.x, t = th / a.H, h = th % a.H;
  if (th == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.ws.Mold[0] = a.in.M[0];
  ft::keys_dd<RT, false, true>([&](int r) { return a.k + ((size_t)(t * a.n + r) * a.H + h) * a.d; }, new_len(a.lens, t, a.n), a.proj, a.c, a.d, a.m, a.mp,
                         a.ws.dd + (size_t)th * a.n * a.mp, a.ws.part + (size_t)th * a.ws.nch + blockIdx.y, xs, s_w);
}

// ---- absorb, launch 2: M', the rescale, A += e^T v, a += rowsum(e^T); vs, cnt and M by designated workgroups ---------------------
__global__ __launch_bounds__(256) void absorb2_kernel(const AbsorbArgs a) {
  __shared__ float es[MAXN * LDE];
  __shared__ float s_w[4], s_diag[MAXN];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x, t = th / a.H, h = th % a.H, chunk = blockIdx.y;
  const int d = a.d, n = a.n, m = a.m, mp = a.mp, H = a.H;
  const int len = new_len(a.lens, t, n);
  ft::part_max(a.ws.part, a.T * H * a.ws.nch, s_w, tid);
  {
    const int r = tid >> 3;
    const float dg = ft::key_diag(r < len ? a.k + ((size_t)(t * n + r) * H + h) * d : nullptr, d, a.c, tid);
    if ((tid & 7) == 0) s_diag[r] = dg;
  }
  __syncthreads();
  const float Mold = a.ws.Mold[0];
  const float M = fmaxf(Mold, ft::max4(s_w[0], s_w[1], s_w[2], s_w[3]));
  const float scale = M == Mold ? 1.f : expf(Mold - M);         // a fresh state (Mold = -inf) with no valid shot keeps M = -inf
  const int j0 = chunk * FC;
  const float* ddb = a.ws.dd + (size_t)th * n * mp;
  for (int idx = tid; idx < MAXN * FC; idx += 256) {
    const int row = idx / FC, jj = idx - row * FC, j = j0 + jj;
    es[row * LDE + jj] = (row < len && j < m) ? expf(ddb[(size_t)row * mp + j] - (s_diag[row] + M)) : 0.f;
  }
  __syncthreads();
  const int jw = j0 + 16 * wv;
  if (jw < mp) {
    const int nks = (len + 3) / 4;                               // shot slots behind len are zeros: their MFMAs add +0 and are skipped
    float ea[MAXN / 4];
#pragma unroll
    for (int ks = 0; ks < MAXN / 4; ++ks) ea[ks] = es[(4 * ks + lq) * LDE + 16 * wv + lr];
    const float* Ain = a.in.A + ((size_t)th * mp + jw) * d;
    float* Aout = a.out.A + ((size_t)th * mp + jw) * d;
    for (int et = 0; 16 * et < d; ++et) {
      const int e = 16 * et + lr;
      float bv[MAXN / 4], old[4];
#pragma unroll
      for (int ks = 0; ks < MAXN / 4; ++ks) { const int np = 4 * ks + lq; bv[ks] = np < len ? a.v[((size_t)(t * n + np) * H + h) * d + e] : 0.f; }
#pragma unroll
      for (int r = 0; r < 4; ++r) old[r] = Ain[(size_t)(4 * lq + r) * d + e];
      f32x4_t o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < MAXN / 4; ++ks)
        if (ks < nks) o = mfma4(ea[ks], bv[ks], o);
#pragma unroll
      for (int r = 0; r < 4; ++r) Aout[(size_t)(4 * lq + r) * d + e] = scale * old[r] + o[r];
    }
  }
  if (tid < FC && j0 + tid < mp) {
    float s = 0.f;
    for (int row = 0; row < len; ++row) s += es[row * LDE + tid];
    a.out.a[(size_t)th * mp + j0 + tid] = scale * a.in.a[(size_t)th * mp + j0 + tid] + s;
  }
  if (chunk == 0) {
    if (tid < d) {
      float s = 0.f;
      for (int row = 0; row < len; ++row) s += a.v[((size_t)(t * n + row) * H + h) * d + tid];
      a.out.vs[(size_t)th * d + tid] = a.in.vs[(size_t)th * d + tid] + s;
    }
    if (tid == 0) a.out.cnt[th] = a.in.cnt[th] + len;
    if (th == 0 && tid == 0) a.out.M[0] = M;
  }
}

// ---- retract, launch 2: shots that were absorbed earlier are taken out again ------------------------------------
// absorb2_kernel's grid and layout with the sign turned: M stays the state's (no rescale; absorb1's maxima in the workspace are not
// read), e[n, j] = exp(min(dd - M, 0) - diag) - for a shot that WAS absorbed dd <= M holds and the min does nothing; for one that never
// was, it keeps e <= 1, so the result is undefined in value but finite - then A <- A - e^T v on the matrix core, a <- max(a - the row
// sums of e^T, 0), vs -= sum v, cnt -= len.  A kernel of its own: absorb2_kernel keeps its code, its bits and its resources.  In place
// (in == out) no workgroup writes M; out of place one workgroup copies M's block and cnt's padding, which nobody reads.
__global__ __launch_bounds__(256) void retract2_kernel(const AbsorbArgs a) {
  __shared__ float es[MAXN * LDE];
  __shared__ float s_diag[MAXN];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x, t = th / a.H, h = th % a.H, chunk = blockIdx.y;
  const int d = a.d, n = a.n, m = a.m, mp = a.mp, H = a.H;
  const int len = new_len(a.lens, t, n);
  {
    const int r = tid >> 3;
    const float dg = ft::key_diag(r < len ? a.k + ((size_t)(t * n + r) * H + h) * d : nullptr, d, a.c, tid);
    if ((tid & 7) == 0) s_diag[r] = dg;
  }
  __syncthreads();
  const float M = a.ws.Mold[0];
  const int j0 = chunk * FC;
  const float* ddb = a.ws.dd + (size_t)th * n * mp;
  for (int idx = tid; idx < MAXN * FC; idx += 256) {
    const int row = idx / FC, jj = idx - row * FC, j = j0 + jj;
    es[row * LDE + jj] = (row < len && j < m) ? expf(fminf(ddb[(size_t)row * mp + j] - M, 0.f) - s_diag[row]) : 0.f;
  }
  __syncthreads();
  const int jw = j0 + 16 * wv;
  if (jw < mp) {
    const int nks = (len + 3) / 4;
    float ea[MAXN / 4];
#pragma unroll
    for (int ks = 0; ks < MAXN / 4; ++ks) ea[ks] = es[(4 * ks + lq) * LDE + 16 * wv + lr];
    const float* Ain = a.in.A + ((size_t)th * mp + jw) * d;
    float* Aout = a.out.A + ((size_t)th * mp + jw) * d;
    for (int et = 0; 16 * et < d; ++et) {
      const int e = 16 * et + lr;
      float bv[MAXN / 4], old[4];
#pragma unroll
      for (int ks = 0; ks < MAXN / 4; ++ks) { const int np = 4 * ks + lq; bv[ks] = np < len ? a.v[((size_t)(t * n + np) * H + h) * d + e] : 0.f; }
#pragma unroll
      for (int r = 0; r < 4; ++r) old[r] = Ain[(size_t)(4 * lq + r) * d + e];
      f32x4_t o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < MAXN / 4; ++ks)
        if (ks < nks) o = mfma4(ea[ks], bv[ks], o);
#pragma unroll
      for (int r = 0; r < 4; ++r) Aout[(size_t)(4 * lq + r) * d + e] = old[r] - o[r];
    }
  }
  if (tid < FC && j0 + tid < mp) {
    float s = 0.f;
    for (int row = 0; row < len; ++row) s += es[row * LDE + tid];
    a.out.a[(size_t)th * mp + j0 + tid] = fmaxf(a.in.a[(size_t)th * mp + j0 + tid] - s, 0.f);
  }
  if (chunk == 0) {
    if (tid < d) {
      float s = 0.f;
      for (int row = 0; row < len; ++row) s += a.v[((size_t)(t * n + row) * H + h) * d + tid];
      a.out.vs[(size_t)th * d + tid] = a.in.vs[(size_t)th * d + tid] - s;
    }
    if (tid == 0) a.out.cnt[th] = a.in.cnt[th] - len;
    if (th == 0 && a.out.M != a.in.M) {                          // a buffer of its own: M's block, and cnt's padding as init leaves it
      if (tid < 16) a.out.M[tid] = tid == 0 ? M : 0.f;
      const int thn = a.T * H;
      if (tid >= 64 && tid < 80 && thn + tid - 64 < (thn + 15) / 16 * 16) a.out.cnt[thn + tid - 64] = 0;
    }
  }
}

// ---- query -------------------------------------------------------------------------------------------------------------------
struct QueryArgs {
  const float *q, *proj;
  State st;
  float* out;
  int T, H, Nq, d, m, mp, ntile;
  ft::Scales sc;
};

// NG: 64-column groups of d (ft::stream_product)
template <int NG>
__global__ __launch_bounds__(256) void query_kernel(const QueryArgs a) {
  __shared__ __attribute__((aligned(16))) float s_f[ft::QT * ft::ldf(ft::MAXM)];
  __shared__ __attribute__((aligned(16))) float xs[ft::QT * ft::LDX];
  __shared__ float s_diag[ft::QT], s_pm[4][ft::QT], s_fs[ft::QT], s_den[ft::QT];
  static_assert(4 * ft::QT * ft::ldo(ft::MAXD) <= ft::QT * ft::ldf(ft::MAXM), "the four partial tiles must fit into F_q's space");
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lq = lane >> 4;
  const int th = blockIdx.x / a.ntile, tile = blockIdx.x % a.ntile, t = th / a.H, h = th % a.H, n0 = tile * ft::QT;
  const int d = a.d, Nq = a.Nq, H = a.H, mp = a.mp, LD = ft::ldf(mp);
  // 1. - 3. c q and diag, dd and the row maxima, F_q in place
  ft::query_front([&](int r) { return n0 + r < Nq ? a.q + (((size_t)t * Nq + n0 + r) * H + h) * d : nullptr; }, a.proj, d, a.m, mp, a.sc, xs, s_f, s_diag, s_pm);
  // 4. per row: fs = sum_j F_q[j], fa = sum_j F_q[j] a[j]
  {
    const int row = tid >> 4, p = tid & 15;
    const float* av = a.st.a + (size_t)th * mp;
    float s[2];
    ft::row_sums(mp, p, s, [&](int j, float (&u)[2]) { const float f = s_f[row * LD + j]; u[0] += f; u[1] += f * av[j]; });
    if (p == 0) { s_fs[row] = s[0]; s_den[row] = s[1] + (EPS * (float)a.st.cnt[th]) * s[0]; }
  }
  // 5. F_q A into the four partial tiles
  ft::stream_product<NG>(s_f, LD, a.st.A + (size_t)th * mp * d, mp, d, wv, lr, lq);
  // 6. fold the waves 0, 1, 2, 3, add eps vs[e] fs, divide, store in mlhot_favor_fwd's merged order
  {
    const float* vs = a.st.vs + (size_t)th * d;
    for (int idx = tid; idx < ft::QT * d; idx += 256) {
      const int row = idx / d, e = idx - row * d, n = n0 + row;
      if (n >= Nq) continue;
      const float s = ft::fold_tiles(s_f, ft::ldo(d), row, e);
      a.out[((size_t)t * Nq + n) * ((size_t)d * H) + (size_t)e * H + h] = (s + (EPS * vs[e]) * s_fs[row]) / s_den[row];
    }
  }
}

// ---- merge: n states that were absorbed apart -> the state of all their shots ---------------------------------------
// The state is a sum over shots, so with M' = max_i M_i (and the caller's floor) it is  X' = sum_i exp(M_i - M') X_i  for A and a and
// the plain sums for vs and cnt.  ONE launch, a stream: every region of the layout starts at a multiple of 4 floats (mp and d are
// multiples of 16), so the whole state is one list of float4 slots and a lane owns MERGE_U of them, one grid stride apart; region, task,
// head and feature row come from the flat slot index (pool_ingest.h's pool1_gather_kernel).  A lane issues its MERGE_U * N loads,
// then folds the states 0, 1, .. N - 1 in ONE chain per element: no atomics, no split, the order a function of N alone.  Every
// workgroup reads the N old stabilisers itself - out is none of the inputs (the entry refuses it), so nobody reads what another
// workgroup writes.  s_i is exactly 1 where M_i == M' (so -inf - -inf never forms), features >= m are written as zeros by index.
constexpr int MERGE_MAX = 8;              // states per launch
constexpr int MERGE_U = 2;                // float4 slots per lane

struct MergeArgs {
  const float* in[MERGE_MAX];
  const float* floor;                     // one float on the device, or nullptr
  float* out;
  long a_at, vs_at, m_at, cnt_at, n4;     // in float4 slots: where a, vs, M's block and cnt begin, and the whole state
  int d4, mp, m, th;                      // d4: slots per row of A
};

// term p of an element's chain  s0 x0 + s1 x1 + s2 x2 + ..,  written with the roundings spelled out - they are the ones the
// compiler's contraction of that sum has given merge_kernel since 6c-6 (of the first two products the SECOND is rounded and the first
// fused onto it), so merge's bits stay where they were whatever a later compiler prefers:
//   p == 0: o = rn(s0 x0)      p == 1: o = fma(s0, x0, rn(s1 x1))      p >= 2: o = fma(sp, xp, o)
// merge_kernel and gather_kernel both fold through this step, so the same terms in the same order give the same bits in either.
__device__ __forceinline__ void fold_step(float4& o, int p, float s0, const float4& x0, float sp, const float4& xp) {
#pragma clang fp contract(off)
  if (p == 0) { o.x = s0 * x0.x; o.y = s0 * x0.y; o.z = s0 * x0.z; o.w = s0 * x0.w; }
  else if (p == 1) { o.x = fmaf(s0, x0.x, sp * xp.x); o.y = fmaf(s0, x0.y, sp * xp.y); o.z = fmaf(s0, x0.z, sp * xp.z); o.w = fmaf(s0, x0.w, sp * xp.w); }
  else { o.x = fmaf(sp, xp.x, o.x); o.y = fmaf(sp, xp.y, o.y); o.z = fmaf(sp, xp.z, o.z); o.w = fmaf(sp, xp.w, o.w); }
}
// features >= m of a slot of A (one feature row `row`) or of a (the four features j .. j + 3) are zeros by index
__device__ __forceinline__ void zero_row_behind_m(float4& o, int row, int m) { if (row >= m) o = float4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ void zero_features_behind_m(float4& o, int j, int m) {
  if (j >= m) o.x = 0.f;
  if (j + 1 >= m) o.y = 0.f;
  if (j + 2 >= m) o.z = 0.f;
  if (j + 3 >= m) o.w = 0.f;
}

template <int N>
__global__ __launch_bounds__(256) void merge_kernel(const MergeArgs a) {
  float s[N];
  float M = a.floor ? a.floor[0] : -INFINITY;
#pragma unroll
  for (int i = 0; i < N; ++i) { s[i] = a.in[i][4 * a.m_at]; M = fmaxf(M, s[i]); }
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = s[i] == M ? 1.f : expf(s[i] - M);
  const long stride = (long)gridDim.x * 256;
  const long q0 = (long)blockIdx.x * 256 + threadIdx.x;
  float4 x[MERGE_U][N];
#pragma unroll
  for (int u = 0; u < MERGE_U; ++u) {
    const long q = q0 + u * stride;
#pragma unroll
    for (int i = 0; i < N; ++i) x[u][i] = q < a.n4 ? reinterpret_cast<const float4*>(a.in[i])[q] : float4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int u = 0; u < MERGE_U; ++u) {
    const long q = q0 + u * stride;
    if (q >= a.n4) continue;
    float4 o;
    if (q < a.m_at) {                      // A, a (rescaled) and vs (plain): one chain, the states in order
      const bool plain = q >= a.vs_at;
      o = float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < N; ++i) fold_step(o, i, plain ? 1.f : s[0], x[u][0], plain ? 1.f : s[i], x[u][i]);
      if (q < a.a_at) {                    // a slot of A lies in one feature row: (task x head, row) = slot / d4
        zero_row_behind_m(o, (int)((q / a.d4) % a.mp), a.m);
      } else if (!plain) {                 // four features of a, never across a (task, head): mp % 4 == 0
        zero_features_behind_m(o, (int)((4 * (q - a.a_at)) % a.mp), a.m);
      }
    } else if (q < a.cnt_at) {             // M's block of 16: M', then zeros as init leaves them
      o = float4{q == a.m_at ? M : 0.f, 0.f, 0.f, 0.f};
    } else {                               // cnt: int32 sums; the padding behind T H stays 0
      const long e = 4 * (q - a.cnt_at);
      int c[4] = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < N; ++i) {
        c[0] += __float_as_int(x[u][i].x); c[1] += __float_as_int(x[u][i].y); c[2] += __float_as_int(x[u][i].z); c[3] += __float_as_int(x[u][i].w);
      }
      o = float4{__int_as_float(e < a.th ? c[0] : 0), __int_as_float(e + 1 < a.th ? c[1] : 0), __int_as_float(e + 2 < a.th ? c[2] : 0),
                 __int_as_float(e + 3 < a.th ? c[3] : 0)};
    }
    reinterpret_cast<float4*>(a.out)[q] = o;
  }
}

// ---- gather: task t of the output = the sum of up to 8 (state, task) parts, named by a table on the device ---------
// merge with a row per task.  The stream runs over the float4 slots of the OUTPUT state; region, (task, head) and the offset inside the
// task come from the flat slot index as in merge_kernel.  Inside a region a task's rows lie at the same offsets in every state - only the
// region's start depends on the state's own task count T_i - so part (i, u) of a slot is read at  T_i x (the floats per task of the regions
// in front) + u x (the region's floats per task) + (the offset inside the task).  A lane owns MERGE_U slots one grid stride apart (they
// may belong to different tasks); it reads their table rows, issues the MERGE_U * P loads, then folds every slot's parts in table order
// through merge's fold_step in ONE chain.  M' is the maximum over all n states passed (and the floor), whether a part names them or not;
// the n pointers, task counts and scales stand in LDS for the per-lane lookup - every workgroup fills its own copy from the kernel
// arguments, nothing is exchanged between workgroups.  No atomics, no scratch.  Whatever the table holds, the state index is held to
// 0 .. n - 1 and the task index to 0 .. T_i - 1 (ft::clamp_len's rule: the host checks the values, the clamp keeps every read in bounds).
constexpr int GATHER_P = 8;               // parts per task and launch

struct GatherArgs {
  const float* in[MERGE_MAX];
  int Ti[MERGE_MAX];                      // tasks of each source state
  const int32_t* parts;                   // [T_out][P][2] on the device: (state, task); state < 0 ends a task's list
  const float* floor;                     // one float on the device, or nullptr
  float* out;
  long a_at, vs_at, m_at, cnt_at, n4;     // of the OUTPUT, in float4 slots (MergeArgs)
  long fA, fa, fv;                        // floats per task of A, a and vs
  int d4, d, mp, m, th, H, n;             // th: T_out H
};

// part p of a task's table row -> (live, state, task), the indices held to their ranges; `on` stays false behind the first state < 0
__device__ __forceinline__ void gather_part(const int32_t* row, int p, int n, const int* s_T, bool& on, int& i, int& u) {
  const int2 e = reinterpret_cast<const int2*>(row)[p];
  on = on && e.x >= 0;
  i = on ? min(e.x, n - 1) : 0;
  u = min(max(e.y, 0), s_T[i] - 1);
}

template <int P>
__global__ __launch_bounds__(256) void gather_kernel(const GatherArgs a) {
  __shared__ const float* s_in[MERGE_MAX];
  __shared__ float s_s[MERGE_MAX];
  __shared__ int s_T[MERGE_MAX];
  const long fT = a.fA + a.fa + a.fv;     // floats per task in front of M's block
  float M = a.floor ? a.floor[0] : -INFINITY;
  {
    float Mi[MERGE_MAX];
#pragma unroll
    for (int i = 0; i < MERGE_MAX; ++i) { Mi[i] = i < a.n ? a.in[i][(long)a.Ti[i] * fT] : -INFINITY; M = fmaxf(M, Mi[i]); }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < MERGE_MAX; ++i) {                  // slots >= n are never looked up: the state index is held below n
        s_in[i] = a.in[i < a.n ? i : 0]; s_T[i] = a.Ti[i < a.n ? i : 0];
        s_s[i] = Mi[i] == M ? 1.f : expf(Mi[i] - M);
      }
    }
  }
  __syncthreads();
  const long stride = (long)gridDim.x * 256;
  const long q0 = (long)blockIdx.x * 256 + threadIdx.x;
  float4 x[MERGE_U][P];
  float sc[MERGE_U][P];
  bool live[MERGE_U][P];
  int row_or_j[MERGE_U];                  // the feature row of a slot of A, the first of the four features of a slot of a
#pragma unroll
  for (int u = 0; u < MERGE_U; ++u) {
    const long q = q0 + u * stride;
    long w = 0, per = 0, pre = 0;         // the offset inside the task, the region's floats per task, the floats per task in front of it
    int th = 0;
    const bool sums = q < a.m_at;
    const bool plain = q >= a.vs_at;
    row_or_j[u] = 0;
    if (q < a.a_at) {                      // A: slot / d4 is the feature row of all (task, head) rows, below 2^31 inside the envelope
      const long R = q / a.d4;
      const unsigned r = (unsigned)R;
      th = (int)(r / (unsigned)a.mp);
      row_or_j[u] = (int)(r - (unsigned)th * (unsigned)a.mp);
      w = ((long)(th % a.H) * a.mp + row_or_j[u]) * a.d + 4 * (q - R * a.d4); per = a.fA;
    } else if (!plain) {                   // a: four features of one (task, head)
      const unsigned e = (unsigned)(4 * (q - a.a_at));
      th = (int)(e / (unsigned)a.mp);
      row_or_j[u] = (int)(e - (unsigned)th * (unsigned)a.mp);
      w = (long)(th % a.H) * a.mp + row_or_j[u]; per = a.fa; pre = a.fA;
    } else if (sums) {                     // vs: four columns of one (task, head)
      const unsigned e = (unsigned)(4 * (q - a.vs_at));
      th = (int)(e / (unsigned)a.d);
      w = (long)(th % a.H) * a.d + (e - (unsigned)th * (unsigned)a.d); per = a.fv; pre = a.fA + a.fa;
    }
    const int32_t* row = a.parts + (long)(th / a.H) * (2 * P);
    bool on = sums;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      int i = 0, t = 0;
      if (sums) gather_part(row, p, a.n, s_T, on, i, t);
      live[u][p] = on;
      sc[u][p] = plain ? 1.f : s_s[i];
      // the pointer comes out of LDS: gfptr says it is global memory (global_load, not flat_load)
      typedef const __attribute__((address_space(1))) f32x4_t* g4ptr;
      f32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (on) v = *(g4ptr)((gfptr)s_in[i] + ((long)s_T[i] * pre + (long)t * per + w));
      x[u][p] = float4{v[0], v[1], v[2], v[3]};
    }
  }
#pragma unroll
  for (int u = 0; u < MERGE_U; ++u) {
    const long q = q0 + u * stride;
    if (q >= a.n4) continue;
    float4 o = float4{0.f, 0.f, 0.f, 0.f};     // a task without a part: the rows of a fresh state
    if (q < a.m_at) {                      // A, a (rescaled) and vs (plain): one chain, the parts in table order
#pragma unroll
      for (int p = 0; p < P; ++p)
        if (live[u][p]) fold_step(o, p, sc[u][0], x[u][0], sc[u][p], x[u][p]);
      if (q < a.a_at) zero_row_behind_m(o, row_or_j[u], a.m);
      else if (q < a.vs_at) zero_features_behind_m(o, row_or_j[u], a.m);
    } else if (q < a.cnt_at) {             // M's block of 16: M', then zeros as init leaves them
      o.x = q == a.m_at ? M : 0.f;
    } else {                               // cnt: int32 sums per (task, head); the padding behind T_out H stays 0
      const long e = 4 * (q - a.cnt_at);
      int c[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (e + k >= a.th) continue;
        const int th = (int)(e + k);
        const int32_t* row = a.parts + (long)(th / a.H) * (2 * P);
        bool on = true;
        for (int p = 0; p < P; ++p) {
          int i, t;
          gather_part(row, p, a.n, s_T, on, i, t);
          if (on) c[k] += __float_as_int(((gfptr)s_in[i])[(long)s_T[i] * fT + 16 + (long)t * a.H + th % a.H]);
        }
      }
      o = float4{__int_as_float(c[0]), __int_as_float(c[1]), __int_as_float(c[2]), __int_as_float(c[3])};
    }
    reinterpret_cast<float4*>(a.out)[q] = o;
  }
}

}  // namespace fsum
#endif

inline size_t favor_summary_need(int T, int H, int d, int m) {
#ifndef MLHOT_HOSTSIM
  if (favor_summary_ok(T, H, d, m)) return fsum::carve_state(T, H, d, m, nullptr).floats * sizeof(float);
#endif
  (void)T; (void)H; (void)d; (void)m; return 0;
}
inline size_t favor_summary_ws_need(int T, int H, int n, int d, int m) {
#ifndef MLHOT_HOSTSIM
  if (favor_summary_ok(T, H, d, m) && n >= 1 && n <= 32) return fsum::carve_ws(T, H, n, (m + 15) / 16 * 16, nullptr).floats * sizeof(float);
#endif
  (void)T; (void)H; (void)n; (void)d; (void)m; return 0;
}
inline size_t favor_summary_query_ws_need(int T, int H, int Nq, int d, int m) {      // the query kernel works in LDS alone
  return Nq >= 1 && favor_summary_ok(T, H, d, m) ? 256 : 0;
}

inline int favor_summary_unsupported(const char* what, int d, int m) {
  set_error("%s serves d %% 16 == 0, 16 <= d <= 256, 16 <= m <= 1536 on the GPU build (got d=%d m=%d)", what, d, m);
  return MLHOT_ERR_UNSUPPORTED;
}

inline int favor_summary_init(int T, int H, int d, int m, void* state, size_t state_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || d <= 0 || m <= 0 || !state) { set_error("favor_summary_init: bad argument"); return MLHOT_ERR_ARG; }
  if (!favor_summary_ok(T, H, d, m)) return favor_summary_unsupported("favor_summary_init", d, m);
#ifdef MLHOT_HOSTSIM
  (void)state_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  const fsum::State st = fsum::carve_state(T, H, d, m, state);
  if (state_bytes < st.floats * sizeof(float)) { set_error("favor_summary_init: state too small (%zu < %zu)", state_bytes, st.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(state)) { set_error("favor_summary_init: state must be 16-byte aligned"); return MLHOT_ERR_ARG; }
  ProfScope ps("favor.sum_init", s);
  const size_t want = (st.floats + 255) / 256;
  const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(fsum::init_kernel, dim3(blocks), dim3(256), 0, s, st.A, st.floats, (size_t)(st.M - st.A));
  return check_launch("favor.sum_init");
#endif
}

inline int favor_summary_absorb(const float* k, const float* v, const float* proj, const int32_t* lens, int T, int H, int n, int d, int m,
                                const void* state_in, void* state_out, size_t state_bytes, void* ws, size_t ws_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || n <= 0 || d <= 0 || m <= 0 || !k || !v || !proj || !state_in || !state_out) { set_error("favor_summary_absorb: bad argument"); return MLHOT_ERR_ARG; }
  if (!favor_summary_ok(T, H, d, m)) return favor_summary_unsupported("favor_summary_absorb", d, m);
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)state_bytes; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (n > fsum::MAXN) { set_error("favor_summary_absorb takes at most 32 new shots per task and call (got n=%d): absorb in chunks", n); return MLHOT_ERR_UNSUPPORTED; }
  fsum::AbsorbArgs a{};
  a.in = fsum::carve_state(T, H, d, m, const_cast<void*>(state_in));
  a.out = fsum::carve_state(T, H, d, m, state_out);
  a.ws = fsum::carve_ws(T, H, n, a.in.mp, ws);
  if (state_bytes < a.in.floats * sizeof(float)) { set_error("favor_summary_absorb: state too small (%zu < %zu)", state_bytes, a.in.floats * sizeof(float)); return MLHOT_ERR_WORKSPACE; }
  if (!ws || ws_bytes < a.ws.floats * sizeof(float)) { set_error("favor_summary_absorb: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(k) || !ft::aligned16(v) || !ft::aligned16(proj) || !ft::aligned16(state_in) || !ft::aligned16(state_out) || !ft::aligned16(ws)) {
    set_error("favor_summary_absorb: k, v, proj, the states and ws must be 16-byte aligned"); return MLHOT_ERR_ARG;
  }
  a.k = k; a.v = v; a.proj = proj; a.lens = lens;
  a.T = T; a.H = H; a.n = n; a.d = d; a.m = m; a.mp = a.in.mp;
  a.c = ft::Scales(d, m).c;
  {
    ProfScope ps("favor.sum_absorb1", s);
    if (n <= 16) hipLaunchKernelGGL((fsum::absorb1_kernel<1>), dim3(T * H, a.ws.nch), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((fsum::absorb1_kernel<2>), dim3(T * H, a.ws.nch), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor.sum_absorb1"));
  {
    ProfScope ps("favor.sum_absorb2", s);
    hipLaunchKernelGGL(fsum::absorb2_kernel, dim3(T * H, (a.mp + fsum::FC - 1) / fsum::FC), dim3(256), 0, s, a);
  }
  return check_launch("favor.sum_absorb2");
#endif
}

// the shots k, v - absorbed into state_in earlier - taken out again: absorb's argument list, absorb's first launch, fsum::retract2_kernel
inline int favor_summary_retract(const float* k, const float* v, const float* proj, const int32_t* lens, int T, int H, int n, int d, int m,
                                 const void* state_in, void* state_out, size_t state_bytes, void* ws, size_t ws_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || n <= 0 || d <= 0 || m <= 0 || !k || !v || !proj || !state_in || !state_out) { set_error("favor_summary_retract: bad argument"); return MLHOT_ERR_ARG; }
  if (!favor_summary_ok(T, H, d, m)) return favor_summary_unsupported("favor_summary_retract", d, m);
#ifdef MLHOT_HOSTSIM
  (void)lens; (void)state_bytes; (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (n > fsum::MAXN) { set_error("favor_summary_retract takes at most 32 shots per task and call (got n=%d): retract in chunks", n); return MLHOT_ERR_UNSUPPORTED; }
  fsum::AbsorbArgs a{};
  a.in = fsum::carve_state(T, H, d, m, const_cast<void*>(state_in));
  a.out = fsum::carve_state(T, H, d, m, state_out);
  a.ws = fsum::carve_ws(T, H, n, a.in.mp, ws);
  const size_t need = a.in.floats * sizeof(float);
  if (state_bytes < need) { set_error("favor_summary_retract: state too small (%zu < %zu)", state_bytes, need); return MLHOT_ERR_WORKSPACE; }
  if (!ws || ws_bytes < a.ws.floats * sizeof(float)) { set_error("favor_summary_retract: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(k) || !ft::aligned16(v) || !ft::aligned16(proj) || !ft::aligned16(state_in) || !ft::aligned16(state_out) || !ft::aligned16(ws)) {
    set_error("favor_summary_retract: k, v, proj, the states and ws must be 16-byte aligned"); return MLHOT_ERR_ARG;
  }
  {
    const char* ib = (const char*)state_in;
    const char* ob = (const char*)state_out;
    if (ib != ob && ib < ob + need && ob < ib + need) {           // the same buffer (in place) or two apart, nothing in between
      set_error("favor_summary_retract: state_out overlaps state_in without being it"); return MLHOT_ERR_ARG;
    }
  }
  a.k = k; a.v = v; a.proj = proj; a.lens = lens;
  a.T = T; a.H = H; a.n = n; a.d = d; a.m = m; a.mp = a.in.mp;
  a.c = ft::Scales(d, m).c;
  {
    ProfScope ps("favor.sum_retract1", s);
    if (n <= 16) hipLaunchKernelGGL((fsum::absorb1_kernel<1>), dim3(T * H, a.ws.nch), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((fsum::absorb1_kernel<2>), dim3(T * H, a.ws.nch), dim3(256), 0, s, a);
  }
  MLHOT_TRY(check_launch("favor.sum_retract1"));
  {
    ProfScope ps("favor.sum_retract2", s);
    hipLaunchKernelGGL(fsum::retract2_kernel, dim3(T * H, (a.mp + fsum::FC - 1) / fsum::FC), dim3(256), 0, s, a);
  }
  return check_launch("favor.sum_retract2");
#endif
}

// states: n device pointers in HOST memory; m_floor: one float in DEVICE memory or NULL ("the stabiliser is at least this")
inline int favor_summary_merge(const void* const* states, int n, const float* m_floor, int T, int H, int d, int m, void* out, size_t state_bytes,
                               hipStream_t s) {
  if (T <= 0 || H <= 0 || d <= 0 || m <= 0 || n < 0 || !states || !out) { set_error("favor_summary_merge: bad argument"); return MLHOT_ERR_ARG; }
  if (!favor_summary_ok(T, H, d, m)) return favor_summary_unsupported("favor_summary_merge", d, m);
#ifdef MLHOT_HOSTSIM
  (void)m_floor; (void)state_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (n < 1 || n > fsum::MERGE_MAX) { set_error("favor_summary_merge takes 1 .. 8 states per call (got n=%d): fold more in groups", n); return MLHOT_ERR_UNSUPPORTED; }
  const fsum::State st = fsum::carve_state(T, H, d, m, out);
  const size_t need = st.floats * sizeof(float);
  if (state_bytes != need) { set_error("favor_summary_merge: state_bytes must be mlhot_favor_summary_bytes' %zu (got %zu)", need, state_bytes); return MLHOT_ERR_WORKSPACE; }
  if (!ft::aligned16(out) || (m_floor && (reinterpret_cast<uintptr_t>(m_floor) & 3))) { set_error("favor_summary_merge: out must be 16-byte aligned, m_floor 4-byte"); return MLHOT_ERR_ARG; }
  fsum::MergeArgs a{};
  const char* ob = (const char*)out;
  for (int i = 0; i < n; ++i) {
    const char* ib = (const char*)states[i];
    if (!ib || !ft::aligned16(ib)) { set_error("favor_summary_merge: state %d is NULL or not 16-byte aligned", i); return MLHOT_ERR_ARG; }
    if (ib < ob + need && ob < ib + need) {       // every workgroup reads every old M and one writes the new one: out is a buffer of its own
      set_error("favor_summary_merge: out overlaps input state %d; the merged state needs its own buffer", i); return MLHOT_ERR_ARG;
    }
    a.in[i] = (const float*)states[i];
  }
  a.floor = m_floor; a.out = (float*)out;
  a.a_at = (long)((st.a - st.A) / 4); a.vs_at = (long)((st.vs - st.A) / 4); a.m_at = (long)((st.M - st.A) / 4); a.cnt_at = a.m_at + 4;
  a.n4 = (long)(st.floats / 4);
  a.d4 = d / 4; a.mp = st.mp; a.m = m; a.th = T * H;
  if ((a.n4 + 256 * fsum::MERGE_U - 1) / (256 * fsum::MERGE_U) >= (1l << 31)) { set_error("favor_summary_merge: the state is too large for one grid"); return MLHOT_ERR_ARG; }
  ProfScope ps("favor.sum_merge", s);
  const dim3 grid((unsigned)((a.n4 + 256 * fsum::MERGE_U - 1) / (256 * fsum::MERGE_U)));
  switch (n) {
    case 1: hipLaunchKernelGGL((fsum::merge_kernel<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((fsum::merge_kernel<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((fsum::merge_kernel<3>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((fsum::merge_kernel<4>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((fsum::merge_kernel<5>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((fsum::merge_kernel<6>), grid, dim3(256), 0, s, a); break;
    case 7: hipLaunchKernelGGL((fsum::merge_kernel<7>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((fsum::merge_kernel<8>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch("favor.sum_merge");
#endif
}

// states: n device pointers, tasks: their n task counts, both in HOST memory; parts: int32 [T_out][P][2] in DEVICE memory, read by the
// kernel alone (no host synchronisation: the call can be captured); m_floor as in merge
inline int favor_summary_gather(const void* const* states, const int* tasks, int n, const int32_t* parts, int P, const float* m_floor, int T_out, int H,
                                int d, int m, void* out, size_t state_bytes, hipStream_t s) {
  if (T_out <= 0 || H <= 0 || d <= 0 || m <= 0 || !states || !tasks || !parts || !out) { set_error("favor_summary_gather: bad argument"); return MLHOT_ERR_ARG; }
  if (n < 1 || n > 8) { set_error("favor_summary_gather takes 1 .. 8 states per call (got n=%d): fold more in groups", n); return MLHOT_ERR_ARG; }
  if (P < 1 || P > 8) { set_error("favor_summary_gather takes 1 .. 8 parts per task and call (got P=%d)", P); return MLHOT_ERR_ARG; }
  for (int i = 0; i < n; ++i)
    if (tasks[i] <= 0) { set_error("favor_summary_gather: state %d has %d tasks", i, tasks[i]); return MLHOT_ERR_ARG; }
  for (int i = -1; i < n; ++i)
    if (!favor_summary_ok(i < 0 ? T_out : tasks[i], H, d, m)) return favor_summary_unsupported("favor_summary_gather", d, m);
#ifdef MLHOT_HOSTSIM
  (void)m_floor; (void)state_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  static_assert(fsum::GATHER_P == 8 && fsum::MERGE_MAX == 8, "the entry's checks and the launch table below are written for 8");
  const fsum::State st = fsum::carve_state(T_out, H, d, m, out);
  const size_t need = st.floats * sizeof(float);
  if (state_bytes != need) { set_error("favor_summary_gather: state_bytes must be mlhot_favor_summary_bytes' %zu for T_out=%d (got %zu)", need, T_out, state_bytes); return MLHOT_ERR_ARG; }
  if (!ft::aligned16(out) || (m_floor && (reinterpret_cast<uintptr_t>(m_floor) & 3)) || (reinterpret_cast<uintptr_t>(parts) & 7)) {
    set_error("favor_summary_gather: out must be 16-byte aligned, parts 8-byte, m_floor 4-byte"); return MLHOT_ERR_ARG;
  }
  fsum::GatherArgs a{};
  const char* ob = (const char*)out;
  for (int i = 0; i < n; ++i) {
    const char* ib = (const char*)states[i];
    if (!ib || !ft::aligned16(ib)) { set_error("favor_summary_gather: state %d is NULL or not 16-byte aligned", i); return MLHOT_ERR_ARG; }
    const size_t have = fsum::carve_state(tasks[i], H, d, m, nullptr).floats * sizeof(float);
    if (ib < ob + need && ob < ib + have) {       // every workgroup reads every old M and one writes the new one: out is a buffer of its own
      set_error("favor_summary_gather: out overlaps input state %d; the gathered state needs its own buffer", i); return MLHOT_ERR_ARG;
    }
    a.in[i] = (const float*)states[i]; a.Ti[i] = tasks[i];
  }
  a.parts = parts; a.floor = m_floor; a.out = (float*)out;
  a.a_at = (long)((st.a - st.A) / 4); a.vs_at = (long)((st.vs - st.A) / 4); a.m_at = (long)((st.M - st.A) / 4); a.cnt_at = a.m_at + 4;
  a.n4 = (long)(st.floats / 4);
  a.fA = (long)H * st.mp * d; a.fa = (long)H * st.mp; a.fv = (long)H * d;
  a.d4 = d / 4; a.d = d; a.mp = st.mp; a.m = m; a.th = T_out * H; a.H = H; a.n = n;
  if ((a.n4 + 256 * fsum::MERGE_U - 1) / (256 * fsum::MERGE_U) >= (1l << 31)) { set_error("favor_summary_gather: the state is too large for one grid"); return MLHOT_ERR_ARG; }
  ProfScope ps("favor.sum_gather", s);
  const dim3 grid((unsigned)((a.n4 + 256 * fsum::MERGE_U - 1) / (256 * fsum::MERGE_U)));
  switch (P) {
    case 1: hipLaunchKernelGGL((fsum::gather_kernel<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((fsum::gather_kernel<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((fsum::gather_kernel<3>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((fsum::gather_kernel<4>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((fsum::gather_kernel<5>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((fsum::gather_kernel<6>), grid, dim3(256), 0, s, a); break;
    case 7: hipLaunchKernelGGL((fsum::gather_kernel<7>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((fsum::gather_kernel<8>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch("favor.sum_gather");
#endif
}

inline int favor_summary_query_forward(const float* q, const void* state, const float* proj, int T, int H, int Nq, int d, int m, float* out,
                                       void* ws, size_t ws_bytes, hipStream_t s) {
  if (T <= 0 || H <= 0 || Nq <= 0 || d <= 0 || m <= 0 || !q || !state || !proj || !out) { set_error("favor_summary_query_fwd: bad argument"); return MLHOT_ERR_ARG; }
  if (!favor_summary_ok(T, H, d, m)) return favor_summary_unsupported("favor_summary_query_fwd", d, m);
#ifdef MLHOT_HOSTSIM
  (void)ws; (void)ws_bytes; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  if (ws == nullptr || ws_bytes < favor_summary_query_ws_need(T, H, Nq, d, m)) { set_error("favor_summary_query_fwd: workspace too small"); return MLHOT_ERR_WORKSPACE; }
  const long long ntile = ((long long)Nq + ft::QT - 1) / ft::QT;
  if (ntile * T * H >= (1ll << 31)) { set_error("favor_summary_query_fwd: T H ceil(Nq / 16) must stay below 2^31 (chunk the query rows)"); return MLHOT_ERR_ARG; }
  if (!ft::aligned16(q) || !ft::aligned16(proj) || !ft::aligned16(state)) { set_error("favor_summary_query_fwd: q, proj and state must be 16-byte aligned"); return MLHOT_ERR_ARG; }
  fsum::QueryArgs a{};
  a.st = fsum::carve_state(T, H, d, m, const_cast<void*>(state));
  a.q = q; a.proj = proj; a.out = out;
  a.T = T; a.H = H; a.Nq = Nq; a.d = d; a.m = m; a.mp = a.st.mp; a.ntile = (int)ntile;
  a.sc = ft::Scales(d, m);
  ProfScope ps("favor.sum_query", s);
  const dim3 grid((unsigned)(ntile * T * H));
  switch ((d + 63) / 64) {
    case 1: hipLaunchKernelGGL((fsum::query_kernel<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((fsum::query_kernel<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((fsum::query_kernel<3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((fsum::query_kernel<4>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch("favor.sum_query");
#endif
}

}  // namespace mlhot
