// The query tail of the vanilla ANP models in ONE launch against a FAVOR+ SUMMARY state: np_query.h's launch for a
// context of any number of shots.
//
//   x [T*Nq, dw] (the encoder's target rows) and the summary state of favor_summary.h for (T, 8 heads, dw, m) - A [T][8][mp][d],
//   a [T][8][mp], vs [T][8][d], cnt [T][8], as absorb, merge and gather leave it:
//     per head h: q_h = x Wq_h^T + b, dd_q = (c q_h) P^T, row maxima, F_q                    (nq::query_kernel's steps 1 - 3)
//                 fs = sum_j F_q[j], fa = sum_j F_q[j] a[j]                                    (ft::row_sums)
//                 F_q A[t, h] with A streamed from memory                                      (ft::stream_product, ft::fold_tiles)
//                 out_h = (F_q A + eps vs fs) / (fa + eps cnt fs) into the merged tile (order e * 8 + h)
//     then r = merged Wo^T + b, z = r_to_z(r), mu = decoder0([x | z])                         (nq::query_kernel's tail)
// The kernel is nq::query_kernel<true, true> (np_query.h): the SUMMARY mode swaps steps 4 and 5 of a head, every other line is the
// per-shot launch's own.  This header holds the envelope and the entry.
// The stabiliser sits in the state and a (task, head) is one [mp x d] matrix and three vectors, so no workgroup depends on another:
// grid (task x 16-row target tile), 256 threads, no workspace, no atomics - whatever number of shots the state has absorbed.
//
// ROW INVARIANCE as in np_query.h: a workgroup owns 16 rows and everything of them, rows >= Nq are read as zeros and never stored, no
// sum mixes rows, and every sum has one order that is a function of the dimensions alone - the Linears' chains over k = 0, 16, ..;
// the row sums 16 lanes x (j = p, p + 16, ..) and a butterfly; F_q A by wave w over the 16-feature chunks w, w + 4, .., the four
// partial tiles folded 0, 1, 2, 3 (fsum::query_kernel's order).
// LDS: [x | z] 8.5 KB, c q_h / r 4.5 KB, dd / F_q 18.5 KB (the four partial tiles of F_q A, 17 KB, lie in it once F_q is dead, and the
// decoder's two hidden tiles later), the merged tile 32.5 KB, the per-row scalars 0.4 KB: 64.4 KB, two workgroups per CU.
#pragma once
#include "np_query.h"
#include "favor_summary.h"

namespace mlhot {

// the dimensions the kernel serves: np_query_ok's for the attention without the Nc clause (d.Nc and d.Nq are not looked at)
inline bool np_query_summary_ok(const mlhot_np_dims& d) {
#ifdef MLHOT_HOSTSIM
  (void)d; return false;
#else
  if (d.T < 1 || d.agg_mode != MLHOT_AGG_ATTENTION) return false;
  if (d.dim_w < 16 || d.dim_w % 16 || d.dim_w > 64 || d.dim_z < 4 || d.dim_z % 4 || d.dim_z > 64) return false;
  if (d.dec_hidden < 4 || d.dec_hidden % 4 || d.dec_hidden > 128 || d.y_dim < 1 || d.y_dim > 16) return false;
  return d.dim_r == d.dim_w && d.m_feat >= 16 && d.m_feat <= 272 && favor_summary_ok(d.T, MLHOT_HEADS, d.dim_w, d.m_feat);
#endif
}

// x_qry [T*Nq, dim_w] -> mu [T*Nq, y_dim] against a summary state (mlhot_favor_summary_bytes(T, 8, dim_w, m_feat) bytes).  d.Nc and
// d.Nq are ignored.  A task that has absorbed no shot has no defined output (0 / 0): the caller refuses it.
inline int np_query_summary_forward(const mlhot_np_dims& d, const mlhot_np_params& p, const float* x_qry, int Nq, const void* summary_state, float* mu,
                                    hipStream_t s) {
  if (Nq < 1 || !x_qry || !mu || !summary_state) { set_error("np_query_summary_fwd: bad argument"); return MLHOT_ERR_ARG; }
  if (!np_query_summary_ok(d)) {
    set_error("np_query_summary_fwd serves attention models with dim_w %% 16 == 0, dim_w <= 64, dim_z %% 4 == 0, dim_z <= 64, dec_hidden %% 4 == 0, "
              "dec_hidden <= 128, y_dim <= 16, dim_r == dim_w, 16 <= m <= 272 on the GPU build (got dim_w=%d dim_r=%d dim_z=%d dec_hidden=%d y_dim=%d m=%d)",
              d.dim_w, d.dim_r, d.dim_z, d.dec_hidden, d.y_dim, d.m_feat);
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifdef MLHOT_HOSTSIM
  (void)p; (void)s; return MLHOT_ERR_UNSUPPORTED;
#else
  bool have = p.r2z_w && p.r2z_b && p.wo_w && p.wo_b && p.proj;
  bool al = ft::aligned16(x_qry) && ft::aligned16(mu) && ft::aligned16(summary_state) && ft::aligned16(p.r2z_w) && ft::aligned16(p.wo_w) && ft::aligned16(p.proj);
  for (int i = 0; i < 3; ++i) { have = have && p.dec_w[i] && p.dec_b[i]; al = al && ft::aligned16(p.dec_w[i]); }
  for (int h = 0; h < MLHOT_HEADS; ++h) { have = have && p.wq_w[h] && p.wq_b[h]; al = al && ft::aligned16(p.wq_w[h]); }
  if (!have) { set_error("np_query_summary_fwd: a null pointer among the query-side parameters"); return MLHOT_ERR_ARG; }
  if (!al) { set_error("np_query_summary_fwd: x_qry, mu, the state and the weights must be 16-byte aligned"); return MLHOT_ERR_UNSUPPORTED; }
  const long long ntile = ((long long)Nq + nq::QT - 1) / nq::QT;
  if (ntile * d.T >= (1ll << 31)) { set_error("np_query_summary_fwd: T ceil(Nq / 16) must stay below 2^31 (chunk the targets)"); return MLHOT_ERR_ARG; }
  nq::Args a{};
  a.x = x_qry; a.mu = mu; a.proj = p.proj;
  for (int h = 0; h < MLHOT_HEADS; ++h) { a.wq_w[h] = p.wq_w[h]; a.wq_b[h] = p.wq_b[h]; }
  a.wo_w = p.wo_w; a.wo_b = p.wo_b; a.r2z_w = p.r2z_w; a.r2z_b = p.r2z_b;
  for (int i = 0; i < 3; ++i) { a.dec_w[i] = p.dec_w[i]; a.dec_b[i] = p.dec_b[i]; }
  a.T = d.T; a.Nq = Nq; a.Nc = 0; a.ntile = (int)ntile; a.dw = d.dim_w; a.dz = d.dim_z; a.dh = d.dec_hidden; a.y = d.y_dim;
  a.out_act = d.out_tanh ? ACT_TANH : ACT_NONE;
  const fsum::State st = fsum::carve_state(d.T, MLHOT_HEADS, d.dim_w, d.m_feat, const_cast<void*>(summary_state));
  if ((const float*)st.cnt != st.vs + (size_t)d.T * MLHOT_HEADS * d.dim_w + 16) { set_error("np_query_summary_fwd: the summary state's layout moved"); return MLHOT_ERR_ARG; }
  a.fk = st.A; a.v = st.a; a.z = st.vs;           // nq::Args: what SUMMARY reads through the context pointers
  a.m = d.m_feat; a.mp = st.mp;
  a.sc = ft::Scales(d.dim_w, d.m_feat);
  ProfScope ps("np.query.summary", s);
  hipLaunchKernelGGL((nq::query_kernel<true, true>), dim3((unsigned)(ntile * d.T)), dim3(256), 0, s, a);
  return check_launch("np.query.summary");
#endif
}

}  // namespace mlhot
