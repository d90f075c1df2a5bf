// Whole-model forward / backward of the vanilla CNP / ANP family (c1-c4):
// CNPVanillaPascal1D, CNPShapeNet1D, ANPVanillaPascal1D, ANPShapeNet1D.
// One C call enqueues the full kernel sequence; nothing returns to Python in between.
//
// Data flow (reference: CNPShapeNet1D.py:96-140, ANPShapeNet1D.py:93-157):
//   images --E1--> x_ctx (cols 0..dw of cat_in) | x_qry (cols 0..dw of dec_in)
//   cat_in = [x_ctx | transform_y(ctx_y)] --EncoderFC--> rs
//   CNP: r = agg(rs) -> z = r_to_z(r), broadcast over targets into dec_in[:, dw:]
//   ANP: K = W_k(x_ctx), V = W_v(rs), Q = W_q(x_qry) (8 heads in one GEMM each) -> FAVOR+
//        -> merged -> _W -> r_to_z -> dec_in[:, dw:]
//   mu = decoder0(dec_in)
#pragma once
#include "encoder.h"
#include "tail_fused.h"
#include "tail_spec.h"
#include "tail_cnp.h"
#include "cnp_spec.h"
#include "linear_skinny.h"
#include "favor2.h"
#include <initializer_list>
#include <type_traits>

namespace mlhot {

struct NpBuf {   // forward activations kept for the backward ("saved")
  void* enc;
  float *cat_in, *h[MLHOT_MAX_HIDDEN], *rs, *dec_in, *d1, *d2;
  float *r, *sigma, *zt, *mu_l, *lv; int32_t* amax;
  float *kh, *vh, *qh, *merged, *rr, *wot; void* favor; size_t favor_bytes;
  bool ok; size_t bytes;
};

inline NpBuf np_saved_carve(const mlhot_np_dims& d, void* base, size_t cap) {
  Arena a(base, cap);
  NpBuf b{};
  const size_t Rc = (size_t)d.T * d.Nc, Rq = (size_t)d.T * d.Nq;
  const int n = (int)(Rc + Rq), dw = d.dim_w, H = MLHOT_HEADS;
  b.enc = a.take<char>(enc_saved_bytes(n));
  b.dec_in = a.take<float>(Rq * (dw + d.dim_z));
  b.d1 = a.take<float>(Rq * d.dec_hidden);
  b.d2 = a.take<float>(Rq * d.dec_hidden);
  if (d.Nc > 0) {
    b.cat_in = a.take<float>(Rc * (dw + dw / 4));
    for (int i = 0; i < d.n_hidden; ++i) b.h[i] = a.take<float>(Rc * d.hidden[i]);
    b.rs = a.take<float>(Rc * d.dim_r);
    if (d.agg_mode == MLHOT_AGG_ATTENTION) {
      b.kh = a.take<float>(Rc * H * dw); b.vh = a.take<float>(Rc * H * dw); b.qh = a.take<float>(Rq * H * dw);
      b.merged = a.take<float>(Rq * H * dw); b.rr = a.take<float>(Rq * dw);
      b.wot = a.take<float>((size_t)H * dw * dw);      // head-major copy of _W's weight (fused tail)
      FavorDims f{d.T, H, d.Nq, d.Nc, dw, d.m_feat};
      b.favor_bytes = favor_ws_need(f);
      b.favor = a.take<char>(b.favor_bytes);
    } else {
      b.r = a.take<float>((size_t)d.T * d.dim_r); b.zt = a.take<float>((size_t)d.T * d.dim_z);
      b.amax = a.take<int32_t>((size_t)d.T * d.dim_r); b.sigma = a.take<float>((size_t)d.T * d.dim_r);
      if (d.agg_mode == MLHOT_AGG_BACO) { b.mu_l = a.take<float>(Rc * d.dim_r); b.lv = a.take<float>(Rc * d.dim_r); }
    }
  }
  b.ok = a.ok; b.bytes = a.off + 256;
  return b;
}

#ifndef MLHOT_HOSTSIM
// ---- the fused tails' dimension / parameter blocks (kernel arguments) -------------------------------
inline tf::TailDims tail_dims(const mlhot_np_dims& d) {
  return tf::TailDims{d.T, d.Nc, d.Nq, d.label_dim, d.y_dim, d.dim_w, d.dim_z, d.hidden[0], d.hidden[1], d.dec_hidden,
                      d.out_tanh ? ACT_TANH : ACT_NONE, d.m_feat};
}
inline tf::TailParams tail_params(const mlhot_np_params& p) {
  tf::TailParams q;
  q.ty_w = p.ty_w; q.ty_b = p.ty_b;
  for (int i = 0; i < 3; ++i) { q.er_w[i] = p.er_w[i]; q.er_b[i] = p.er_b[i]; q.dec_w[i] = p.dec_w[i]; q.dec_b[i] = p.dec_b[i]; }
  q.r2z_w = p.r2z_w; q.r2z_b = p.r2z_b;
  for (int i = 0; i < MLHOT_HEADS; ++i) {
    q.wk_w[i] = p.wk_w[i]; q.wk_b[i] = p.wk_b[i]; q.wv_w[i] = p.wv_w[i]; q.wv_b[i] = p.wv_b[i];
    q.wq_w[i] = p.wq_w[i]; q.wq_b[i] = p.wq_b[i];
  }
  q.wo_w = p.wo_w; q.wo_b = p.wo_b; q.proj = p.proj;
  return q;
}
inline tf::CnpDims cnp_dims(const mlhot_np_dims& d) {
  return tf::CnpDims{d.T, d.Nc, d.Nq, d.label_dim, d.y_dim, d.dim_w, d.dim_r, d.dim_z, d.hidden[0], d.hidden[1], d.dec_hidden,
                     d.out_tanh ? ACT_TANH : ACT_NONE, d.agg_mode};
}
inline tf::CnpParams cnp_params(const mlhot_np_params& p) {
  tf::CnpParams q;
  q.ty_w = p.ty_w; q.ty_b = p.ty_b; q.r2z_w = p.r2z_w; q.r2z_b = p.r2z_b;
  for (int i = 0; i < 3; ++i) { q.er_w[i] = p.er_w[i]; q.er_b[i] = p.er_b[i]; q.dec_w[i] = p.dec_w[i]; q.dec_b[i] = p.dec_b[i]; }
  return q;
}
#endif

// ---- the route: what runs between the encoder and the loss for these dims and these options -----------------
// np_route() is the ONE place that reads the dims' limits and the options tail_fused / tail_spec (the encoder's side of enc_fold comes
// from enc_route(), encoder.h); np_forward, np_backward, np_scratch_carve and np_grads_flat_layout take its answer and pass it down.
enum class Tail { Generic, Attention, Cnp };   // the operator chain below | tail_fused.h + tail_spec.h | tail_cnp.h + cnp_spec.h
struct NpRoute {
  Tail family;
  Tail slab;            // whose per-task gradient slab the scratch reserves: every two-hidden-layer model of that aggregation, whatever
                        // the options and the shot counts (wider than `family`; mlhot_np_scratch_bytes has always reported it so)
  // Which launches are the kernels specialised for the shipped dimensions (false: the run-time-shaped ones).  The CNP tail is one
  // kernel per direction: fwd_A is its forward, bwd_C its backward, the other four stay false.
  bool fwd_A, fwd_B, fwd_C, bwd_C, bwd_B, bwd_A;
  bool enc_fold;        // the first forward kernel folds the encoder Linear's split-K partial results (the encoder skips its own fold)
  bool loss_in_kernel;  // the first backward kernel takes a loss descriptor itself (otherwise np_backward materialises the gradient)
  bool bwd_B_split;     // B' as two workgroups per (task, head): query side | key / value side
  int bwd_C_wg, bwd_A_wg;   // workgroups per task of C' (the CNP backward) and A': 1, 2 or 4
};
// gfx950 (CDNA4): 160 KB of LDS per compute unit, and one workgroup may have all of it.  A launch that asks for more is refused by
// hipFuncSetAttribute (tail_launch), so a family whose kernels need more is never picked.
constexpr size_t LDS_PER_WORKGROUP = 160 * 1024;
static_assert(LDS_PER_WORKGROUP == 163840, "gfx950: 160 KB of LDS per workgroup");
#ifndef MLHOT_HOSTSIM
inline bool lds_fits(std::initializer_list<size_t> launches) {
  for (size_t bytes : launches) if (bytes > LDS_PER_WORKGROUP) return false;
  return true;
}
// every launch of the attention family, forward and backward, with the kernels the bits `spec` select
inline bool tail_lds_fits(const tf::TailDims& td, int spec) {
  return lds_fits({(spec & TAIL_SPEC_FWD_A) ? ts::phaseA_lds_bytes() : tf::phaseA_lds_bytes(td),
                   (spec & TAIL_SPEC_FWD_B) ? ts::phaseB_lds_bytes() : tf::phaseB_lds_bytes(td),
                   (spec & TAIL_SPEC_FWD_C) ? ts::phaseC_lds_bytes() : tf::phaseC_lds_bytes(td),
                   (spec & TAIL_SPEC_BWD_C) ? ts::phaseC_bwd_lds_bytes() : tf::phaseC_bwd_lds_bytes(td),
                   (spec & TAIL_SPEC_BWD_B) ? ts::phaseB_bwd_lds_bytes() : tf::phaseB_bwd_lds_bytes(td),
                   (spec & TAIL_SPEC_BWD_A) ? ts::phaseA_bwd_lds_bytes() : tf::phaseA_bwd_lds_bytes(td)});
}
inline bool cnp_lds_fits(const tf::CnpDims& cd, int spec) {
  return lds_fits({(spec & TAIL_SPEC_FWD_A) ? ts::cnp_fwd_lds_bytes() : tf::cnp_fwd_lds_bytes(cd),
                   (spec & TAIL_SPEC_BWD_C) ? ts::cnp_bwd_lds_bytes() : tf::cnp_bwd_lds_bytes(cd)});
}
#endif
inline NpRoute np_route(const mlhot_np_dims& d) {
  NpRoute r{};
  r.bwd_C_wg = r.bwd_A_wg = 1;
#ifndef MLHOT_HOSTSIM      // the host simulation has the operator chain only
  static_assert(ts::XK == el::F_KS, "the first forward kernel folds the encoder Linear's split-K factor");
  const bool attn = d.agg_mode == MLHOT_AGG_ATTENTION, pooled = d.agg_mode == MLHOT_AGG_MEAN || d.agg_mode == MLHOT_AGG_MAX;
  if (d.Nc > 0 && d.n_hidden == 2) r.slab = attn ? Tail::Attention : pooled ? Tail::Cnp : Tail::Generic;
  const bool one_tile = g_opt.tail_fused && d.Nc >= 1 && d.Nc <= 16 && d.Nq <= 16 && d.n_hidden == 2;   // a task's rows fit one 16-row tile
  // One decision for both directions (they share the saved and scratch layouts): a fused family is picked only when EVERY launch of
  // it, forward and backward, gets its LDS; otherwise the operator chain runs.
  int spec = 0;
  if (one_tile && attn && d.dim_w % 64 == 0 && d.dim_w <= tf::KEYHEAD_MAX_DW && d.dim_r == d.dim_w && d.m_feat <= tf::KMAX_COLS &&
      (long long)d.T * d.Nc * MLHOT_HEADS < (1ll << 19)) {      // key arg-max positions are packed row * 4096 + col
    const tf::TailDims td = tail_dims(d);
    const int sp = ts::applies(td) ? g_opt.tail_spec : 0;
    if (tail_lds_fits(td, sp)) { r.family = Tail::Attention; spec = sp; }
  } else if (one_tile && pooled && d.dim_w % 16 == 0 && d.dim_r <= 128) {
    const tf::CnpDims cd = cnp_dims(d);
    const int sp = ts::cnp_applies(cd)
        ? g_opt.tail_spec & (TAIL_SPEC_FWD_A | TAIL_SPEC_BWD_C | TAIL_SPEC_ENC_FOLD | TAIL_SPEC_LOSS | TAIL_SPEC_BWD_C_WG2 | TAIL_SPEC_WG4) : 0;
    if (cnp_lds_fits(cd, sp)) { r.family = Tail::Cnp; spec = sp; }
  }
  r.fwd_A = spec & TAIL_SPEC_FWD_A; r.fwd_B = spec & TAIL_SPEC_FWD_B; r.fwd_C = spec & TAIL_SPEC_FWD_C;
  r.bwd_C = spec & TAIL_SPEC_BWD_C; r.bwd_B = spec & TAIL_SPEC_BWD_B; r.bwd_A = spec & TAIL_SPEC_BWD_A;
  r.enc_fold = r.fwd_A && (spec & TAIL_SPEC_ENC_FOLD) && enc_route(d.T * (d.Nc + d.Nq), d.dim_w).own_linear;
  r.loss_in_kernel = r.bwd_C && (spec & TAIL_SPEC_LOSS);
  r.bwd_B_split = r.bwd_B && (spec & TAIL_SPEC_BWD_B_SPLIT);
  const int wg = (spec & TAIL_SPEC_WG4) ? 4 : 2;
  if (r.bwd_C && (spec & TAIL_SPEC_BWD_C_WG2)) r.bwd_C_wg = wg;
  if (r.bwd_A && (spec & TAIL_SPEC_BWD_A_WG2)) r.bwd_A_wg = wg;
#endif
  return r;
}

// ---- the parameter table: the tail's parameters in the order their gradients lie in a per-task slab ----------
// The slab layouts the kernels index (tf::TailSlab / tf::CnpSlab), the slab reduce's segments and the flat gradient layout are all
// derived from tail_table(); the contiguous one-launch reduce is correct because they are.
struct TailParam {
  size_t grad;    // offsetof(mlhot_np_grads, .): its gradient pointer (a head stack's: the first of MLHOT_HEADS consecutive ones)
  size_t field;   // offsetof(tf::TailSlab, .): the field a kernel reads its slab offset from (tf::CnpSlab: the same place)
  int len;        // floats (of one head)
  int heads;      // 1, or MLHOT_HEADS: a head stack, its heads' blocks back to back
  bool attn;      // attention models only
  int off;        // slab offset in floats; every entry starts 4-float aligned
};
struct TailTable { TailParam p[2 * (MLHOT_MAX_HIDDEN + 1) + 18]; int n, total; };
#ifndef MLHOT_HOSTSIM
#define MLHOT_TAIL_ROW(f, i) offsetof(mlhot_np_grads, f) + (i) * sizeof(float*), offsetof(tf::TailSlab, f) + (i) * sizeof(int)
#else
#define MLHOT_TAIL_ROW(f, i) offsetof(mlhot_np_grads, f) + (i) * sizeof(float*), 0      // no slabs without the fused tails
#endif
inline TailTable tail_table(const mlhot_np_dims& d) {
  const int dw = d.dim_w, dr = d.dim_r, dz = d.dim_z, dh = d.dec_hidden, H = MLHOT_HEADS;
  TailTable t{};
  auto row = [&](size_t grad, size_t field, int len, int heads = 1, bool attn = false) {
    t.p[t.n++] = TailParam{grad, field, len, heads, attn, t.total};
    t.total += (len * heads + 3) / 4 * 4;
  };
  row(MLHOT_TAIL_ROW(ty_w, 0), dw / 4 * d.label_dim); row(MLHOT_TAIL_ROW(ty_b, 0), dw / 4);
  for (int i = 0, in = dw + dw / 4; i <= d.n_hidden; ++i) {          // EncoderFC: the hidden layers, then the one onto dim_r
    const int out = i < d.n_hidden ? d.hidden[i] : dr;
    row(MLHOT_TAIL_ROW(er_w, i), out * in); row(MLHOT_TAIL_ROW(er_b, i), out);
    in = out;
  }
  row(MLHOT_TAIL_ROW(r2z_w, 0), dz * dr); row(MLHOT_TAIL_ROW(r2z_b, 0), dz);
  row(MLHOT_TAIL_ROW(dec_w, 0), dh * (dw + dz)); row(MLHOT_TAIL_ROW(dec_b, 0), dh);
  row(MLHOT_TAIL_ROW(dec_w, 1), dh * dh); row(MLHOT_TAIL_ROW(dec_b, 1), dh);
  row(MLHOT_TAIL_ROW(dec_w, 2), d.y_dim * dh); row(MLHOT_TAIL_ROW(dec_b, 2), d.y_dim);
  if (d.agg_mode == MLHOT_AGG_ATTENTION) {                           // (dim_r == dim_w)
    row(MLHOT_TAIL_ROW(wk_w, 0), dw * dw, H, true); row(MLHOT_TAIL_ROW(wk_b, 0), dw, H, true);
    row(MLHOT_TAIL_ROW(wv_w, 0), dw * dw, H, true); row(MLHOT_TAIL_ROW(wv_b, 0), dw, H, true);
    row(MLHOT_TAIL_ROW(wq_w, 0), dw * dw, H, true); row(MLHOT_TAIL_ROW(wq_b, 0), dw, H, true);
    row(MLHOT_TAIL_ROW(wo_w, 0), dw * H * dw, 1, true); row(MLHOT_TAIL_ROW(wo_b, 0), dw, 1, true);
  }
  return t;
}
#undef MLHOT_TAIL_ROW
// entry `r`'s (head `h`'s) pointer in a gradient block
inline float*& tail_grad(mlhot_np_grads& g, const TailParam& r, int h = 0) {
  return reinterpret_cast<float**>(reinterpret_cast<char*>(&g) + r.grad)[h];
}

struct NpScratch {
  void* enc; size_t enc_bytes;
  float *d_dec_in, *dd1, *dd2, *d_cat_in, *dh[MLHOT_MAX_HIDDEN], *d_rs;
  float *d_rr, *d_merged, *dqh, *dkh, *dvh, *dzt, *dr, *d_mu_l, *d_lv;
  float* tail_slab;   // fused tail: per-task weight-gradient partials
  float* dmu_tmp;     // [Rq][y_dim]: upstream gradient + the loss's own, where the first backward kernel cannot take the loss itself
  bool ok; size_t bytes;
};

inline NpScratch np_scratch_carve(const mlhot_np_dims& d, const NpRoute& rt, void* base, size_t cap) {
  Arena a(base, cap);
  NpScratch s{};
  const size_t Rc = (size_t)d.T * d.Nc, Rq = (size_t)d.T * d.Nq;
  const int n = (int)(Rc + Rq), dw = d.dim_w, H = MLHOT_HEADS;
  s.enc_bytes = enc_scratch_bytes(n, dw);
  s.enc = a.take<char>(s.enc_bytes);
  s.d_dec_in = a.take<float>(Rq * (dw + d.dim_z));
  s.dd1 = a.take<float>(Rq * d.dec_hidden); s.dd2 = a.take<float>(Rq * d.dec_hidden);
  s.dmu_tmp = a.take<float>(Rq * d.y_dim);
  if (d.Nc > 0) {
    s.d_cat_in = a.take<float>(Rc * (dw + dw / 4));
    for (int i = 0; i < d.n_hidden; ++i) s.dh[i] = a.take<float>(Rc * d.hidden[i]);
    s.d_rs = a.take<float>(Rc * d.dim_r);
    if (d.agg_mode == MLHOT_AGG_ATTENTION) {
      s.d_rr = a.take<float>(Rq * dw); s.d_merged = a.take<float>(Rq * H * dw);
      s.dqh = a.take<float>(Rq * H * dw); s.dkh = a.take<float>(Rc * H * dw); s.dvh = a.take<float>(Rc * H * dw);
    } else {
      s.dzt = a.take<float>((size_t)d.T * d.dim_z); s.dr = a.take<float>((size_t)d.T * d.dim_r);
      if (d.agg_mode == MLHOT_AGG_BACO) { s.d_mu_l = a.take<float>(Rc * d.dim_r); s.d_lv = a.take<float>(Rc * d.dim_r); }
    }
    if (rt.slab != Tail::Generic) s.tail_slab = a.take<float>((size_t)d.T * tail_table(d).total);
  }
  s.ok = a.ok; s.bytes = a.off + 256;
  return s;
}

// What every route needs of the dims; a refusal names the width it is about.  Which widths must be multiples of 4: dim_w (rows of
// kh / vh / qh and of the projection matrix are read as float4 by FAVOR+, favor2.h) and dim_z (rows of d_dec_in, dim_w + dim_z wide,
// are read as float4 by the encoder Linear's backward, enc_linear.h).  hidden[], dec_hidden and dim_r need not be: linear_skinny.h is
// entered only with K % 4 == 0 / N % 4 == 0 and 16-byte aligned rows (lin_fwd, lin_dgrad below), and the fused tails' layer function
// reads weights as float4 only when its K % 4 == 0 (wg_linear_t, tail_fused.h).
inline int np_check_dims(const mlhot_np_dims& d) {
  if (d.T <= 0 || d.Nq <= 0 || d.Nc < 0 || d.n_hidden < 1 || d.n_hidden > MLHOT_MAX_HIDDEN ||
      d.agg_mode < 0 || d.agg_mode > 3 || d.y_dim < 1 || d.y_dim > 8) {
    set_error("np_vanilla: bad dims (T %d, Nc %d, Nq %d, n_hidden %d, agg_mode %d, y_dim %d)", d.T, d.Nc, d.Nq, d.n_hidden, d.agg_mode, d.y_dim);
    return MLHOT_ERR_ARG;
  }
  if (d.dim_w < 4 || d.dim_w % 4) { set_error("np_vanilla: dim_w = %d must be a positive multiple of 4", d.dim_w); return MLHOT_ERR_ARG; }
  if (d.dim_z < 4 || d.dim_z % 4) { set_error("np_vanilla: dim_z = %d must be a positive multiple of 4", d.dim_z); return MLHOT_ERR_ARG; }
  if (d.dim_r < 1) { set_error("np_vanilla: dim_r = %d must be positive", d.dim_r); return MLHOT_ERR_ARG; }
  if (d.dec_hidden < 1) { set_error("np_vanilla: dec_hidden = %d must be positive", d.dec_hidden); return MLHOT_ERR_ARG; }
  if (d.label_dim < 1) { set_error("np_vanilla: label_dim = %d must be positive", d.label_dim); return MLHOT_ERR_ARG; }
  for (int i = 0; i < d.n_hidden; ++i)
    if (d.hidden[i] < 1) { set_error("np_vanilla: hidden[%d] = %d must be positive", i, d.hidden[i]); return MLHOT_ERR_ARG; }
  if (d.agg_mode == MLHOT_AGG_ATTENTION && (d.dim_r != d.dim_w || d.m_feat <= 0)) {
    set_error("np_vanilla: attention needs dim_r == dim_w and m_feat > 0 (dim_r %d, dim_w %d, m_feat %d)", d.dim_r, d.dim_w, d.m_feat); return MLHOT_ERR_ARG;
  }
  // row counts and row * width products are ints in the launches' arguments (T * Nc, T * Nq rows; the widest row is the head stack's)
  long long widest = (long long)d.dim_w + (d.dim_z > d.dim_w / 4 ? d.dim_z : d.dim_w / 4);
  if (d.agg_mode == MLHOT_AGG_ATTENTION) widest = (long long)MLHOT_HEADS * d.dim_w > widest ? (long long)MLHOT_HEADS * d.dim_w : widest;
  if (d.dim_r > widest) widest = d.dim_r;
  if (d.dec_hidden > widest) widest = d.dec_hidden;
  for (int i = 0; i < d.n_hidden; ++i) if (d.hidden[i] > widest) widest = d.hidden[i];
  if (((long long)d.T * d.Nc + (long long)d.T * d.Nq) * widest >= (1ll << 31)) {
    set_error("np_vanilla: T * (Nc + Nq) = %lld rows of up to %lld floats overflow the kernels' 32-bit indices", (long long)d.T * ((long long)d.Nc + d.Nq), widest);
    return MLHOT_ERR_UNSUPPORTED;
  }
  return MLHOT_OK;
}

// ---- thin wrappers over the igemm problems -------------------------------------------------
inline WBlocks wb1(const float* w, const float* b, int rows) { WBlocks x{}; x.w[0] = w; x.b[0] = b; x.rows = rows; return x; }
inline WBlocks wb8(const float* const* w, const float* const* b, int rows) {
  WBlocks x{}; for (int i = 0; i < MLHOT_HEADS; ++i) { x.w[i] = w[i]; x.b[i] = b ? b[i] : nullptr; } x.rows = rows; return x;
}
inline WBlocksMut gb1(float* w, float* b, int rows) { WBlocksMut x{}; x.w[0] = w; x.b[0] = b; x.rows = rows; return x; }
inline WBlocksMut gb8(float* const* w, float* const* b, int rows) {
  WBlocksMut x{}; for (int i = 0; i < MLHOT_HEADS; ++i) { x.w[i] = w[i]; x.b[i] = b[i]; } x.rows = rows; return x;
}

// Few-row layers with a single weight block and 16-byte aligned rows take the direct-from-global kernels (linear_skinny.h).
inline int lin_fwd(const float* x, int ldx, const WBlocks& wb, float* y, int ldy, int M, int K, int N, int act,
                   hipStream_t s, const char* what) {
#ifndef MLHOT_HOSTSIM
  if (M <= sk::MAX_ROWS && wb.w[1] == nullptr && wb.rows >= N && K % 4 == 0 && sk::aligned4(x, ldx) && sk::aligned4(wb.w[0], K))
    return sk::run_fwd(x, ldx, wb.w[0], wb.b[0], y, ldy, M, K, N, act, s, what);
#endif
  LinearFwd p{M, N, K, x, ldx, wb, y, ldy, act};
  return run_igemm_auto(p, s, what);
}
// dx[M][Kin] (+)= (dy * act'(y)) W
inline int lin_dgrad(const float* dy, int lddy, const float* y, int ldy, int act, const WBlocks& wb,
                     float* dx, int lddx, int accumulate, int M, int Kin, int Nout, hipStream_t s, const char* what) {
#ifndef MLHOT_HOSTSIM
  if (M <= sk::MAX_ROWS && wb.w[1] == nullptr && wb.rows >= Nout && Nout % 4 == 0 && sk::aligned4(dy, lddy) && (act == ACT_NONE || sk::aligned4(y, ldy)))
    return sk::run_dgrad(dy, lddy, y, ldy, act, wb.w[0], dx, lddx, accumulate, M, Kin, Nout, s, what);
#endif
  LinearDgrad p{M, Kin, Nout, dy, lddy, y, ldy, act, wb, dx, lddx, accumulate};
  return run_igemm_auto(p, s, what);
}
inline int lin_wgrad(const float* dy, int lddy, const float* y, int ldy, int act, const float* x, int ldx,
                     const WBlocksMut& gb, int M, int Kin, int Nout, hipStream_t s, const char* what) {
#ifndef MLHOT_HOSTSIM
  if (M <= sk::MAX_ROWS && gb.w[1] == nullptr && gb.rows >= Nout)
    return sk::run_wgrad(dy, lddy, y, ldy, act, x, ldx, gb.w[0], gb.b[0], M, Kin, Nout, s, what);
#endif
  LinearWgrad p{Nout, Kin + 1, M, dy, lddy, y, ldy, act, x, ldx, gb};
  return run_igemm_auto(p, s, what);
}

#ifndef MLHOT_HOSTSIM
// ---- the fused tails' launches (kernels: tail_fused.h / tail_spec.h, tail_cnp.h / cnp_spec.h) -----------------------
template <class K, class A, class... More>
inline int tail_launch(K kernel, int grid, int block, size_t lds, const A& args, hipStream_t s, const char* what, const More&... more) {
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    set_error("%s: %zu bytes of LDS refused", what, lds);
    return MLHOT_ERR_LAUNCH;
  }
  {
    ProfScope ps(what, s);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, s, args, more...);
  }
  return check_launch(what);
}
// launch(integral_constant<G>) with G = wg: picks a kernel template's instance for 1, 2 or 4 workgroups per task
template <class F>
inline int with_wg(int wg, F launch) {
  if (wg == 4) return launch(std::integral_constant<int, 4>{});
  if (wg == 2) return launch(std::integral_constant<int, 2>{});
  return launch(std::integral_constant<int, 1>{});
}

// the kernels' slab-offset block, filled from the parameter table
template <class Slab>
inline Slab slab_layout(const TailTable& t) {
  static_assert(offsetof(tf::CnpSlab, ty_w) == offsetof(tf::TailSlab, ty_w) && offsetof(tf::CnpSlab, er_w) == offsetof(tf::TailSlab, er_w) &&
                offsetof(tf::CnpSlab, er_b) == offsetof(tf::TailSlab, er_b) && offsetof(tf::CnpSlab, r2z_w) == offsetof(tf::TailSlab, r2z_w) &&
                offsetof(tf::CnpSlab, dec_w) == offsetof(tf::TailSlab, dec_w) && offsetof(tf::CnpSlab, dec_b) == offsetof(tf::TailSlab, dec_b),
                "TailParam::field serves both slab blocks");
  Slab sl{};
  for (int i = 0; i < t.n; ++i) *reinterpret_cast<int*>(reinterpret_cast<char*>(&sl) + t.p[i].field) = t.p[i].off;
  sl.total = t.total;
  return sl;
}
// Per-task slabs -> parameter gradients.  When the caller laid the gradient tensors out as ONE flat buffer in slab
// order (mlhot_np_grads_flat_layout) the reduce is a single contiguous float4 sum; otherwise every element looks up
// its destination segment.
// `later`: where a contiguous sum may be parked instead of launched (the encoder backward that follows folds it into its own
// final reduce launch).
inline int tail_slab_reduce(const TailTable& t, const mlhot_np_grads& g, int T, const float* slab, hipStream_t s, PendingSum* later) {
  static_assert(16 + 6 * MLHOT_HEADS + 2 <= tf::MAX_SEG, "one segment per gradient tensor");
  tf::SlabReduce r{};
  for (int i = 0; i < t.n; ++i)
    for (int h = 0; h < t.p[i].heads; ++h, ++r.nseg) {
      r.dst[r.nseg] = reinterpret_cast<float* const*>(reinterpret_cast<const char*>(&g) + t.p[i].grad)[h]; r.off[r.nseg] = t.p[i].off + h * t.p[i].len; r.len[r.nseg] = t.p[i].len;
    }
  r.T = T; r.total = t.total; r.slab = slab;
  bool flat = r.nseg > 0 && r.off[0] == 0 && (reinterpret_cast<uintptr_t>(r.dst[0]) & 15) == 0 && (r.total & 3) == 0;
  for (int i = 1; flat && i < r.nseg; ++i) flat = r.dst[i] == r.dst[0] + r.off[i];
  if (flat && later != nullptr) {
    *later = PendingSum{r.slab, r.dst[0], r.T, r.total, r.total};
    return MLHOT_OK;
  }
  {
    ProfScope ps("tail.bwd.reduce", s);
    if (flat) hipLaunchKernelGGL(c2::sum_parts_kernel, dim3((r.total + 63) / 64), dim3(256), 0, s, r.slab, r.T, r.total, r.dst[0], r.total);
    else hipLaunchKernelGGL(tf::slab_to_grads_kernel, dim3((r.total + 255) / 256), dim3(256), 0, s, r);
  }
  return check_launch("tail.bwd.reduce");
}

// ---- fused attention tail ---------------------------------------------------------------------------
struct TailView { tf::TailDims td; tf::TailParams tp; FavorWs w; };   // what its forward and its backward both build their arguments from
inline TailView tail_view(const mlhot_np_dims& d, const mlhot_np_params& p, const NpBuf& b) {
  const FavorDims f{d.T, MLHOT_HEADS, d.Nq, d.Nc, d.dim_w, d.m_feat};
  return TailView{tail_dims(d), tail_params(p), favor_carve(f, b.favor, b.favor_bytes)};
}
inline int tail_forward_fused(const mlhot_np_dims& d, const mlhot_np_params& p, const NpRoute& rt, const float* ctx_y, float* mu,
                              const NpBuf& b, const NpScratch& sc, hipStream_t s, const Stage& st, const EncXFold& xf) {
  const TailView v = tail_view(d, p, b);
  const tf::TailDims& td = v.td; const tf::TailParams& tp = v.tp; const FavorWs& w = v.w;
  const int TH = d.T * MLHOT_HEADS;
  if (!w.ok || !sc.d_merged) { set_error("tail_fused: workspace"); return MLHOT_ERR_WORKSPACE; }
  tf::PhaseAArgs a{g_opt.dbg, td, tp, ctx_y, b.cat_in, b.h[0], b.h[1], b.rs, b.dec_in, b.kh, w.pc, w.max_k, w.arg_k, b.wot, xf.slab, xf.bias, xf.k, xf.n};
  if (xf.slab != nullptr && !rt.fwd_A) { set_error("tail_fused: the encoder left its fold to a phase A that cannot do it"); return MLHOT_ERR_ARG; }
  if (st.first()) {
    if (rt.fwd_A) MLHOT_TRY(tail_launch(ts::phaseA_fwd_kernel, d.T + TH + (xf.slab != nullptr ? d.T : 0), 512, ts::phaseA_lds_bytes(), a, s, "tail.A"));
    else MLHOT_TRY(tail_launch(tf::phaseA_fwd_kernel, d.T + TH, 512, tf::phaseA_lds_bytes(td), a, s, "tail.A"));
  }
  // strict sharded parity (stab_xchg.h): phase B folds the (task, head) shares (max_k, arg_k) into the batch-global key stabiliser
  if (st.stage == 0) return sx::max_publish(w.max_k, TH, st.x, s);
  if (st.stage == 1) MLHOT_TRY(sx::max_apply(w.max_k, w.arg_k, TH, st.x, s));
  tf::PhaseBArgs bb{td, tp, b.dec_in, b.rs, b.qh, b.vh, b.kh, w.pc, w.max_k, w.arg_k, w.qf, w.kf, w.S, w.D, w.gmax, w.arg_q, w.gpos, b.merged, sc.d_merged, b.wot};   // sc.d_merged: forward scratch for the heads' _W shares
  if (rt.fwd_B) MLHOT_TRY(tail_launch(ts::phaseB_fwd_kernel, TH, 512, ts::phaseB_lds_bytes(), bb, s, "tail.B"));
  else MLHOT_TRY(tail_launch(tf::phaseB_fwd_kernel, TH, 512, tf::phaseB_lds_bytes(td), bb, s, "tail.B"));
  tf::PhaseCArgs c{td, tp, sc.d_merged, b.rr, b.dec_in, b.d1, b.d2, mu};
  if (rt.fwd_C) MLHOT_TRY(tail_launch(ts::phaseC_fwd_kernel, d.T, 512, ts::phaseC_lds_bytes(), c, s, "tail.C"));
  else MLHOT_TRY(tail_launch(tf::phaseC_fwd_kernel, d.T, 512, tf::phaseC_lds_bytes(td), c, s, "tail.C"));
  return MLHOT_OK;
}
inline int tail_backward_fused(const mlhot_np_dims& d, const mlhot_np_params& p, const NpRoute& rt, const float* ctx_y, const float* mu,
                               const float* dmu, const mlhot_np_grads& g, const NpBuf& b, const NpScratch& sc, hipStream_t s,
                               PendingSum* later, const Stage& st, const LossDesc& loss) {
  const TailView v = tail_view(d, p, b);
  const tf::TailDims& td = v.td; const tf::TailParams& tp = v.tp; const FavorWs& w = v.w;
  const TailTable tab = tail_table(d);
  const tf::TailSlab sl = slab_layout<tf::TailSlab>(tab);
  const int TH = d.T * MLHOT_HEADS;
  if (!w.ok || !sc.tail_slab) { set_error("tail_fused: workspace"); return MLHOT_ERR_WORKSPACE; }
  float* part_k = w.rsum_k;   // [T*H]
  tf::PhaseCBwdArgs c{td, tp, sl, dmu, mu, b.d2, b.d1, b.dec_in, b.rr, sc.d_dec_in, sc.d_rr, sc.tail_slab, loss};
  if (loss.kind >= 0 && !rt.loss_in_kernel) { set_error("tail_fused: a loss descriptor reached a phase C' that cannot take it"); return MLHOT_ERR_ARG; }
  // sc.dqh / dkh / dvh double as the heads' input-gradient shares [T*H][N][dw] (same sizes)
  tf::PhaseBBwdArgs bb{td, tp, sl, b.qh, b.kh, b.vh, w.pc, w.qf, w.kf, w.S, w.D, b.merged, sc.d_rr, w.arg_q,
                       b.dec_in, b.cat_in, b.rs, b.wot, sc.dqh, sc.dkh, sc.dvh, part_k, sc.tail_slab};
  if (st.first()) {
    const int lv = loss.value != nullptr ? 1 : 0;           // one workgroup more: the loss value
    if (rt.bwd_C) MLHOT_TRY(with_wg(rt.bwd_C_wg, [&](auto G) { return tail_launch(ts::phaseC_bwd_kernel<decltype(G)::value>, G * d.T + lv, 512, ts::phaseC_bwd_lds_bytes(), c, s, "tail.bwd.C"); }));
    else MLHOT_TRY(tail_launch(tf::phaseC_bwd_kernel, d.T, 512, tf::phaseC_bwd_lds_bytes(td), c, s, "tail.bwd.C"));
    if (rt.bwd_B_split) MLHOT_TRY(tail_launch(ts::phaseB_bwd_kernel<true>, 2 * TH, 512, ts::phaseB_bwd_lds_bytes(), bb, s, "tail.bwd.B"));
    else if (rt.bwd_B) MLHOT_TRY(tail_launch(ts::phaseB_bwd_kernel<false>, TH, 512, ts::phaseB_bwd_lds_bytes(), bb, s, "tail.bwd.B"));
    else MLHOT_TRY(tail_launch(tf::phaseB_bwd_kernel, TH, 512, tf::phaseB_bwd_lds_bytes(td), bb, s, "tail.bwd.B"));
  }
  // strict sharded parity: phase A folds part_k into the stabiliser's gradient and routes it to the arg-max key's task
  if (st.stage == 0) return sx::sum_publish(part_k, TH, st.x, s);
  if (st.stage == 1) MLHOT_TRY(sx::sum_apply(part_k, TH, st.x, part_k, 1, s));
  tf::PhaseABwdArgs a{td, tp, sl, ctx_y, b.cat_in, b.h[0], b.h[1], sc.dqh, sc.dkh, sc.dvh, w.pc, part_k, w.gpos,
                      sc.d_dec_in, sc.d_cat_in, sc.tail_slab};
  if (rt.bwd_A) MLHOT_TRY(with_wg(rt.bwd_A_wg, [&](auto G) { return tail_launch(ts::phaseA_bwd_kernel<decltype(G)::value>, G * d.T, 512, ts::phaseA_bwd_lds_bytes(), a, s, "tail.bwd.A"); }));
  else MLHOT_TRY(tail_launch(tf::phaseA_bwd_kernel, d.T, 512, tf::phaseA_bwd_lds_bytes(td), a, s, "tail.bwd.A"));
  return tail_slab_reduce(tab, g, d.T, sc.tail_slab, s, later);
}

// ---- fused CNP tail: one kernel per direction ----------------------------------------------------------
inline int cnp_forward_fused(const mlhot_np_dims& d, const mlhot_np_params& p, const NpRoute& rt, const float* ctx_y, float* mu,
                             const NpBuf& b, hipStream_t s, const EncXFold& xf) {
  const tf::CnpDims cd = cnp_dims(d);
  tf::CnpFwdArgs a{cd, cnp_params(p), ctx_y, b.cat_in, b.h[0], b.h[1], b.rs, b.r, b.zt, b.dec_in, b.d1, b.d2, mu, b.amax};
  if (rt.fwd_A) return tail_launch(ts::cnp_fwd_kernel, d.T, 512, ts::cnp_fwd_lds_bytes(), a, s, "tail.cnp", ts::CnpXFold{xf.slab, xf.bias, xf.k, xf.n});
  if (xf.slab != nullptr) { set_error("cnp_fused: the encoder left its fold to a tail kernel that cannot do it"); return MLHOT_ERR_ARG; }
  return tail_launch(tf::cnp_fwd_kernel, d.T, 512, tf::cnp_fwd_lds_bytes(cd), a, s, "tail.cnp");
}
inline int cnp_backward_fused(const mlhot_np_dims& d, const mlhot_np_params& p, const NpRoute& rt, const float* ctx_y, const float* mu,
                              const float* dmu, const mlhot_np_grads& g, const NpBuf& b, const NpScratch& sc, hipStream_t s,
                              PendingSum* later, const LossDesc& loss) {
  const tf::CnpDims cd = cnp_dims(d);
  const TailTable tab = tail_table(d);
  if (!sc.tail_slab) { set_error("cnp_fused: workspace"); return MLHOT_ERR_WORKSPACE; }
  tf::CnpBwdArgs a{cd, cnp_params(p), slab_layout<tf::CnpSlab>(tab), ctx_y, dmu, mu, b.d2, b.d1, b.dec_in, b.r, b.rs, b.h[1], b.h[0], b.cat_in, b.amax,
                   sc.d_dec_in, sc.d_cat_in, sc.tail_slab};
  if (rt.bwd_C) {
    const int lv = loss.value != nullptr ? 1 : 0;           // one workgroup more: the loss value
    MLHOT_TRY(with_wg(rt.bwd_C_wg, [&](auto G) { return tail_launch(ts::cnp_bwd_kernel<decltype(G)::value>, G * d.T + lv, 512, ts::cnp_bwd_lds_bytes(), a, s, "tail.bwd.cnp", loss); }));
  } else {
    if (loss.kind >= 0) { set_error("cnp_fused: a loss descriptor reached a backward kernel that cannot take it"); return MLHOT_ERR_ARG; }
    MLHOT_TRY(tail_launch(tf::cnp_bwd_kernel, d.T, 512, tf::cnp_bwd_lds_bytes(cd), a, s, "tail.bwd.cnp"));
  }
  return tail_slab_reduce(tab, g, d.T, sc.tail_slab, s, later);
}
#endif

// Layout of ONE flat gradient buffer: the fused tails' parameters at their slab offsets (so the per-task slabs reduce
// with a single contiguous sum), everything else packed behind, 4-float aligned.  `o` receives BYTE offsets in its
// pointer fields (fields of parameters the model does not have stay null); returns the buffer size in floats.
inline size_t np_grads_flat_layout(const mlhot_np_dims& d, const NpRoute& rt, mlhot_np_grads& o) {
  memset(&o, 0, sizeof(o));
  const int dw = d.dim_w;
  size_t next = 0;
  auto at = [](size_t off_floats) { return reinterpret_cast<float*>(off_floats * sizeof(float)); };
  auto take = [&](size_t n) { const size_t r = next; next += (n + 3) / 4 * 4; return at(r); };
  const TailTable t = tail_table(d);
  const TailParam* const end = t.p + t.n;
  if (rt.family != Tail::Generic) {
    for (const TailParam* r = t.p; r != end; ++r)
      for (int h = 0; h < r->heads; ++h) tail_grad(o, *r, h) = at(r->off + (size_t)h * r->len);
    next = t.total;
  } else {      // the table's order, except that the head stacks lie head by head: k, v, q of head 0, of head 1, ...
    for (const TailParam* r = t.p; r != end; ++r) if (!r->attn) tail_grad(o, *r) = take(r->len);
    for (int h = 0; h < MLHOT_HEADS; ++h)
      for (const TailParam* r = t.p; r != end; ++r) if (r->heads > 1) tail_grad(o, *r, h) = take(r->len);
    for (const TailParam* r = t.p; r != end; ++r) if (r->attn && r->heads == 1) tail_grad(o, *r) = take(r->len);
  }
  if (d.agg_mode == MLHOT_AGG_BACO) {
    o.mu_w = take((size_t)d.dim_r * d.dim_r); o.mu_b = take(d.dim_r); o.var_w = take((size_t)d.dim_r * d.dim_r); o.var_b = take(d.dim_r);
  }
  o.enc.w1 = take(32 * 9); o.enc.b1 = take(32); o.enc.w2 = take(48 * 288); o.enc.b2 = take(48);
  o.enc.w3 = take(64 * 432); o.enc.b3 = take(64); o.enc.wl = take((size_t)dw * 4096); o.enc.bl = take(dw);
  return next;
}

inline int np_forward(const mlhot_np_dims& d, const mlhot_np_params& p, const float* ctx_x, const float* ctx_y,
                      const float* qry_x, float* mu, void* saved, void* scratch, size_t scratch_bytes, hipStream_t s,
                      const Stage& st = Stage{}) {
  MLHOT_TRY(np_check_dims(d));
  MLHOT_TRY(stage_check(st, "np_vanilla_fwd"));
  NpBuf b = np_saved_carve(d, saved, (size_t)-1 / 2);
  const NpRoute rt = np_route(d);
  NpScratch sc = np_scratch_carve(d, rt, scratch, scratch_bytes);
  if (!sc.ok) { set_error("np_vanilla_fwd: scratch too small (%zu < %zu)", scratch_bytes, sc.bytes); return MLHOT_ERR_WORKSPACE; }
  const int Rc = d.T * d.Nc, Rq = d.T * d.Nq, dw = d.dim_w, H = MLHOT_HEADS;
  const int ldc = dw + dw / 4, ldd = dw + d.dim_z;

  // E1 on [context | target] images in one pass; rows land in cat_in / dec_in
  if (st.staged() && rt.family != Tail::Attention) {      // the staged pass is built on the fused attention tail's launch boundaries
    set_error("np_vanilla_fwd: staged passes need the fused attention tail (attention aggregation, Nc, Nq <= 16, option tail_fused)");
    return MLHOT_ERR_UNSUPPORTED;
  }
  EncXFold xf{nullptr, nullptr, 0, 0};
  if (st.first()) MLHOT_TRY(enc_forward(ctx_x, Rc, qry_x, Rq, p.enc, dw, Rows2{b.cat_in, ldc, Rc, b.dec_in, ldd}, b.enc, sc.enc, sc.enc_bytes, s,
                                        rt.enc_fold ? &xf : nullptr));
#ifndef MLHOT_HOSTSIM
  if (rt.family == Tail::Attention) return tail_forward_fused(d, p, rt, ctx_y, mu, b, sc, s, st, xf);
  if (rt.family == Tail::Cnp) return cnp_forward_fused(d, p, rt, ctx_y, mu, b, s, xf);
#endif


  if (d.Nc > 0) {
    MLHOT_TRY(lin_fwd(ctx_y, d.label_dim, wb1(p.ty_w, p.ty_b, dw / 4), b.cat_in + dw, ldc, Rc, d.label_dim, dw / 4, ACT_NONE, s, "np.transform_y"));
    const float* x = b.cat_in; int ldx = ldc, kin = ldc;
    for (int i = 0; i < d.n_hidden; ++i) {
      MLHOT_TRY(lin_fwd(x, ldx, wb1(p.er_w[i], p.er_b[i], d.hidden[i]), b.h[i], d.hidden[i], Rc, kin, d.hidden[i], ACT_RELU, s, "np.encoder_r"));
      x = b.h[i]; ldx = kin = d.hidden[i];
    }
    MLHOT_TRY(lin_fwd(x, ldx, wb1(p.er_w[d.n_hidden], p.er_b[d.n_hidden], d.dim_r), b.rs, d.dim_r, Rc, kin, d.dim_r, ACT_NONE, s, "np.encoder_r.out"));

    if (d.agg_mode == MLHOT_AGG_ATTENTION) {
      MLHOT_TRY(lin_fwd(b.cat_in, ldc, wb8(p.wk_w, p.wk_b, dw), b.kh, H * dw, Rc, dw, H * dw, ACT_NONE, s, "np.W_k"));
      MLHOT_TRY(lin_fwd(b.rs, d.dim_r, wb8(p.wv_w, p.wv_b, dw), b.vh, H * dw, Rc, dw, H * dw, ACT_NONE, s, "np.W_v"));
      MLHOT_TRY(lin_fwd(b.dec_in, ldd, wb8(p.wq_w, p.wq_b, dw), b.qh, H * dw, Rq, dw, H * dw, ACT_NONE, s, "np.W_q"));
      FavorDims f{d.T, H, d.Nq, d.Nc, dw, d.m_feat};
      MLHOT_TRY(favor_fwd_any(f, b.qh, b.kh, b.vh, p.proj, b.merged, b.favor, b.favor_bytes, s));
      MLHOT_TRY(lin_fwd(b.merged, H * dw, wb1(p.wo_w, p.wo_b, dw), b.rr, dw, Rq, H * dw, dw, ACT_NONE, s, "np.W"));
      MLHOT_TRY(lin_fwd(b.rr, dw, wb1(p.r2z_w, p.r2z_b, d.dim_z), b.dec_in + dw, ldd, Rq, d.dim_r, d.dim_z, ACT_NONE, s, "np.r_to_z"));
    } else {
      const float* src = b.rs;
      if (d.agg_mode == MLHOT_AGG_BACO) {
        MLHOT_TRY(lin_fwd(b.rs, d.dim_r, wb1(p.mu_w, p.mu_b, d.dim_r), b.mu_l, d.dim_r, Rc, d.dim_r, d.dim_r, ACT_NONE, s, "np.rs_to_mu"));
        MLHOT_TRY(lin_fwd(b.rs, d.dim_r, wb1(p.var_w, p.var_b, d.dim_r), b.lv, d.dim_r, Rc, d.dim_r, d.dim_r, ACT_NONE, s, "np.rs_to_var"));
        src = b.mu_l;
      }
      MLHOT_TRY(run_foreach(AggFwd{d.agg_mode, d.Nc, d.dim_r, src, b.lv, b.r, b.sigma, b.amax}, (size_t)d.T * d.dim_r, s, "np.agg"));
      MLHOT_TRY(lin_fwd(b.r, d.dim_r, wb1(p.r2z_w, p.r2z_b, d.dim_z), b.zt, d.dim_z, d.T, d.dim_r, d.dim_z, ACT_NONE, s, "np.r_to_z"));
      MLHOT_TRY(run_foreach(BcastRows{b.zt, d.dim_z, d.Nq, b.dec_in + dw, ldd}, (size_t)Rq * d.dim_z, s, "np.bcast_z"));
    }
  } else {
    MLHOT_TRY(run_foreach(Fill2D{b.dec_in + dw, ldd, d.dim_z, 0.f}, (size_t)Rq * d.dim_z, s, "np.zero_z"));
  }
  MLHOT_TRY(lin_fwd(b.dec_in, ldd, wb1(p.dec_w[0], p.dec_b[0], d.dec_hidden), b.d1, d.dec_hidden, Rq, ldd, d.dec_hidden, ACT_RELU, s, "np.decoder0.0"));
  MLHOT_TRY(lin_fwd(b.d1, d.dec_hidden, wb1(p.dec_w[1], p.dec_b[1], d.dec_hidden), b.d2, d.dec_hidden, Rq, d.dec_hidden, d.dec_hidden, ACT_RELU, s, "np.decoder0.2"));
  MLHOT_TRY(lin_fwd(b.d2, d.dec_hidden, wb1(p.dec_w[2], p.dec_b[2], d.y_dim), mu, d.y_dim, Rq, d.dec_hidden, d.y_dim,
                    d.out_tanh ? ACT_TANH : ACT_NONE, s, "np.decoder0.4"));
  return MLHOT_OK;
}

inline int np_backward(const mlhot_np_dims& d, const mlhot_np_params& p, const float* ctx_x, const float* ctx_y,
                       const float* qry_x, const float* mu, const float* dmu, const mlhot_np_grads& g,
                       const void* saved, void* scratch, size_t scratch_bytes, hipStream_t s, const Stage& st = Stage{},
                       const LossDesc* loss = nullptr) {
  MLHOT_TRY(np_check_dims(d));
  MLHOT_TRY(stage_check(st, "np_vanilla_bwd"));
  NpBuf b = np_saved_carve(d, (void*)saved, (size_t)-1 / 2);
  const NpRoute rt = np_route(d);
  NpScratch sc = np_scratch_carve(d, rt, scratch, scratch_bytes);
  if (!sc.ok) { set_error("np_vanilla_bwd: scratch too small (%zu < %zu)", scratch_bytes, sc.bytes); return MLHOT_ERR_WORKSPACE; }
  const int Rc = d.T * d.Nc, Rq = d.T * d.Nq, dw = d.dim_w, H = MLHOT_HEADS, dh = d.dec_hidden;
  const int ldc = dw + dw / 4, ldd = dw + d.dim_z;
  const int out_act = d.out_tanh ? ACT_TANH : ACT_NONE;

  // The loss's gradient, when the caller left it to this call (mlhot_np_vanilla_bwd_loss): the specialised phase C' derives it in
  // its prologue; every other first kernel gets it materialised (dmu_tmp = dmu + d loss / d mu, one launch as mlhot_loss_bwd's).
  LossDesc in_kernel{-1, nullptr, 0, nullptr, nullptr};
  if (loss != nullptr) {
    if (st.staged()) { set_error("np_vanilla_bwd: the staged pass takes dmu, not a loss descriptor"); return MLHOT_ERR_UNSUPPORTED; }
    if (rt.loss_in_kernel) in_kernel = *loss;
    if (in_kernel.kind < 0) {
      // (the loss VALUE, when the caller left that to this call as well: the launch mlhot_loss_fwd would have made)
      if (loss->value != nullptr) MLHOT_TRY(run_reduce1(LossRed{loss->kind, d.y_dim, loss->gt_dim, Rq, mu, loss->gt, loss->value}, Rq, s, "loss_fwd"));
      MLHOT_TRY(run_foreach(LossBwd{loss->kind, d.y_dim, loss->gt_dim, Rq, mu, loss->gt, loss->dloss, sc.dmu_tmp, dmu}, (size_t)Rq, s, "loss_bwd"));
      dmu = sc.dmu_tmp;
    }
  } else if (dmu == nullptr) { set_error("np_vanilla_bwd: null dmu"); return MLHOT_ERR_ARG; }
  if (st.staged() && rt.family != Tail::Attention) {
    set_error("np_vanilla_bwd: staged passes need the fused attention tail (attention aggregation, Nc, Nq <= 16, option tail_fused)");
    return MLHOT_ERR_UNSUPPORTED;
  }
#ifndef MLHOT_HOSTSIM
  if (rt.family != Tail::Generic) {
    PendingSum tail_sum{};       // the tail's per-task slabs: summed by the encoder backward's final reduce launch when contiguous
    if (rt.family == Tail::Attention) MLHOT_TRY(tail_backward_fused(d, p, rt, ctx_y, mu, dmu, g, b, sc, s, &tail_sum, st, in_kernel));
    else MLHOT_TRY(cnp_backward_fused(d, p, rt, ctx_y, mu, dmu, g, b, sc, s, &tail_sum, in_kernel));
    if (st.stage == 0) return MLHOT_OK;
    return enc_backward(ctx_x, Rc, qry_x, Rq, p.enc, dw, Rows2{sc.d_cat_in, ldc, Rc, sc.d_dec_in, ldd}, b.enc, g.enc, sc.enc, sc.enc_bytes, s,
                        &tail_sum);
  }
#endif
  // decoder0
  MLHOT_TRY(lin_wgrad(dmu, d.y_dim, mu, d.y_dim, out_act, b.d2, dh, gb1(g.dec_w[2], g.dec_b[2], d.y_dim), Rq, dh, d.y_dim, s, "np.bwd.dec4.w"));
  MLHOT_TRY(lin_dgrad(dmu, d.y_dim, mu, d.y_dim, out_act, wb1(p.dec_w[2], nullptr, d.y_dim), sc.dd2, dh, 0, Rq, dh, d.y_dim, s, "np.bwd.dec4.x"));
  MLHOT_TRY(lin_wgrad(sc.dd2, dh, b.d2, dh, ACT_RELU, b.d1, dh, gb1(g.dec_w[1], g.dec_b[1], dh), Rq, dh, dh, s, "np.bwd.dec2.w"));
  MLHOT_TRY(lin_dgrad(sc.dd2, dh, b.d2, dh, ACT_RELU, wb1(p.dec_w[1], nullptr, dh), sc.dd1, dh, 0, Rq, dh, dh, s, "np.bwd.dec2.x"));
  MLHOT_TRY(lin_wgrad(sc.dd1, dh, b.d1, dh, ACT_RELU, b.dec_in, ldd, gb1(g.dec_w[0], g.dec_b[0], dh), Rq, ldd, dh, s, "np.bwd.dec0.w"));
  MLHOT_TRY(lin_dgrad(sc.dd1, dh, b.d1, dh, ACT_RELU, wb1(p.dec_w[0], nullptr, dh), sc.d_dec_in, ldd, 0, Rq, ldd, dh, s, "np.bwd.dec0.x"));

  if (d.Nc > 0) {
    const float* dz = sc.d_dec_in + dw;   // [Rq][dim_z], ld = ldd
    if (d.agg_mode == MLHOT_AGG_ATTENTION) {
      MLHOT_TRY(lin_wgrad(dz, ldd, nullptr, 0, ACT_NONE, b.rr, dw, gb1(g.r2z_w, g.r2z_b, d.dim_z), Rq, d.dim_r, d.dim_z, s, "np.bwd.r2z.w"));
      MLHOT_TRY(lin_dgrad(dz, ldd, nullptr, 0, ACT_NONE, wb1(p.r2z_w, nullptr, d.dim_z), sc.d_rr, dw, 0, Rq, d.dim_r, d.dim_z, s, "np.bwd.r2z.x"));
      MLHOT_TRY(lin_wgrad(sc.d_rr, dw, nullptr, 0, ACT_NONE, b.merged, H * dw, gb1(g.wo_w, g.wo_b, dw), Rq, H * dw, dw, s, "np.bwd.W.w"));
      MLHOT_TRY(lin_dgrad(sc.d_rr, dw, nullptr, 0, ACT_NONE, wb1(p.wo_w, nullptr, dw), sc.d_merged, H * dw, 0, Rq, H * dw, dw, s, "np.bwd.W.x"));
      FavorDims f{d.T, H, d.Nq, d.Nc, dw, d.m_feat};
      MLHOT_TRY(favor_bwd_any(f, b.qh, b.kh, b.vh, p.proj, b.merged, sc.d_merged, sc.dqh, sc.dkh, sc.dvh, b.favor, b.favor_bytes, s));
      // Q projection: x_qry gradient accumulates onto the decoder's
      MLHOT_TRY(lin_wgrad(sc.dqh, H * dw, nullptr, 0, ACT_NONE, b.dec_in, ldd, gb8(g.wq_w, g.wq_b, dw), Rq, dw, H * dw, s, "np.bwd.W_q.w"));
      MLHOT_TRY(lin_dgrad(sc.dqh, H * dw, nullptr, 0, ACT_NONE, wb8(p.wq_w, nullptr, dw), sc.d_dec_in, ldd, 1, Rq, dw, H * dw, s, "np.bwd.W_q.x"));
      MLHOT_TRY(lin_wgrad(sc.dvh, H * dw, nullptr, 0, ACT_NONE, b.rs, d.dim_r, gb8(g.wv_w, g.wv_b, dw), Rc, dw, H * dw, s, "np.bwd.W_v.w"));
      MLHOT_TRY(lin_dgrad(sc.dvh, H * dw, nullptr, 0, ACT_NONE, wb8(p.wv_w, nullptr, dw), sc.d_rs, d.dim_r, 0, Rc, dw, H * dw, s, "np.bwd.W_v.x"));
      MLHOT_TRY(lin_wgrad(sc.dkh, H * dw, nullptr, 0, ACT_NONE, b.cat_in, ldc, gb8(g.wk_w, g.wk_b, dw), Rc, dw, H * dw, s, "np.bwd.W_k.w"));
    } else {
      MLHOT_TRY(run_foreach(BcastRowsBwd{dz, ldd, d.dim_z, d.Nq, sc.dzt}, (size_t)d.T * d.dim_z, s, "np.bwd.bcast_z"));
      MLHOT_TRY(lin_wgrad(sc.dzt, d.dim_z, nullptr, 0, ACT_NONE, b.r, d.dim_r, gb1(g.r2z_w, g.r2z_b, d.dim_z), d.T, d.dim_r, d.dim_z, s, "np.bwd.r2z.w"));
      MLHOT_TRY(lin_dgrad(sc.dzt, d.dim_z, nullptr, 0, ACT_NONE, wb1(p.r2z_w, nullptr, d.dim_z), sc.dr, d.dim_r, 0, d.T, d.dim_r, d.dim_z, s, "np.bwd.r2z.x"));
      if (d.agg_mode == MLHOT_AGG_BACO) {
        MLHOT_TRY(run_foreach(AggBwd{d.agg_mode, d.Nc, d.dim_r, b.mu_l, b.lv, b.r, b.sigma, b.amax, sc.dr, sc.d_mu_l, sc.d_lv},
                              (size_t)d.T * d.dim_r, s, "np.bwd.agg"));
        MLHOT_TRY(lin_wgrad(sc.d_mu_l, d.dim_r, nullptr, 0, ACT_NONE, b.rs, d.dim_r, gb1(g.mu_w, g.mu_b, d.dim_r), Rc, d.dim_r, d.dim_r, s, "np.bwd.rs_to_mu.w"));
        MLHOT_TRY(lin_dgrad(sc.d_mu_l, d.dim_r, nullptr, 0, ACT_NONE, wb1(p.mu_w, nullptr, d.dim_r), sc.d_rs, d.dim_r, 0, Rc, d.dim_r, d.dim_r, s, "np.bwd.rs_to_mu.x"));
        MLHOT_TRY(lin_wgrad(sc.d_lv, d.dim_r, nullptr, 0, ACT_NONE, b.rs, d.dim_r, gb1(g.var_w, g.var_b, d.dim_r), Rc, d.dim_r, d.dim_r, s, "np.bwd.rs_to_var.w"));
        MLHOT_TRY(lin_dgrad(sc.d_lv, d.dim_r, nullptr, 0, ACT_NONE, wb1(p.var_w, nullptr, d.dim_r), sc.d_rs, d.dim_r, 1, Rc, d.dim_r, d.dim_r, s, "np.bwd.rs_to_var.x"));
      } else {
        MLHOT_TRY(run_foreach(AggBwd{d.agg_mode, d.Nc, d.dim_r, b.rs, nullptr, b.r, b.sigma, b.amax, sc.dr, sc.d_rs, nullptr},
                              (size_t)d.T * d.dim_r, s, "np.bwd.agg"));
      }
    }
    // EncoderFC, last layer first
    const float* dy = sc.d_rs; int lddy = d.dim_r, nout = d.dim_r, act = ACT_NONE; const float* yv = nullptr; int ldy = 0;
    for (int i = d.n_hidden; i >= 0; --i) {
      const float* x = i > 0 ? b.h[i - 1] : b.cat_in;
      const int kin = i > 0 ? d.hidden[i - 1] : ldc, ldx = kin;
      float* dx = i > 0 ? sc.dh[i - 1] : sc.d_cat_in;
      MLHOT_TRY(lin_wgrad(dy, lddy, yv, ldy, act, x, ldx, gb1(g.er_w[i], g.er_b[i], nout), Rc, kin, nout, s, "np.bwd.encoder_r.w"));
      MLHOT_TRY(lin_dgrad(dy, lddy, yv, ldy, act, wb1(p.er_w[i], nullptr, nout), dx, kin, 0, Rc, kin, nout, s, "np.bwd.encoder_r.x"));
      if (i > 0) { dy = dx; lddy = kin; nout = kin; act = ACT_RELU; yv = b.h[i - 1]; ldy = kin; }
    }
    if (d.agg_mode == MLHOT_AGG_ATTENTION)   // K projection: second consumer of x_ctx
      MLHOT_TRY(lin_dgrad(sc.dkh, H * dw, nullptr, 0, ACT_NONE, wb8(p.wk_w, nullptr, dw), sc.d_cat_in, ldc, 1, Rc, dw, H * dw, s, "np.bwd.W_k.x"));
    MLHOT_TRY(lin_wgrad(sc.d_cat_in + dw, ldc, nullptr, 0, ACT_NONE, ctx_y, d.label_dim, gb1(g.ty_w, g.ty_b, dw / 4), Rc, d.label_dim, dw / 4, s, "np.bwd.transform_y.w"));
  }
  MLHOT_TRY(enc_backward(ctx_x, Rc, qry_x, Rq, p.enc, dw, Rows2{sc.d_cat_in, ldc, Rc, sc.d_dec_in, ldd}, b.enc, g.enc, sc.enc, sc.enc_bytes, s));
  return MLHOT_OK;
}

}  // namespace mlhot
