// E1: the vanilla image encoder (conv-conv-pool-conv-linear), forward and backward.
// Activations stay NCHW fp32 in HBM; what the backward needs is kept in `saved`:
//   a1  [n][32][64][64]  conv1 output (post-ReLU)          512 KiB / image
//   p2  [n][48][16][16]  pooled conv2 output (post-ReLU)    48 KiB / image
//   am2 [n][48][16][16]  pool arg-max (uint8)               12 KiB / image
//   a3  [n][4096]        conv3 output (post-ReLU, C-major flatten = nn.Flatten order)
// conv2's 192 KiB/image pre-pool map is scratch: ReLU and pool commute, so the pooled value
// and the arg-max are all the backward needs (DyPooled in problems.h).
#pragma once
#include "common.h"
#include "options.h"
#include "foreach.h"
#include "igemm.h"
#include "ops_direct.h"
#include "problems.h"
#include "conv_tc.h"
#include "conv_split.h"
#include "conv3_tc.h"
#include "enc_linear.h"
#include "../../include/mlhot.h"

namespace mlhot {

struct EncSaved {
  float* a1; float* p2; uint8_t* am2; float* a3; unsigned* m1; bool ok; size_t bytes;
};
inline EncSaved enc_saved_carve(int n, void* base, size_t cap) {
  Arena a(base, cap);
  EncSaved s;
  s.a1 = a.take<float>((size_t)n * 32 * 64 * 64);
  s.p2 = a.take<float>((size_t)n * 48 * 16 * 16);
  s.am2 = a.take<uint8_t>((size_t)n * 48 * 16 * 16);
  s.a3 = a.take<float>((size_t)n * 4096);
  s.m1 = a.take<unsigned>((size_t)n * 64 * 64 + 16);     // conv1 ReLU bits (16-dword records per 16 columns + one junk record, conv_tc.h m1_record), written by the fused forward
  s.ok = a.ok; s.bytes = a.off + 256;
  return s;
}
inline size_t enc_saved_bytes(int n) { return enc_saved_carve(n, nullptr, 0).bytes; }

// split-K factors (bounded so the slabs stay a few MB and every launch has >= ~256 workgroups)
inline int enc_lin_split(int n) { (void)n; return 32; }
inline int enc_linw_split(int n) { return n >= 64 ? 4 : 1; }
inline int conv3w_split(int n) { int s = n / 4; return s < 1 ? 1 : (s > 128 ? 128 : s); }
inline int conv2w_split(int n) { int s = n / 2; return s < 1 ? 1 : (s > 240 ? 240 : s); }
inline int conv1w_split(int n) { int s = n * 2; return s > 1024 ? 1024 : s; }

// ---- the route: which kernels run for n images of width dim_w under the current options ------------------------------------------
// enc_route() is the ONE place that reads the options conv2_tc / conv2_split / conv3_bwd_merged / materialize_a1 / dbg for the
// encoder; enc_forward, enc_backward, the conv12 block's entries (mlhot.hip) and np_route() (np_vanilla.h) take its answer.
// DESIGN.md "The encoder's route" lists the launches of every route.
constexpr int C2_GRID = 256;   // one persistent workgroup per CU
struct EncRoute {
  bool ws;          // the weight-stationary kernels (conv_tc.h, conv3_tc.h; conv_split.h by `split`) | false: the generic implicit-GEMM
                    // chain, the A/B reference (and all the host simulation has)
  bool own_linear;  // ws and dim_w == el::DW: enc_linear.h's Linear.  ws with another width is the one mixed route: the generic Linear
                    // between the weight-stationary convolutions
  int split;        // option conv2_split (read where conv12 runs): bit 1 forward, 2 data gradient, 4 weight gradient on the bf16 pipe
  int conv3_nw;     // conv3 backward: 0 = weight and data gradient as two launches; else ONE launch of C2_GRID workgroups, the first
                    // conv3_nw of them the weight gradient (only when the batch fills the grid: n >= C2_GRID)
  bool keep_a1;     // ws: also store conv1's output (option materialize_a1; the fused kernels never need it, tests read it)
  int dbg;          // option dbg, handed to the kernels that take it
};
inline EncRoute enc_route(int n, int dim_w) {
  EncRoute r{};
#ifndef MLHOT_HOSTSIM
  r.ws = g_opt.conv2_tc != 0;
  r.own_linear = r.ws && dim_w == el::DW;
  r.split = g_opt.conv2_split;
  const int m = g_opt.conv3_bwd_merged;
  if (r.ws && m && n >= C2_GRID) r.conv3_nw = m > 1 && m < C2_GRID ? m : C2_GRID / 2;
  r.keep_a1 = r.ws && g_opt.materialize_a1;
  r.dbg = g_opt.dbg;
#else
  (void)n; (void)dim_w;
#endif
  return r;
}

// ---- the weight-stationary backward's slabs: one row per workgroup, all rows alive until the single deferred reduce ------------
//   conv3 rows [dW3 64 x 432 | db3 64], conv2 rows [dW2 48 x 288 | db2 48] (both weight blocks in their kernel's accumulator order,
//   un-permuted by the fold: c2::SumParts kind 2 / 1), conv1 rows [dW1 288 | db1 32].  When the caller's gradient tensors are adjacent
//   in that order (mlhot_np_grads_flat_layout) a row reduces as one segment.
// enc_slab_floats, enc_backward_ws, mlhot_conv12_bwd and mlhot_conv12_scratch_bytes all place and size by this carve.
constexpr int C3_L = 64 * 432, C3_R = C3_L + 64, C12_L2 = 48 * 288, C12_R2 = C12_L2 + 48, C1_R = 320;
struct EncBwdSlabs { float *c3, *c2, *c1; size_t floats; };
// `rows`: the rows reserved per layer (the encoder: C2_GRID whatever n; the conv12 block on its own: its grid, and no conv3 region)
inline EncBwdSlabs enc_bwd_slabs(float* base, int rows = C2_GRID, bool conv3 = true) {
  const size_t o2 = conv3 ? (size_t)rows * C3_R : 0, o1 = o2 + (size_t)rows * C12_R2;
  return EncBwdSlabs{base, base ? base + o2 : nullptr, base ? base + o1 : nullptr, o1 + (size_t)rows * C1_R};
}
inline int conv12_grid(int n) { return n * 8 < C2_GRID ? n * 8 : C2_GRID; }
// Behind the rows: 2 x C2_GRID x 48 x 288 floats that no kernel uses (left from an earlier conv2 slab layout).  Kept so that every
// reported scratch size stays what callers have allocated against; shrinking it is a change of its own.
constexpr size_t ENC_SLAB_RESERVE = (size_t)2 * C2_GRID * 48 * 288;

struct EncScratch {
  float* a2;      // fwd: [n][48][32][32]
  float* slab;    // split-K partials (fwd linear, bwd wgrads)
  float* dy3;     // bwd: [n][4096]
  float* dp2;     // bwd: [n][48][16][16]
  float* dy1;     // bwd: [n][32][64][64]
  bool ok; size_t bytes;
};
inline size_t enc_slab_floats(int n, int dim_w) {
  size_t m = (size_t)enc_lin_split(n) * n * dim_w;
  size_t v;
  v = (size_t)enc_linw_split(n) * dim_w * 4097; if (v > m) m = v;
  v = (size_t)conv3w_split(n) * 64 * 433;       if (v > m) m = v;
  v = (size_t)conv2w_split(n) * 48 * 289;       if (v > m) m = v;
  v = (size_t)conv1w_split(n) * 32 * 10;        if (v > m) m = v;
  v = enc_bwd_slabs(nullptr).floats + ENC_SLAB_RESERVE;     if (v > m) m = v;
  return m;
}
inline EncScratch enc_scratch_carve(int n, int dim_w, void* base, size_t cap) {
  Arena a(base, cap);
  EncScratch s;
  s.slab = a.take<float>(enc_slab_floats(n, dim_w));
  // forward and backward never run concurrently on one scratch: a2 aliases the backward buffers
  const size_t mark = a.off;
  s.a2 = a.take<float>((size_t)n * 48 * 32 * 32);
  const size_t fwd_end = a.off;
  a.off = mark;
  s.dy3 = a.take<float>((size_t)n * 4096);
  s.dp2 = a.take<float>((size_t)n * 48 * 16 * 16);
  s.dy1 = a.take<float>((size_t)n * 32 * 64 * 64);
  if (fwd_end > a.off) a.off = fwd_end;
  s.ok = a.ok; s.bytes = a.off + 256;
  return s;
}
inline size_t enc_scratch_bytes(int n, int dim_w) { return enc_scratch_carve(n, dim_w, nullptr, 0).bytes; }

// One call's operands, carved: what every function below works on.
struct EncCall {
  const float* img0; int n0; const float* img1; int n1;
  const mlhot_enc_params& p; int dim_w;
  EncSaved sv; EncScratch sc; hipStream_t s;
  int n() const { return n0 + n1; }
  Src2 x() const { return Src2{img0, n0, img1, (size_t)128 * 128}; }
};
inline int enc_scratch_short(const char* who, size_t have, size_t need) {
  set_error("%s: scratch too small (%zu < %zu)", who, have, need);
  return MLHOT_ERR_WORKSPACE;
}

// `xfold`: the caller's first kernel folds the Linear's split-K partial results itself (the fused attention tail's phase A reads the
// feature tiles anyway: one launch and its ~4.7 us off the forward's critical path).  On return xfold->slab / bias / k / n describe
// the partial results [k][n][dim_w] - or slab == nullptr when this path wrote `feat` itself (generic Linear, other widths).
struct EncXFold { const float* slab; const float* bias; int k, n; };
// A slab sum that has not been launched yet: out[e] = sum over parts p < nparts of slab[p * stride + e], e < len.
struct PendingSum { const float* slab; float* out; int nparts, len, stride; };

// ---- the generic chain (both builds) ---------------------------------------------------------------------------------------------
inline int enc_linear_forward_generic(const EncCall& c, Rows2 feat) {
  EncLinFwd lf{c.n(), c.dim_w, 4096, c.sv.a3, c.p.wl, c.p.bl, feat};
  return run_igemm<EncLinFwd, 64, 64, 16, 2, 2>(lf, enc_lin_split(c.n()), c.sc.slab, c.s, "enc.linear");
}
inline int enc_forward_generic(const EncCall& c, Rows2 feat) {
  const int n = c.n();
  const mlhot_enc_params& p = c.p;
  MLHOT_TRY(run_foreach(Conv1Fwd<Src2>{c.x(), p.w1, p.b1, c.sv.a1}, (size_t)n * 4096, c.s, "enc.conv1"));
  typedef ConvFwd<32, 64, 64, 48, Src1> C2;
  C2 c2{n * 1024, 48, 288, Src1{c.sv.a1, (size_t)32 * 4096}, p.w2, p.b2, c.sc.a2};
  MLHOT_TRY((run_igemm<C2, 128, 48, 16, 4, 1>(c2, 1, nullptr, c.s, "enc.conv2")));
  MLHOT_TRY(run_foreach(Pool2Fwd{c.sc.a2, c.sv.p2, c.sv.am2, 32, 32}, (size_t)n * 48 * 256, c.s, "enc.pool"));
  typedef ConvFwd<48, 16, 16, 64, Src1> C3;
  C3 c3{n * 64, 64, 432, Src1{c.sv.p2, (size_t)48 * 256}, p.w3, p.b3, c.sv.a3};
  MLHOT_TRY((run_igemm<C3, 64, 64, 16, 2, 2>(c3, 1, nullptr, c.s, "enc.conv3")));
  return enc_linear_forward_generic(c, feat);
}

template <int PY, int PX>
inline int enc_conv3_dgrad(int n, const float* dy3, const float* w3, float* dp2, hipStream_t s) {
  typedef DyPlain<64, 8, 8> DY;
  typedef ConvDgrad<48, 16, 16, 64, PY, PX, DY> P;
  P p{n * 64, 48, P::NTY * P::NTX * 64, DY{dy3}, w3, nullptr, dp2};
  return run_igemm<P, 64, 48, 16, 4, 1>(p, 1, nullptr, s, "enc.bwd.conv3.dgrad");
}
template <int PY, int PX>
inline int enc_conv2_dgrad(int n, const DyPooled<48, 32, 32>& dy, const float* w2, const float* a1, float* dy1, hipStream_t s) {
  typedef ConvDgrad<32, 64, 64, 48, PY, PX, DyPooled<48, 32, 32>> P;
  P p{n * 1024, 32, P::NTY * P::NTX * 48, dy, w2, a1, dy1};
  return run_igemm<P, 128, 32, 16, 4, 1>(p, 1, nullptr, s, "enc.bwd.conv2.dgrad");
}
// Linear(4096 -> dim_w): input gradient (masked by conv3's ReLU), weight + bias gradient
inline int enc_linear_backward_generic(const EncCall& c, Rows2 dfeat, const mlhot_enc_grads& g) {
  const int n = c.n();
  EncLinDgrad ld{n, 4096, c.dim_w, dfeat, c.p.wl, c.sv.a3, c.sc.dy3};
  MLHOT_TRY((run_igemm<EncLinDgrad, 64, 64, 16, 2, 2>(ld, 1, nullptr, c.s, "enc.bwd.linear.dgrad")));
  EncLinWgrad lw{c.dim_w, 4097, n, dfeat, c.sv.a3, g.wl, g.bl};
  return run_igemm<EncLinWgrad, 64, 64, 16, 2, 2>(lw, enc_linw_split(n), c.sc.slab, c.s, "enc.bwd.linear.wgrad");
}
inline int enc_backward_generic(const EncCall& c, Rows2 dfeat, const mlhot_enc_grads& g) {
  const int n = c.n();
  const mlhot_enc_params& p = c.p;
  const EncSaved& sv = c.sv;
  const EncScratch& sc = c.sc;
  hipStream_t s = c.s;
  MLHOT_TRY(enc_linear_backward_generic(c, dfeat, g));
  // conv3
  typedef ConvWgrad<48, 16, 16, 64, DyPlain<64, 8, 8>, Src1> W3;
  W3 w3{64, 433, n * 64, DyPlain<64, 8, 8>{sc.dy3}, Src1{sv.p2, (size_t)48 * 256}, g.w3, g.b3};
  MLHOT_TRY((run_igemm<W3, 64, 64, 16, 2, 2>(w3, conv3w_split(n), sc.slab, s, "enc.bwd.conv3.wgrad")));
  MLHOT_TRY((enc_conv3_dgrad<0, 0>(n, sc.dy3, p.w3, sc.dp2, s)));
  MLHOT_TRY((enc_conv3_dgrad<0, 1>(n, sc.dy3, p.w3, sc.dp2, s)));
  MLHOT_TRY((enc_conv3_dgrad<1, 0>(n, sc.dy3, p.w3, sc.dp2, s)));
  MLHOT_TRY((enc_conv3_dgrad<1, 1>(n, sc.dy3, p.w3, sc.dp2, s)));
  // conv2 (pool + ReLU backward are folded into the dY gather)
  const DyPooled<48, 32, 32> dy2{sc.dp2, sv.p2, sv.am2};
  typedef ConvWgrad<32, 64, 64, 48, DyPooled<48, 32, 32>, Src1> W2;
  W2 w2{48, 289, n * 1024, dy2, Src1{sv.a1, (size_t)32 * 4096}, g.w2, g.b2};
  MLHOT_TRY((run_igemm<W2, 48, 64, 16, 1, 4>(w2, conv2w_split(n), sc.slab, s, "enc.bwd.conv2.wgrad")));
  MLHOT_TRY((enc_conv2_dgrad<0, 0>(n, dy2, p.w2, sv.a1, sc.dy1, s)));
  MLHOT_TRY((enc_conv2_dgrad<0, 1>(n, dy2, p.w2, sv.a1, sc.dy1, s)));
  MLHOT_TRY((enc_conv2_dgrad<1, 0>(n, dy2, p.w2, sv.a1, sc.dy1, s)));
  MLHOT_TRY((enc_conv2_dgrad<1, 1>(n, dy2, p.w2, sv.a1, sc.dy1, s)));
  // conv1 (no input gradient: images are leaves)
  typedef ConvWgrad<1, 128, 128, 32, DyPlain<32, 64, 64>, Src2> W1;
  W1 w1{32, 10, n * 4096, DyPlain<32, 64, 64>{sc.dy1}, c.x(), g.w1, g.b1};
  return run_igemm<W1, 32, 16, 16, 2, 1>(w1, conv1w_split(n), sc.slab, s, "enc.bwd.conv1.wgrad");
}

#ifndef MLHOT_HOSTSIM
// ---- the weight-stationary family (GPU build only) ---------------------------------------------------------------------------------
template <class K, class... A>      // one launch under its profiler label
inline int ws_launch(const char* label, K kernel, int grid, int block, hipStream_t s, const A&... args) {
  {
    ProfScope ps(label, s);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, args...);
  }
  return check_launch(label);
}
// Slab sums parked for ONE launch (c2::sum_parts_multi_kernel): the backward's weight-gradient folds are deferred to its very end
// (4 kernels fewer on the step's critical path).  Fixed fold order, so the result does not depend on who launches it.
struct SlabFolds {
  c2::SumPartsMulti mp{};
  static constexpr int MAX = sizeof(mp.seg) / sizeof(mp.seg[0]);
  static_assert(sizeof(mp.first) / sizeof(mp.first[0]) == MAX + 1, "first[i] .. first[i + 1]: segment i's blocks");
  int pend(const float* slab, float* out, int nparts, int len, int stride, int kind = 0) {
    if (mp.n >= MAX) { set_error("slab folds: more than %d sums pending for one launch", MAX); return MLHOT_ERR_LAUNCH; }
    mp.seg[mp.n] = c2::SumParts{slab, out, nparts, len, stride, kind};
    mp.first[mp.n + 1] = mp.first[mp.n] + c2::sum_parts_blocks(len);
    ++mp.n;
    return MLHOT_OK;
  }
  int flush(hipStream_t s, const char* label) {
    if (mp.n == 0) return MLHOT_OK;
    const c2::SumPartsMulti now = mp;
    mp.n = 0;
    return ws_launch(label, c2::sum_parts_multi_kernel, now.first[now.n], 256, s, now);
  }
};

// conv1 + ReLU + conv2 + ReLU + 2x2 max-pool in one kernel (a1 is recomputed band by band in LDS and never stored): p2, the pool
// arg-max and conv1's ReLU sign bits land in `sv`.  r.split: bit 1 forward, bit 2 data gradient, bit 4 weight gradient run conv2 on
// the bf16 pipe over split operands (conv_split.h) - same inputs, same outputs' layout.
inline int conv12_forward(const c2::ImgSrc& xs, int n, const float* w1, const float* b1, const float* w2, const float* b2,
                          const EncSaved& sv, const EncRoute& r, hipStream_t s) {
  if (r.split & 1)
    return ws_launch("enc.conv12.split", c2s::conv12_fwd_split_kernel, n * 16 < C2_GRID ? n * 16 : C2_GRID, c2s::NT, s, xs, w1, b1, w2, b2, sv.p2, sv.am2, sv.m1, n);
  return ws_launch("enc.conv12", c2::conv12_fwd_pool_kernel, conv12_grid(n), c2::NT, s, xs, w1, b1, w2, b2, sv.p2, sv.am2, sv.m1, n, r.dbg);
}
// the block's two backward kernels: conv12_grid(n) rows of sl.c2 and of sl.c1 (the split kernels: the same rows), which the caller folds
inline int conv12_backward(const c2::ImgSrc& xs, int n, const float* w1, const float* b1, const float* w2, const float* dp2,
                           const EncSaved& sv, const EncBwdSlabs& sl, const EncRoute& r, hipStream_t s) {
  const int grid = conv12_grid(n);
  float *slab_w = sl.c2, *slab_b = sl.c2 + C12_L2;
  if (r.split & 4) MLHOT_TRY(ws_launch("enc.bwd.conv12.wgrad.split", c2s::conv12_wgrad_split_kernel, grid, c2s::NT, s, xs, w1, b1, dp2, sv.p2, sv.am2, slab_w, slab_b, n));
  else MLHOT_TRY(ws_launch("enc.bwd.conv12.wgrad", c2::conv12_wgrad_kernel, grid, c2::NT, s, xs, w1, b1, dp2, sv.p2, sv.am2, slab_w, slab_b, n, r.dbg));
  if (r.split & 2) return ws_launch("enc.bwd.conv12.dgrad.split", c2s::conv12_dgrad_split_kernel, grid, c2s::dg::NT2, s, xs, sv.m1, dp2, sv.p2, sv.am2, w2, sl.c1, n);
  return ws_launch("enc.bwd.conv12.dgrad", c2::conv12_dgrad_kernel, grid, c2::NT2, s, xs, sv.m1, dp2, sv.p2, sv.am2, w2, sl.c1, n);
}
// conv2's gradients out of the block's rows (conv1's: the callers differ)
inline int conv12_pend_conv2(const EncBwdSlabs& sl, int n, float* dw2, float* db2, SlabFolds& folds) {
  MLHOT_TRY(folds.pend(sl.c2, dw2, conv12_grid(n), C12_L2, C12_R2, 1));
  return folds.pend(sl.c2 + C12_L2, db2, conv12_grid(n), 48, C12_R2);
}

inline int enc_forward_ws(const EncCall& c, const EncRoute& r, Rows2 feat, EncXFold* xfold) {
  const int n = c.n();
  const mlhot_enc_params& p = c.p;
  if (r.keep_a1) MLHOT_TRY(run_foreach(Conv1Fwd<Src2>{c.x(), p.w1, p.b1, c.sv.a1}, (size_t)n * 4096, c.s, "enc.conv1.debug"));
  MLHOT_TRY(conv12_forward(c2::ImgSrc{c.img0, c.n0, c.img1}, n, p.w1, p.b1, p.w2, p.b2, c.sv, r, c.s));
  MLHOT_TRY(ws_launch("enc.conv3", c3::conv3_fwd_kernel, n * 2 < C2_GRID ? n * 2 : C2_GRID, c3::F_NT, c.s, c.sv.p2, p.w3, p.b3, c.sv.a3, n));
  if (!r.own_linear) return enc_linear_forward_generic(c, feat);      // the mixed route
  MLHOT_TRY(ws_launch("enc.linear", el::enc_linear_fwd_kernel, ((n + 15) / 16) * el::F_KS, 256, c.s, c.sv.a3, p.wl, c.sc.slab, n));
  if (xfold != nullptr) { *xfold = EncXFold{c.sc.slab, p.bl, el::F_KS, n}; return MLHOT_OK; }
  return ws_launch("slab_reduce", el::enc_linear_fold_kernel, (n * el::DW + 255) / 256, 256, c.s, c.sc.slab, p.bl, feat, n);
}

// `folds`: may hold the caller's pending sum already; everything is summed by ONE launch at the very end.
inline int enc_backward_ws(const EncCall& c, const EncRoute& r, Rows2 dfeat, const mlhot_enc_grads& g, SlabFolds& folds) {
  const int n = c.n();
  const mlhot_enc_params& p = c.p;
  const EncSaved& sv = c.sv;
  const EncScratch& sc = c.sc;
  const EncBwdSlabs sl = enc_bwd_slabs(sc.slab);
  if (r.own_linear) MLHOT_TRY(ws_launch("enc.bwd.linear", el::enc_linear_bwd_kernel, el::KIN / 16, el::NTH, c.s, dfeat, p.wl, sv.a3, sc.dy3, g.wl, g.bl, n));
  else MLHOT_TRY(enc_linear_backward_generic(c, dfeat, g));      // the mixed route (its split-K partials are summed before conv3 writes the slab)
  // conv3: as ONE launch the first conv3_nw workgroups take the weight gradient, the rest the data gradient (conv3_tc.h)
  const int grid = n < C2_GRID ? n : C2_GRID, rows3 = r.conv3_nw ? r.conv3_nw : grid;
  float *slab_w3 = sl.c3, *slab_b3 = sl.c3 + C3_L;
  if (r.conv3_nw) {
    MLHOT_TRY(ws_launch("enc.bwd.conv3", c3::conv3_bwd_kernel, C2_GRID, c3::W_NT, c.s, sv.p2, p.w3, sc.dy3, slab_w3, slab_b3, sc.dp2, n, r.conv3_nw));
  } else {
    MLHOT_TRY(ws_launch("enc.bwd.conv3.wgrad", c3::conv3_wgrad_kernel, grid, c3::W_NT, c.s, sv.p2, sc.dy3, slab_w3, slab_b3, n));
    MLHOT_TRY(ws_launch("enc.bwd.conv3.dgrad", c3::conv3_dgrad_kernel, grid, c3::D_NT, c.s, p.w3, sc.dy3, sc.dp2, n));
  }
  MLHOT_TRY(folds.pend(slab_w3, g.w3, rows3, C3_L, C3_R, 2));
  MLHOT_TRY(folds.pend(slab_b3, g.b3, rows3, 64, C3_R));
  // conv2 + conv1 (pool + ReLU backward on the way in; conv1's gradients come out of the data-gradient kernel)
  MLHOT_TRY(conv12_backward(c2::ImgSrc{c.img0, c.n0, c.img1}, n, p.w1, p.b1, p.w2, sc.dp2, sv, sl, r, c.s));
  MLHOT_TRY(conv12_pend_conv2(sl, n, g.w2, g.b2, folds));
  if (g.b1 == g.w1 + 288 && (reinterpret_cast<uintptr_t>(g.w1) & 15) == 0) MLHOT_TRY(folds.pend(sl.c1, g.w1, conv12_grid(n), C1_R, C1_R));
  else MLHOT_TRY(ws_launch("slab_reduce", c2::conv1_grads_kernel, 16, 320, c.s, sl.c1, conv12_grid(n), g.w1, g.b1));
  return folds.flush(c.s, "slab_reduce");
}
#endif

// ---- the entries: carve, check, route, dispatch --------------------------------------------------------------------------------------
inline int enc_forward(const float* img0, int n0, const float* img1, int n1, const mlhot_enc_params& p, int dim_w,
                       Rows2 feat, void* saved, void* scratch, size_t scratch_bytes, hipStream_t s, EncXFold* xfold = nullptr) {
  if (xfold != nullptr) *xfold = EncXFold{nullptr, nullptr, 0, 0};
  const int n = n0 + n1;
  if (n <= 0) return MLHOT_OK;
  const EncCall c{img0, n0, img1, n1, p, dim_w, enc_saved_carve(n, saved, (size_t)-1 / 2), enc_scratch_carve(n, dim_w, scratch, scratch_bytes), s};
  if (!c.sc.ok) return enc_scratch_short("enc_vanilla_fwd", scratch_bytes, c.sc.bytes);
#ifndef MLHOT_HOSTSIM
  const EncRoute r = enc_route(n, dim_w);
  if (r.ws) return enc_forward_ws(c, r, feat, xfold);
#endif
  return enc_forward_generic(c, feat);
}

// `extra`: a slab sum the caller has pending (the fused tail's per-task gradient slabs); the weight-stationary backward folds it
// into its own final reduce launch, the generic chain (and an empty batch) sums it first.
inline int enc_backward(const float* img0, int n0, const float* img1, int n1, const mlhot_enc_params& p, int dim_w,
                        Rows2 dfeat, const void* saved, const mlhot_enc_grads& g,
                        void* scratch, size_t scratch_bytes, hipStream_t s, const PendingSum* extra = nullptr) {
  const int n = n0 + n1;
  const EncCall c{img0, n0, img1, n1, p, dim_w, enc_saved_carve(n, (void*)saved, (size_t)-1 / 2), enc_scratch_carve(n, dim_w, scratch, scratch_bytes), s};
#ifndef MLHOT_HOSTSIM
  const EncRoute r = enc_route(n, dim_w);
  SlabFolds folds;
  if (extra != nullptr && extra->slab != nullptr) MLHOT_TRY(folds.pend(extra->slab, extra->out, extra->nparts, extra->len, extra->stride));
  if (r.ws && n > 0) return c.sc.ok ? enc_backward_ws(c, r, dfeat, g, folds) : enc_scratch_short("enc_vanilla_bwd", scratch_bytes, c.sc.bytes);
  MLHOT_TRY(folds.flush(s, "slab_reduce"));
#else
  (void)extra;
#endif
  if (n <= 0) return MLHOT_OK;
  if (!c.sc.ok) return enc_scratch_short("enc_vanilla_bwd", scratch_bytes, c.sc.bytes);
  return enc_backward_generic(c, dfeat, g);
}

}  // namespace mlhot
