// Host orchestration of the ResNet trunks (5x5 s2 stem + four BN-free BasicBlocks; networks/models.py:63-192,
// networks/ResNet.py:58-74, BBB twin networks/ANPMRShapeNet3D.py:40-90) on the weight-stationary kernels of resnet_ws.h.
// ONE call runs every pass of a model step (context images, target images, decoder images ...), each pass with its weight set:
//   forward  : prep (lane-native weight images) -> stem -> per block {conv1 3x3 s2 + ReLU [+ fused 1x1 s2 skip | + 3x3 s2 skip
//              as a second job of the same launch]} -> {conv2 3x3 s1 + skip + ReLU}                       (14 launches for c5)
//   backward : prep -> ReLU mask of the incoming gradient -> per block {conv2 data gradient (+ mask), conv2 weight gradient,
//              conv1 / skip data gradient (stride-2 classes, join + mask fused), conv1 / skip weight gradient} -> stem weight
//              gradient -> ONE fold of all weight-gradient slabs.  Passes that share a weight set (the deterministic encoder over
//              context and target images) write into the same slab rows' segment, so their gradients come out already summed.
// Everything lives in caller-owned buffers: `act` (saved activations per pass) and one scratch arena per call.
// trunk_route() decides what a call launches (the only reader of the trunk's options), trunk_plan() where its weight-gradient jobs write.
#pragma once
#include "common.h"
#include "foreach.h"
#include "options.h"
#include "resnet_ws.h"
#include "../../include/mlhot.h"

namespace mlhot {
#ifndef MLHOT_HOSTSIM
namespace rt {

constexpr int NCONV = 13;           // stem, then (conv1, conv2, skip) of the four blocks

struct Levels { int C, H, L[5]; };  // L[0] = stem output size, L[i] = output size of block i
inline Levels trunk_levels(int C, int H) { Levels v{C, H, {H / 2, H / 4, H / 8, H / 16, H / 32}}; return v; }
inline bool trunk_supported(int C, int H) { return rw::stem_supported(C, H); }      // (3, 64) and (1, 128): every block geometry below them is instantiated
inline size_t act_floats(const Levels& lv, int n, int k) {      // k: 0 = a0, 2i-1 = mid_i, 2i = y_i
  const int l = k == 0 ? lv.L[0] : lv.L[(k + 1) / 2];
  return (size_t)n * 64 * l * l;
}

struct MaskJob { const float* g; const float* y; float* out; size_t n; };
struct MaskJobs { MaskJob j[MLHOT_TRUNK_MAX_PASS]; int n; size_t first[MLHOT_TRUNK_MAX_PASS + 1]; };
__global__ __launch_bounds__(256) void mask_kernel(const MaskJobs jobs) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < jobs.first[jobs.n]; i += (size_t)gridDim.x * 256) {
    int k = 0;
    while (k + 1 < jobs.n && i >= jobs.first[k + 1]) ++k;
    const size_t e = i - jobs.first[k];
    jobs.j[k].out[e] = jobs.j[k].y[e] > 0.f ? jobs.j[k].g[e] : 0.f;
  }
}

inline int conv_hin(const Levels& lv, int conv) {        // input size of conv index 1..12: (c1, c2, sk) of block b = (conv - 1) / 3 + 1
  const int b = (conv - 1) / 3 + 1, r = (conv - 1) % 3;
  return r == 1 ? lv.L[b] : lv.L[b - 1];
}
inline int conv_stride(int conv) { return (conv - 1) % 3 == 1 ? 1 : 2; }

// ---- the route: every decision of a call, taken once ------------------------------------------------------------------
struct TrunkRoute {
  bool fuse34;              // blocks 3 and 4 as one launch per direction (rw::tail34_*): 64 x 64 trunks (8 x 8 -> 4 x 4 -> 2 x 2 maps), "trunk_fuse34" option
  bool wgrad34;             // ... and their 3x3 weight gradients as ONE launch (rw::wgrad34_kernel) when its job table holds them: conv1 + conv2 of every
                            // pass + the 3x3 skips, for both blocks (16 jobs for c5's three passes); per-block launches otherwise
  bool split_kinds[5];      // [block] forward stage A: the 1x1-skip and the 3x3-skip passes as two launches.  On the 32x32 input the kernel variant with the
                            // fused 1x1 skip (16 more weight registers, a second epilogue) costs the passes that do not need it more than a launch (158 us
                            // in one launch, 49 + 97 us in two); from 16x16 down one launch is the faster way
  bool dual_dgrad[5];       // [block] a 3x3-skip block's two stride-2 data gradients in ONE launch (rw::dgrad2_dual_kernel), "trunk_dual_dgrad" option
  // [conv] slab rows a weight-gradient launch is planned against (x 4 channel tiles = workgroups): every row is 147 KB written by the
  // kernel and read again by the fold.  The stem gets 512 workgroups in all.  The 4 x 4 / 2 x 2 output maps get 64 rows (256
  // workgroups): measured 128 / 64 / 32 rows at c5's shape - weight gradient of block 3's conv1 19.2 / 17.9 / 22.9 us, conv2 13.0 /
  // 13.0 / 15.4, fold 34.3 / 33.9 / 32.9.  The larger maps: option "trunk_wg_rows", default 128
  int wg_target[NCONV];
  bool skip1_set[MLHOT_TRUNK_MAX_WSET];
  bool is_skip1(int w) const { return skip1_set[w]; }                              // the weight set's skip convolutions are 1x1 (else 3x3)
  bool skip1(int w, int conv) const { return conv > 0 && conv % 3 == 0 && skip1_set[w]; }      // conv is a 1x1 skip convolution of weight set w
};
inline TrunkRoute trunk_route(const Levels& lv, const mlhot_trunk_pass* ps, int n_pass, const mlhot_trunk_wset* ws, int n_wset) {
  TrunkRoute r{};
  int n_skip3 = 0;
  for (int w = 0; w < n_wset; ++w) r.skip1_set[w] = ws[w].skip_k == 1;
  for (int p = 0; p < n_pass; ++p) n_skip3 += !r.skip1_set[ps[p].wset];
  r.fuse34 = g_opt.trunk_fuse34 && lv.L[2] == 8;
  r.wgrad34 = r.fuse34 && 2 * (2 * n_pass + n_skip3) <= rw::WG34_MAX;
  for (int b = 1; b <= 4; ++b) { r.split_kinds[b] = lv.L[b - 1] >= 32; r.dual_dgrad[b] = g_opt.trunk_dual_dgrad && rw::dgrad2_dual_supported(lv.L[b]); }
  r.wg_target[0] = 512;
  for (int c = 1; c < NCONV; ++c) r.wg_target[c] = conv_hin(lv, c) / conv_stride(c) <= 4 ? 64 : g_opt.trunk_wg_rows;
  return r;
}

// ---- the slab-row plan: where every weight-gradient job writes --------------------------------------------------------
struct TrunkPlan {
  int z0[MLHOT_TRUNK_MAX_PASS][NCONV], nz[MLHOT_TRUNK_MAX_PASS][NCONV];      // (pass, conv): first row in its weight set's slab, row count
  int rows[MLHOT_TRUNK_MAX_WSET][NCONV];                                     // (weight set, conv): rows in all
};
// slab rows (position splits) of one weight-gradient job: the launch aims at `target` rows over all its jobs, a row covers at least one band
inline int wg_rows(int bands, int total_bands, int target) {
  int nz = total_bands <= target ? bands : (int)((long)target * bands / total_bands);
  if (nz < 1) nz = 1;
  if (nz > bands) nz = bands;
  return nz;
}
// Per convolution, passes in index order: the passes of a weight set get adjacent row ranges, so their gradients come out summed.
inline TrunkPlan trunk_plan(const mlhot_trunk_pass* ps, int n_pass, const Levels& lv, const TrunkRoute& rt) {
  TrunkPlan pl{};
  for (int c = 0; c < NCONV; ++c) {
    int bands[MLHOT_TRUNK_MAX_PASS], total = 0, total1 = 0;      // bands of every pass / of the 1x1-skip passes
    for (int p = 0; p < n_pass; ++p) {
      bands[p] = c == 0 ? ps[p].n_img * (lv.L[0] * lv.L[0] / 256) : rw::wgrad_bands_rt(conv_hin(lv, c), conv_stride(c), ps[p].n_img);
      total += bands[p];
      if (rt.is_skip1(ps[p].wset)) total1 += bands[p];
    }
    // conv1 of every pass and the 3x3 skips (same input, same geometry) share ONE launch: its ~512 workgroups are split over all
    // of those jobs.  (Planned per convolution, ShapeNet3D's block-1 launch came to 840 workgroups for 512 resident slots: a second
    // round 64 % full, 143 us where one round needs ~95 - per-workgroup start / end stamps, scripts/dev/trunk_wgrad_ts.py.)
    const int shared = total + (total - total1);
    for (int p = 0; p < n_pass; ++p) {
      const int w = ps[p].wset;
      // the band total a job's rows are planned against, that of its launch: the stem and conv2 have one of their own over all
      // passes; the 1x1 skips of a step share one (rw::skip1_wgrad_kernel), so they split ITS workgroups among themselves
      const int launch = c == 0 || c % 3 == 2 ? total : rt.skip1(w, c) ? total1 : shared;
      pl.z0[p][c] = pl.rows[w][c];
      pl.nz[p][c] = wg_rows(bands[p], launch, rt.wg_target[c]);
      pl.rows[w][c] += pl.nz[p][c];
    }
  }
  return pl;
}

struct TrunkScratch {
  float* wimg[MLHOT_TRUNK_MAX_WSET][NCONV];       // F images (forward) / D images (backward; stem: unused)
  float* idn[MLHOT_TRUNK_MAX_PASS];               // forward: skip-path output of the current block
  float* G[MLHOT_TRUNK_MAX_PASS][5];              // backward: masked gradient wrt a0 / y_1..y_4
  float* DM[MLHOT_TRUNK_MAX_PASS];                // backward: masked gradient wrt mid_i of the current block
  float* idn4[MLHOT_TRUNK_MAX_PASS];              // fused blocks 3-4, forward: block 4's skip-path output (idn = block 3's)
  float* DM34[MLHOT_TRUNK_MAX_PASS][2];           // fused blocks 3-4, backward: masked gradients wrt mid_3, mid_4 (both outlive the fused launch)
  float* slab[MLHOT_TRUNK_MAX_WSET][NCONV]; float* slab_b[MLHOT_TRUNK_MAX_WSET][NCONV];      // backward: TrunkPlan::rows rows each
  bool ok; size_t bytes;
};

inline TrunkScratch trunk_carve(const mlhot_trunk_pass* ps, int n_pass, int n_wset, const Levels& lv, const TrunkRoute& rt, const TrunkPlan& pl, bool backward, void* base, size_t cap) {
  Arena a(base, cap);
  TrunkScratch s{};
  for (int w = 0; w < n_wset; ++w) {
    s.wimg[w][0] = a.take<float>((size_t)4 * ((25 * lv.C + 3) / 4) * 64);
    for (int c = 1; c < NCONV; ++c) s.wimg[w][c] = a.take<float>(rt.skip1(w, c) ? rw::WIMG1 : rw::WIMG);
  }
  for (int p = 0; p < n_pass; ++p) {
    if (!backward) { s.idn[p] = a.take<float>(act_floats(lv, ps[p].n_img, 2)); s.idn4[p] = a.take<float>(act_floats(lv, ps[p].n_img, 8)); continue; }
    for (int l = 0; l < 5; ++l) s.G[p][l] = a.take<float>(act_floats(lv, ps[p].n_img, 2 * l));
    s.DM[p] = a.take<float>(act_floats(lv, ps[p].n_img, 1));
    s.DM34[p][0] = a.take<float>(act_floats(lv, ps[p].n_img, 5)); s.DM34[p][1] = a.take<float>(act_floats(lv, ps[p].n_img, 7));
  }
  for (int c = 0; backward && c < NCONV; ++c)
    for (int w = 0; w < n_wset; ++w) {
      const size_t rowlen = c == 0 ? (size_t)rw::stem_slab_row(lv.C) : (rt.skip1(w, c) ? rw::SLAB1 : rw::SLAB3);
      s.slab[w][c] = a.take<float>(rowlen * pl.rows[w][c]);      // trunk_check: every weight set has a pass, so at least one row
      s.slab_b[w][c] = a.take<float>((size_t)64 * pl.rows[w][c]);
    }
  s.ok = a.ok; s.bytes = a.off + 256;
  return s;
}

inline int trunk_check(const mlhot_trunk_pass* ps, int n_pass, const mlhot_trunk_wset* ws, int n_wset, int C, int H) {
  if (!ps || !ws || n_pass < 1 || n_pass > MLHOT_TRUNK_MAX_PASS || n_wset < 1 || n_wset > MLHOT_TRUNK_MAX_WSET) { set_error("resnet trunk: bad pass / weight-set count"); return MLHOT_ERR_ARG; }
  if (!trunk_supported(C, H)) { set_error("resnet trunk: no kernels for %d-channel %dx%d images", C, H, H); return MLHOT_ERR_UNSUPPORTED; }
  for (int p = 0; p < n_pass; ++p)
    if (ps[p].n_img < 1 || ps[p].wset < 0 || ps[p].wset >= n_wset || !ps[p].img) { set_error("resnet trunk: bad pass %d", p); return MLHOT_ERR_ARG; }
  for (int w = 0; w < n_wset; ++w) {
    if (ws[w].skip_k != 1 && ws[w].skip_k != 3) { set_error("resnet trunk: skip kernel must be 1 or 3"); return MLHOT_ERR_ARG; }
    bool used = false;
    for (int p = 0; p < n_pass; ++p) used = used || ps[p].wset == w;
    // a weight set without a pass would get no slab rows: its gradients would never be written (the caller would read whatever was in the buffers)
    if (!used) { set_error("resnet trunk: weight set %d is not used by any pass", w); return MLHOT_ERR_ARG; }
  }
  return MLHOT_OK;
}

// One call: its arguments, what was decided for it, where its buffers are.  The steps below read it and launch.
struct TrunkCall {
  const mlhot_trunk_pass* ps; int n_pass; const mlhot_trunk_wset* ws; int n_wset;
  Levels lv; TrunkRoute rt; TrunkPlan pl; TrunkScratch sc; hipStream_t s;
  const mlhot_trunk_wset& wset(int p) const { return ws[ps[p].wset]; }
  const float* wimg(int p, int conv) const { return sc.wimg[ps[p].wset][conv]; }
  bool in_fused(int b) const { return rt.fuse34 && b >= 3; }
  // block b of pass p: its input, conv1's output, and the masked gradients wrt its output and wrt conv1's output
  const float* xin(int p, int b) const { return ps[p].act[2 * b - 2]; }
  const float* mid(int p, int b) const { return ps[p].act[2 * b - 1]; }
  float* g(int p, int b) const { return sc.G[p][b]; }
  float* dm(int p, int b) const { return in_fused(b) ? sc.DM34[p][b - 3] : sc.DM[p]; }
};
// of arguments trunk_check() has passed; base = nullptr: the size query (sc.bytes)
inline TrunkCall trunk_call(const mlhot_trunk_pass* ps, int n_pass, const mlhot_trunk_wset* ws, int n_wset, int C, int H, bool backward, void* base, size_t cap, hipStream_t s) {
  TrunkCall t{ps, n_pass, ws, n_wset, trunk_levels(C, H)};
  t.rt = trunk_route(t.lv, ps, n_pass, ws, n_wset);
  t.pl = trunk_plan(ps, n_pass, t.lv, t.rt);
  t.sc = trunk_carve(ps, n_pass, n_wset, t.lv, t.rt, t.pl, backward, base, cap);
  t.s = s;
  return t;
}

inline int trunk_prep(const TrunkCall& t, bool d_images) {
  rw::PrepItems items{};
  for (int w = 0; w < t.n_wset; ++w) {
    if (!d_images) items.it[items.n++] = rw::PrepItem{t.ws[w].w[0], t.sc.wimg[w][0], nullptr, 2, 25 * t.lv.C};
    for (int c = 1; c < NCONV; ++c) {
      const int kind = t.rt.skip1(w, c) ? 1 : 0;
      items.it[items.n++] = d_images ? rw::PrepItem{t.ws[w].w[c], nullptr, t.sc.wimg[w][c], kind, 0} : rw::PrepItem{t.ws[w].w[c], t.sc.wimg[w][c], nullptr, kind, 0};
    }
  }
  ProfScope ps("trunk.prep", t.s);
  hipLaunchKernelGGL(rw::prep_kernel, dim3(144, items.n), dim3(256), 0, t.s, items);      // 4 x 144 = the 576 wave items of a 3x3 image: one trip per wave (with 16 blocks a wave made nine load -> store trips, each a round trip: 10.6 us)
  return check_launch("trunk.prep");
}

// launch labels per block (mlhot_prof_*): a label is one geometry, so its time over its algorithmic FLOPs is a kernel's rate
#define MLHOT_TRUNK_LABELS(name) {name ".b0", name ".b1", name ".b2", name ".b3", name ".b4"}
static const char* const LBL_CONV1[5] = MLHOT_TRUNK_LABELS("trunk.conv1");
static const char* const LBL_CONV2[5] = MLHOT_TRUNK_LABELS("trunk.conv2");
static const char* const LBL_C2_DGRAD[5] = MLHOT_TRUNK_LABELS("trunk.bwd.conv2.dgrad");
static const char* const LBL_C2_WGRAD[5] = MLHOT_TRUNK_LABELS("trunk.bwd.conv2.wgrad");
static const char* const LBL_C1_DGRAD[5] = MLHOT_TRUNK_LABELS("trunk.bwd.conv1.dgrad");
static const char* const LBL_C1_DGRAD2[5] = MLHOT_TRUNK_LABELS("trunk.bwd.conv1.dgrad2");
static const char* const LBL_C1_WGRAD[5] = MLHOT_TRUNK_LABELS("trunk.bwd.conv1.wgrad");

// blocks 3 and 4 in one launch, either direction: one record per pass (the other direction's buffers are not carved: null)
inline int trunk_b34(const TrunkCall& t, bool backward) {
  rw::T34Jobs jobs{};
  for (int p = 0; p < t.n_pass; ++p) {
    rw::T34Pass& r = jobs.p[jobs.n++];
    r = rw::T34Pass{};
    r.x = t.ps[p].act[4]; r.mid3 = t.ps[p].act[5]; r.y3 = t.ps[p].act[6]; r.mid4 = t.ps[p].act[7]; r.y4 = t.ps[p].act[8];
    r.idn3 = t.sc.idn[p]; r.idn4 = t.sc.idn4[p];
    for (int i = 0; i < 6; ++i) { r.wimg[i] = t.wimg(p, 7 + i); r.b[i] = backward ? nullptr : t.wset(p).b[7 + i]; }      // c1_3, c2_3, sk_3, c1_4, c2_4, sk_4
    r.g4 = t.sc.G[p][4]; r.dm4 = t.sc.DM34[p][1]; r.g3 = t.sc.G[p][3]; r.dm3 = t.sc.DM34[p][0]; r.g2 = t.sc.G[p][2];
    r.n_img = t.ps[p].n_img; r.skip1 = t.rt.is_skip1(t.ps[p].wset);
  }
  return rw::tail34_launch(jobs, backward, t.s, backward ? "trunk.bwd.b34.dgrad" : "trunk.fwd.b34");
}

// ---- forward steps ------------------------------------------------------------------------------------------------------
inline int fwd_stem(const TrunkCall& t) {
  rw::StemJobs jobs{};
  for (int p = 0; p < t.n_pass; ++p) jobs.j[jobs.n++] = rw::StemJob{t.ps[p].img, t.wimg(p, 0), t.wset(p).b[0], t.ps[p].act[0], t.ps[p].n_img, 0, 0};
  return rw::stem_dispatch(t.lv.C, t.lv.H, jobs, t.s, "trunk.stem");
}
// stage A: conv1 (+ReLU) and the skip convolution, both on the block input - ONE launch for every pass (two under split_kinds; one
// more whenever the job table is full): a 3x3 skip is a second job on the same input, a 1x1 skip rides in its conv1 job
// (centre-tap operand)
inline int fwd_stage_a(const TrunkCall& t, int b) {
  const int c1 = 3 * b - 2, sk = c1 + 2, hin = t.lv.L[b - 1];
  const bool split = t.rt.split_kinds[b];
  for (int kind = 0; kind < (split ? 2 : 1); ++kind) {
    rw::FwdJobs jobs{};
    bool any1 = false;
    for (int p = 0; p < t.n_pass; ++p) {
      const mlhot_trunk_wset& w = t.wset(p);
      const bool s1 = t.rt.is_skip1(t.ps[p].wset);
      if (split && s1 != (kind == 0)) continue;
      if (jobs.n + (s1 ? 1 : 2) > rw::MAX_JOBS) { MLHOT_TRY(rw::conv3x3_dispatch(hin, 2, any1, jobs, t.s, LBL_CONV1[b])); jobs.n = 0; any1 = false; }
      any1 = any1 || s1;
      jobs.j[jobs.n++] = rw::FwdJob{t.xin(p, b), t.wimg(p, c1), w.b[c1], t.ps[p].act[2 * b - 1], nullptr, s1 ? t.wimg(p, sk) : nullptr, s1 ? w.b[sk] : nullptr, s1 ? t.sc.idn[p] : nullptr,
                                    t.ps[p].n_img, rw::EPI_BIAS_RELU, 0, 0, 0};
      if (!s1) jobs.j[jobs.n++] = rw::FwdJob{t.xin(p, b), t.wimg(p, sk), w.b[sk], t.sc.idn[p], nullptr, nullptr, nullptr, nullptr, t.ps[p].n_img, rw::EPI_BIAS, 0, 0, 0};
    }
    if (jobs.n) MLHOT_TRY(rw::conv3x3_dispatch(hin, 2, any1, jobs, t.s, LBL_CONV1[b]));
  }
  return MLHOT_OK;
}
// stage B: conv2 + skip + ReLU
inline int fwd_stage_b(const TrunkCall& t, int b) {
  const int c2 = 3 * b - 1;
  rw::FwdJobs jobs{};
  for (int p = 0; p < t.n_pass; ++p)
    jobs.j[jobs.n++] = rw::FwdJob{t.mid(p, b), t.wimg(p, c2), t.wset(p).b[c2], t.ps[p].act[2 * b], t.sc.idn[p], nullptr, nullptr, nullptr, t.ps[p].n_img, rw::EPI_BIAS_RES_RELU, 0, 0, 0};
  return rw::conv3x3_dispatch(t.lv.L[b], 1, false, jobs, t.s, LBL_CONV2[b]);
}

inline int trunk_forward(const mlhot_trunk_pass* ps, int n_pass, const mlhot_trunk_wset* ws, int n_wset, int C, int H, void* scratch,
                         size_t scratch_bytes, hipStream_t s) {
  MLHOT_TRY(trunk_check(ps, n_pass, ws, n_wset, C, H));
  const TrunkCall t = trunk_call(ps, n_pass, ws, n_wset, C, H, false, scratch, scratch_bytes, s);
  if (!t.sc.ok) { set_error("resnet trunk fwd: scratch too small (%zu < %zu)", scratch_bytes, t.sc.bytes); return MLHOT_ERR_WORKSPACE; }
  MLHOT_TRY(trunk_prep(t, false));
  MLHOT_TRY(fwd_stem(t));
  for (int b = 1; b <= (t.rt.fuse34 ? 2 : 4); ++b) { MLHOT_TRY(fwd_stage_a(t, b)); MLHOT_TRY(fwd_stage_b(t, b)); }
  if (t.rt.fuse34) MLHOT_TRY(trunk_b34(t, false));
  return MLHOT_OK;
}

// ---- backward steps -----------------------------------------------------------------------------------------------------
inline int bwd_mask(const TrunkCall& t) {
  MaskJobs mj{};
  for (int p = 0; p < t.n_pass; ++p) {
    mj.j[p] = MaskJob{t.ps[p].dfeat, t.ps[p].act[8], t.sc.G[p][4], act_floats(t.lv, t.ps[p].n_img, 8)};
    mj.first[p + 1] = mj.first[p] + mj.j[p].n;
  }
  mj.n = t.n_pass;
  const size_t want = (mj.first[t.n_pass] + 255) / 256, blocks = want > 1024 ? 1024 : want;
  ProfScope pr("trunk.bwd.mask", t.s);
  hipLaunchKernelGGL(mask_kernel, dim3((unsigned)blocks), dim3(256), 0, t.s, mj);
  return check_launch("trunk.bwd.mask");
}
// the 3x3 weight-gradient jobs of one convolution (conv1: block input x d_mid, conv2: mid x g, 3x3 skip: block input x g), passes in
// index order, each into the slab rows the plan gave it
inline void wg_jobs(const TrunkCall& t, int conv, rw::WgJobs& jobs) {
  const int b = (conv - 1) / 3 + 1, r = (conv - 1) % 3;
  for (int p = 0; p < t.n_pass; ++p) {
    const int w = t.ps[p].wset;
    if (!t.rt.skip1(w, conv)) jobs.j[jobs.n++] = rw::WgJob{r == 1 ? t.mid(p, b) : t.xin(p, b), r == 0 ? t.dm(p, b) : t.g(p, b), t.sc.slab[w][conv], t.sc.slab_b[w][conv], t.ps[p].n_img, t.pl.z0[p][conv], t.pl.nz[p][conv], 0};
  }
}
inline void wg34_add(rw::Wg34Jobs& w34, const rw::WgJobs& jobs, int geo) { for (int i = 0; i < jobs.n; ++i) { w34.j[w34.n] = jobs.j[i]; w34.geo[w34.n++] = (unsigned char)geo; } }
// conv2 data gradient: d_mid = conv^T(g, W2) * (mid > 0)
inline int bwd_conv2_dgrad(const TrunkCall& t, int b) {
  rw::FwdJobs jobs{};
  for (int p = 0; p < t.n_pass; ++p)
    jobs.j[jobs.n++] = rw::FwdJob{t.g(p, b), t.wimg(p, 3 * b - 1), nullptr, t.sc.DM[p], t.mid(p, b), nullptr, nullptr, nullptr, t.ps[p].n_img, rw::EPI_MASK, 1, 0, 0};
  return rw::conv3x3_dispatch(t.lv.L[b], 1, false, jobs, t.s, LBL_C2_DGRAD[b]);
}
// conv2 weight gradient; fused blocks 3-4 under wgrad34: into the one launch behind block 3
inline int bwd_conv2_wgrad(const TrunkCall& t, int b, rw::Wg34Jobs& w34) {
  rw::WgJobs jobs{};
  wg_jobs(t, 3 * b - 1, jobs);
  if (t.in_fused(b) && t.rt.wgrad34) { wg34_add(w34, jobs, b == 3 ? 1 : 3); return MLHOT_OK; }
  return rw::wgrad_dispatch(t.lv.L[b], 1, false, jobs, t.s, LBL_C2_WGRAD[b]);
}
// data gradient into the block input (not needed for images: block 1's input is the stem output, whose gradient feeds the stem's wgrad)
// launch 1: every first writer of dx - the 3x3 skips' data gradients and the 1x1-skip blocks' fused conv1 + skip gradient; launch 2: the
// 3x3-skip blocks' conv1 gradient, added onto launch 1's result and masked - or, under dual_dgrad, both sources of a 3x3-skip block
// (skip^T(g), conv1^T(dm)) in ONE launch, dx written once with its mask (rw::dgrad2_dual_kernel)
inline int bwd_conv1_dgrad(const TrunkCall& t, int b) {
  const int c1 = 3 * b - 2, sk = c1 + 2;
  rw::DgJobs ja{}, jb2{}, jd{};
  bool any1 = false;
  for (int p = 0; p < t.n_pass; ++p) {
    float* dx = t.g(p, b - 1);
    const int n = t.ps[p].n_img;
    if (t.rt.is_skip1(t.ps[p].wset)) { any1 = true; ja.j[ja.n++] = rw::DgJob{t.dm(p, b), t.wimg(p, c1), dx, t.xin(p, b), t.g(p, b), t.wimg(p, sk), n, 0, 0, 0}; }
    else if (t.rt.dual_dgrad[b]) jd.j[jd.n++] = rw::DgJob{t.g(p, b), t.wimg(p, sk), dx, t.xin(p, b), t.dm(p, b), t.wimg(p, c1), n, 0, 0, 0};
    else {
      ja.j[ja.n++] = rw::DgJob{t.g(p, b), t.wimg(p, sk), dx, nullptr, nullptr, nullptr, n, 0, 0, 0};
      jb2.j[jb2.n++] = rw::DgJob{t.dm(p, b), t.wimg(p, c1), dx, t.xin(p, b), nullptr, nullptr, n, 1, 0, 0};
    }
  }
  MLHOT_TRY(rw::dgrad2_dispatch(t.lv.L[b], any1, ja, t.s, LBL_C1_DGRAD[b]));      // (split by kind like the forward: no gain here)
  MLHOT_TRY(rw::dgrad2_dispatch(t.lv.L[b], false, jb2, t.s, LBL_C1_DGRAD2[b]));
  return rw::dgrad2_dual_dispatch(t.lv.L[b], jd, t.s, LBL_C1_DGRAD2[b]);
}
// conv1 and 3x3-skip weight gradients (same input, same geometry): one launch, a second one when the job table is full; fused
// blocks 3-4 under wgrad34: ONE launch for both blocks, conv2's jobs included, behind block 3
inline int bwd_conv1_wgrad(const TrunkCall& t, int b, rw::Wg34Jobs& w34) {
  const int c1 = 3 * b - 2, sk = c1 + 2;
  rw::WgJobs jobs{};
  wg_jobs(t, c1, jobs);
  if (t.in_fused(b) && t.rt.wgrad34) {
    wg34_add(w34, jobs, b == 3 ? 0 : 2);
    jobs.n = 0;
    wg_jobs(t, sk, jobs);
    wg34_add(w34, jobs, b == 3 ? 0 : 2);
    return b == 3 ? rw::wgrad34_launch(w34, t.s, "trunk.bwd.b34.wgrad") : MLHOT_OK;
  }
  if (jobs.n + t.n_pass > rw::MAX_JOBS) { MLHOT_TRY(rw::wgrad_dispatch(t.lv.L[b - 1], 2, false, jobs, t.s, LBL_C1_WGRAD[b])); jobs.n = 0; }
  wg_jobs(t, sk, jobs);
  return rw::wgrad_dispatch(t.lv.L[b - 1], 2, false, jobs, t.s, LBL_C1_WGRAD[b]);
}
// 1x1-skip weight gradients: collected over the blocks, one launch behind them (same slab rows as a per-block launch would use)
inline int bwd_skip1_collect(const TrunkCall& t, int b, rw::Sk1Jobs& sk1) {
  const int sk = 3 * b;
  int lg = 0;
  while ((2 << lg) < t.lv.L[b - 1]) ++lg;      // output map HO = L[b - 1] / 2 = 1 << lg
  for (int p = 0; p < t.n_pass; ++p) {
    const int w = t.ps[p].wset;
    if (!t.rt.skip1(w, sk)) continue;
    if (sk1.n >= rw::SK1_MAX) { set_error("resnet trunk bwd: too many 1x1 skip jobs"); return MLHOT_ERR_ARG; }
    sk1.j[sk1.n++] = rw::Sk1Job{t.xin(p, b), t.g(p, b), t.sc.slab[w][sk], t.sc.slab_b[w][sk], t.ps[p].n_img, lg, t.pl.z0[p][sk], t.pl.nz[p][sk], 0};      // a row beyond the last chunk is written as zeros
  }
  return MLHOT_OK;
}
inline int bwd_stem_wgrad(const TrunkCall& t) {
  rw::StemWgJobs jobs{};
  for (int p = 0; p < t.n_pass; ++p)
    jobs.j[jobs.n++] = rw::StemWgJob{t.ps[p].img, t.sc.G[p][0], t.sc.slab[t.ps[p].wset][0], t.ps[p].n_img, t.pl.z0[p][0], t.pl.nz[p][0], 0};
  return rw::stem_wgrad_dispatch(t.lv.C, t.lv.H, jobs, t.s, "trunk.bwd.stem.wgrad");
}
// fold the slabs: every convolution's weight and bias gradient of every weight set in one launch (a second one only if the
// segment table overflows its kernel-argument block)
inline int bwd_fold(const TrunkCall& t, const void* scratch) {
  rw::WsumSegs segs{};
  segs.base = static_cast<const float*>(scratch);
  auto flush = [&]() -> int {
    if (segs.blocks > 0) {
      ProfScope pr("trunk.bwd.wsum", t.s);
      hipLaunchKernelGGL(rw::wsum_kernel, dim3(segs.blocks), dim3(256), 0, t.s, segs);
      MLHOT_TRY(check_launch("trunk.bwd.wsum"));
    }
    segs.n = 0; segs.blocks = 0;
    return MLHOT_OK;
  };
  auto add = [&](const float* slab, float* out, float* out_b, int nrows, int kind, int K) -> int {
    if (segs.n >= rw::WSUM_MAX) MLHOT_TRY(flush());
    if (!rw::wsum_add(segs, slab, out, out_b, nrows, kind, K)) { set_error("resnet trunk bwd: slab does not fit the fold table"); return MLHOT_ERR_ARG; }
    return MLHOT_OK;
  };
  for (int w = 0; w < t.n_wset; ++w) {
    const mlhot_trunk_wset& ws = t.ws[w];
    if (ws.dw[0]) MLHOT_TRY(add(t.sc.slab[w][0], ws.dw[0], ws.db[0], t.pl.rows[w][0], 3, 25 * t.lv.C));
    for (int c = 1; c < NCONV; ++c) {
      if (!ws.dw[c]) continue;
      MLHOT_TRY(add(t.sc.slab[w][c], ws.dw[c], nullptr, t.pl.rows[w][c], t.rt.skip1(w, c) ? 1 : 0, 0));
      if (ws.db[c]) MLHOT_TRY(add(t.sc.slab_b[w][c], ws.db[c], nullptr, t.pl.rows[w][c], 2, 0));
    }
  }
  return flush();
}

inline int trunk_backward(const mlhot_trunk_pass* ps, int n_pass, const mlhot_trunk_wset* ws, int n_wset, int C, int H, void* scratch,
                          size_t scratch_bytes, hipStream_t s) {
  MLHOT_TRY(trunk_check(ps, n_pass, ws, n_wset, C, H));
  const TrunkCall t = trunk_call(ps, n_pass, ws, n_wset, C, H, true, scratch, scratch_bytes, s);
  if (!t.sc.ok) { set_error("resnet trunk bwd: scratch too small (%zu < %zu)", scratch_bytes, t.sc.bytes); return MLHOT_ERR_WORKSPACE; }
  for (int p = 0; p < n_pass; ++p) if (!ps[p].dfeat) { set_error("resnet trunk bwd: pass %d has no output gradient", p); return MLHOT_ERR_ARG; }
  MLHOT_TRY(trunk_prep(t, true));
  MLHOT_TRY(bwd_mask(t));
  if (t.rt.fuse34) MLHOT_TRY(trunk_b34(t, true));      // every data gradient of blocks 4 and 3 in one launch; their weight gradients follow in the loop below
  rw::Sk1Jobs sk1{};
  rw::Wg34Jobs w34{};
  for (int b = 4; b >= 1; --b) {
    if (!t.in_fused(b)) MLHOT_TRY(bwd_conv2_dgrad(t, b));
    MLHOT_TRY(bwd_conv2_wgrad(t, b, w34));
    if (!t.in_fused(b)) MLHOT_TRY(bwd_conv1_dgrad(t, b));
    MLHOT_TRY(bwd_conv1_wgrad(t, b, w34));
    MLHOT_TRY(bwd_skip1_collect(t, b, sk1));
  }
  MLHOT_TRY(rw::skip1_wgrad_launch(sk1, s, "trunk.bwd.skip1.wgrad"));
  MLHOT_TRY(bwd_stem_wgrad(t));
  return bwd_fold(t, scratch);
}

}  // namespace rt
#endif  // !MLHOT_HOSTSIM
}  // namespace mlhot
