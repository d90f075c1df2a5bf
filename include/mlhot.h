/* mlhot.h - C ABI of libmlhot.so, the MI355X-native CNP/ANP meta-batch hot path.
 *
 * The reference (boschresearch/what-matters-for-meta-learning) is pure Python on torch and
 * has no FFI of its own; its plugin boundary is `networks/<Method>.py::<Method>(config)`
 * (train.py:41-45).  This header is the C boundary UNDER that plugin (SURVEY.md §8b, row
 * "C-ABI under the plugin"): one forward and one backward entry per hot-path row of
 * SURVEY.md §8(a), each citing the reference code it replaces.  The Python host mirror
 * (what-matters-for-meta-learning_amd/networks/*) binds these with ctypes.
 *
 * Contract for every entry:
 *   - returns 0 on success, a non-zero MLHOT_ERR_* code otherwise (mlhot_last_error() has text);
 *   - all pointers are DEVICE pointers to fp32 unless noted, caller-owned, 16-byte aligned;
 *   - no allocation, no host synchronisation, no default-stream use inside: work is enqueued
 *     on `stream` in order, so calls are hipGraph-capturable and re-entrant across streams;
 *   - workspaces are caller-provided; the *_bytes() helpers size them.
 *   - `stream` is a hipStream_t passed as void*.
 *
 * Threading (the reference's callers are ONE Python thread on the default stream).  The compute entries keep no
 * state between calls - everything lives in the caller's buffers - so concurrent calls from several host threads on different
 * streams and buffers are safe, and mlhot_last_error() is per thread.  The two DIAGNOSTIC facilities are process-global and are
 * not part of that guarantee: mlhot_set_option() flips implementation switches read by every later call of every thread (set
 * them before the first compute call, or from the one thread that issues the calls - the A/B tests do the latter), and the
 * mlhot_prof_begin/end() recorder may be driven by one thread at a time while no other thread is inside the library.
 */
#ifndef MLHOT_H
#define MLHOT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLHOT_ABI_VERSION 8

enum { MLHOT_ACT_NONE = 0, MLHOT_ACT_RELU = 1, MLHOT_ACT_TANH = 2 };
enum { MLHOT_AGG_MEAN = 0, MLHOT_AGG_MAX = 1, MLHOT_AGG_BACO = 2, MLHOT_AGG_ATTENTION = 3 };
/* trainer/losses.py:32-80 */
enum { MLHOT_LOSS_AZIMUTH = 0, MLHOT_LOSS_MSE = 1, MLHOT_LOSS_QUATERNION = 2, MLHOT_LOSS_DEGREE = 3, MLHOT_LOSS_DISTRACTOR = 4 };

int mlhot_version(void);
const char* mlhot_last_error(void);

/* Implementation switches for A/B tests (process-global, see Threading above): "conv2_tc" = 1 (default) runs the
 * weight-stationary conv2 kernels (csrc/conv_tc.h), 0 the generic implicit-GEMM problems; "tail_fused" = 1 (default) runs the
 * fused per-task tail kernels where they apply, "tail_spec" = bit mask of what the fused tails run specialised for the shipped
 * dimensions (csrc/tail_spec.h, cnp_spec.h; names in csrc/options.h enum TailSpec): 1 / 2 / 4 forward phases A / B / C, 8 / 16 / 32
 * backward phases C' / B' / A' (the CNP tail's one forward / backward kernel: 1 / 8), 64 phase A also folds the encoder Linear's
 * split-K partial results, 128 phase C' takes the loss's gradient itself when handed a loss descriptor, 512 phase B' as two
 * workgroups per (task, head), 1024 / 2048 phases C' / A' as two workgroups per task, 4096 four instead of two, 256 unassigned;
 * default 7935 = all, 0 = the run-time-shaped csrc/tail_fused.h / tail_cnp.h; "favor2" = 1
 * (default) the two-launch FAVOR+ kernels, 0 the operator chain; "favor_linear" = 1 (default 0) FAVOR+ in linear form above 32 shots
 * (mlhot_favor_linear_supported); "materialize_a1" = 1 additionally stores the conv1 output
 * (debug / tests; the fused conv1+conv2 kernels never need it); "conv2_split" = 1 (default 0) runs the vanilla encoder's conv1 +
 * conv2 + pool forward with conv2 on the bf16 matrix pipe over exact hi / mid / lo splits of the fp32 operands (csrc/conv_split.h:
 * same outputs' layout, same parity tolerances, 1.5 x the fp32 kernel; the benchmark's headline stays on the fp32 kernels).      */
int mlhot_set_option(const char* name, int value);

/* ---- bench-only: per-launch HIP-event timing ------------------------------------------------
 * Between begin and end every kernel launch of the library is bracketed by two events recorded
 * on its launch stream.  end() synchronises them and returns (label, milliseconds) records.
 * Not re-entrant, not capturable; used only by bench.py's roofline leg.                        */
int mlhot_prof_begin(int max_records);
int mlhot_prof_end(const char** labels, float* ms, int cap);

/* ---- NT-Xent, the functional-contrastive term of the FCL* models ------------------
 * replaces trainer/losses.py:82-99 (LossFunc.contrastive_loss / contrastive_loss_ANP -> pytorch_metric_learning.losses.NTXentLoss
 * (temperature = t), an un-vendored dependency: algorithm restated in oracle/ref_cpu.py::nt_xent, value parity unpinned).  z: [N, d]
 * embeddings (N <= 2048, d <= 256, d % 16 == 0); the labels are always arange blocks, label(i) = (i / div) % mod
 * (contrastive_loss: div = 1, mod = T, N = 2T; contrastive_loss_ANP: div = Nq, mod = T, N = T Nq).  ws: mlhot_nt_xent_ws_floats(N)
 * floats kept between forward and backward.  loss / dloss: device scalars; dz: [N, d].                                          */
size_t mlhot_nt_xent_ws_floats(int N);
int mlhot_nt_xent_fwd(const float* z, int N, int d, int div, int mod, float t, float* ws, float* loss, void* stream);
int mlhot_nt_xent_bwd(const float* z, int N, int d, int div, int mod, float t, const float* ws, const float* dloss, float* dz, void* stream);

/* ---- B1 (eps stream): torch's CPU normal_() random stream continued on the device -------------------
 * replaces the host-side `torch.empty(size).normal_(0, 1)` + `.to(device)` of bbb/BBBConv.py:86-95 and BBBLinear.py:79-88 for callers
 * that hand the generator over (what-matters-for-meta-learning_amd/mlhot/rng.py): MT19937 (ATen/core/MT19937RNGEngine.h), 24-bit
 * float uniforms, ATen's 16-wide Box-Muller normal_fill.  engine: uint32[626] = state[624], left, next - the engine's fields,
 * advanced in place exactly as `total_outputs` calls would.  segs: nseg records of 4 int64 {dst offset in out, size (>= 16), stream
 * offset of its first output, index of its first group of 16} in call order; a size that is not a multiple of 16 consumes
 * size + 16 outputs and owns size / 16 + 1 groups.  uniform_ws: total_outputs floats of scratch.  Uniforms and engine state are
 * bit-identical to torch's, the normals equal up to the last ulps of logf / sincosf.                                        */
int mlhot_mt19937_normal(uint32_t* engine, float* uniform_ws, float* out, const int64_t* segs, int nseg, int64_t total_outputs,
                         int64_t total_groups, void* stream);
/* The same draw from n_sub parallel sub-streams of stride_blocks 624-word blocks each (MT19937 jump-ahead; the polynomials
 * polys[n_sub - 1][624] = t^(624 stride_blocks k) mod phi, k = 1 .. n_sub - 1, come from mlhot/mt_jump.py): identical uniforms, normals
 * and final engine state.  Needs n_sub * stride_blocks >= the number of new blocks of the draw; jump_ws: mlhot_mt19937_jump_ws_words(n_sub)
 * uint32 words of scratch.  ~0.1 ms for 0.9 M outputs where the one-workgroup form takes ~1 ms.                               */
size_t mlhot_mt19937_jump_ws_words(int n_sub);
int mlhot_mt19937_normal_par(uint32_t* engine, float* uniform_ws, float* out, const int64_t* segs, int nseg, int64_t total_outputs,
                             int64_t total_groups, const uint32_t* polys, int n_sub, int stride_blocks, uint32_t* jump_ws, void* stream);

/* Host only (no device, no stream): the engine (uint32[626] as above) moved forward by n_outputs calls without producing them - the
 * state `n_outputs` draws of torch's CPU generator would leave behind.  Lets K host threads draw K contiguous pieces of one
 * `normal_()` stream at once, each on a torch.Generator set to its piece's starting state (networks/bbb/eps.py, bit-identical to
 * the sequential draw of bbb/BBBConv.py:86-95).                                                                              */
int mlhot_mt19937_advance(uint32_t* engine, uint64_t n_outputs);

/* Host only (no device, no stream; ABI 6): the inverse of the loaders' host conversion `img.astype(float32) / 255.0`
 * (dataset/shapenet_1d.py:189-190, dataset/shapenet_3d.py, utils/utils.py:26-30), checked element by element: dst[i] = the byte k
 * nearest to src[i] * div, *n_inexact = the number of elements whose (float)k / div differs from src[i] in any bit.  When it is 0
 * the batch may cross PCIe as the n bytes of dst and mlhot_ingest_u8_nhwc (same div) reproduces src bit for bit on the device;
 * otherwise the caller ships the fp32 data as before.  Element order is kept (a channel-first fp32 batch gives channel-first bytes:
 * ingest it as [n_img * C, H, W, 1]).  `threads` (1 .. 64): the conversion runs on that many native host threads started by
 * the call (pieces of >= 64 K elements); thread-safe.                                                                         */
int mlhot_host_f32_to_u8_exact(const float* src, uint8_t* dst, int64_t n, float div, int threads, int64_t* n_inexact);

/* ---- E1: vanilla image encoder `encoder_w0` -------------------------------------------
 * replaces nn.Sequential(conv3x3s2+ReLU, conv3x3s2+ReLU, MaxPool2d(2), conv3x3s2+ReLU,
 * Flatten, Linear(4096,dim_w))   (networks/ANPShapeNet1D.py:46-56, CNPShapeNet1D.py:46-56,
 * CNPVanillaPascal1D.py:48-58, ANPVanillaPascal1D.py:50-60) for [n,1,128,128] images.
 * The image batch may come as two segments (context images, target images) that share the
 * weights; rows [0,n0) of the logical batch read img0 / write feat0, rows [n0,n0+n1) use
 * img1 / feat1 (n1 may be 0).  feat rows have leading dimension ld0 / ld1 (floats).        */
typedef struct mlhot_enc_params {
  const float *w1, *b1;   /* encoder_w0.0  [32,1,3,3],  [32] */
  const float *w2, *b2;   /* encoder_w0.2  [48,32,3,3], [48] */
  const float *w3, *b3;   /* encoder_w0.5  [64,48,3,3], [64] */
  const float *wl, *bl;   /* encoder_w0.8  [dim_w,4096], [dim_w] */
} mlhot_enc_params;
typedef struct mlhot_enc_grads {
  float *w1, *b1, *w2, *b2, *w3, *b3, *wl, *bl;
} mlhot_enc_grads;

size_t mlhot_enc_vanilla_saved_bytes(int n_img);
size_t mlhot_enc_vanilla_scratch_bytes(int n_img, int dim_w);
int mlhot_enc_vanilla_fwd(const float* img0, int n0, const float* img1, int n1, const mlhot_enc_params* p, int dim_w,
                          float* feat0, int ld0, float* feat1, int ld1,
                          void* saved, void* scratch, size_t scratch_bytes, void* stream);
int mlhot_enc_vanilla_bwd(const float* img0, int n0, const float* img1, int n1, const mlhot_enc_params* p, int dim_w,
                          const float* dfeat0, int ldd0, const float* dfeat1, int ldd1,
                          const void* saved, const mlhot_enc_grads* g, void* scratch, size_t scratch_bytes, void* stream);

/* E1's first block on its own - conv1 (1 -> 32, 3x3 s2 p1) + ReLU + conv2 (32 -> 48, 3x3 s2 p1) + ReLU + 2x2 max-pool of n
 * 128 x 128 images (networks/conv_embedding_model.py:18-31, the first five layers) - for tests and micro-benchmarks of the three
 * kernels that carry 80 % of the vanilla models' FLOPs.  `saved` has the layout and size of mlhot_enc_vanilla_saved_bytes(n): the
 * forward leaves p2 [n,48,16,16], the pool arg-max and conv1's ReLU sign bits there; the backward takes d p2 and returns the four
 * parameter gradients.  Option "conv2_split" (bit 1 forward, 2 data gradient, 4 weight gradient) selects the split-bf16 kernels. */
size_t mlhot_conv12_scratch_bytes(int n_img);
int mlhot_conv12_fwd(const float* img, int n_img, const float* w1, const float* b1, const float* w2, const float* b2,
                     void* saved, void* stream);
int mlhot_conv12_bwd(const float* img, int n_img, const float* w1, const float* b1, const float* w2, const float* dp2,
                     const void* saved, float* dw1, float* db1, float* dw2, float* db2, void* scratch, size_t scratch_bytes,
                     void* stream);

/* ---- M1 / D1 / A1 / A4: nn.Linear (+ReLU / tanh) ----------------------------------------
 * y[M,N] = act(x[M,K] w[N,K]^T + b)   (networks/models.py:27-60 EncoderFC, 195-203 AttnLinear;
 * ANPShapeNet1D.py:58-72 transform_y / r_to_z / decoder0).  b may be NULL.                  */
size_t mlhot_linear_bwd_scratch_bytes(int M, int K, int N);
int mlhot_linear_fwd(const float* x, int ldx, const float* w, const float* b, float* y, int ldy,
                     int M, int K, int N, int act, void* stream);
/* dx (+)= (dy*act'(y)) w ; dw = (dy*act'(y))^T x ; db = column sums.  dx/dw/db may be NULL.
 * M == 0 is a valid call: y and dx are left untouched, dw and db are written as zeros (the gradient of an empty sum).
 * Operands of these two entries need 4-byte alignment only and any ld >= their width: the float4 kernels are taken for
 * 16-byte aligned rows, the generic ones otherwise (tests/test_linear_abi_gpu.py runs every such route). */
int mlhot_linear_bwd(const float* x, int ldx, const float* w, const float* y, int ldy, const float* dy, int lddy,
                     int M, int K, int N, int act, float* dx, int lddx, int accumulate, float* dw, float* db,
                     void* scratch, size_t scratch_bytes, void* stream);

/* ---- M1 / D2 as chains: up to 4 Linear(+ReLU / tanh) layers on few rows (M <= 512) in ONE launch --------------------------
 * The ResNet-family models' task-side MLPs (networks/ANP.py:44-52 task_encoder + mu, models.py:139-145,182-184 fc_mu behind
 * torch.cat([x, sample_features]); ANPMRShapeNet3D.py:135-139,204-216).  Layer k computes
 *     y_k = act_k([side_k | y_{k-1}] w_k^T + b_k)   (side_first = 1)    or    act_k([y_{k-1} | side_k] w_k^T + b_k)   (side_first = 0)
 * with y_{-1} = x0 and side_k an optional second input tensor of side_w columns (the reference's torch.cat, folded: the labels
 * behind the context features, the decoder's image features in front of the sampled latent).  K = the layer's total input width
 * (side_w + the previous layer's N; 4 <= K <= 512, K % 4 == 0, side_w % 4 == 0), N <= 256 (inner layers N % 4 == 0); every y_k is
 * written to the caller's buffer (ldy >= N): the backward reads them.  All operand rows 16-byte aligned.                       */
#define MLHOT_CHAIN_MAX_LAYERS 4
typedef struct {
  const float* w; const float* b;      /* [N][K], [N] or NULL */
  int K, N, act;
  const float* side; int side_w, side_ld, side_first;   /* side_w = 0: no side input */
  float* y; int ldy;                   /* [M][ldy]: this layer's output */
} mlhot_chain_layer;
typedef struct {
  float* dw; float* db;                /* [N][K], [N] or NULL: written */
  float* g; int ldg;                   /* workspace [M][ldg], ldg >= N, ldg % 4 == 0: dy_k * act'(y_k) */
  float* dside; int dside_ld, dside_accumulate;         /* gradient of the side columns, or NULL */
} mlhot_chain_grads;
int mlhot_mlp_chain_fwd(const float* x0, int ldx0, int M, const mlhot_chain_layer* layers, int n_layers, void* stream);
/* dy[M][lddy]: gradient of the last layer's output; dx0 (NULL: not wanted) (+)= the gradient of x0's columns.  Two launches:
 * the data-gradient walk (also fills every g) and ONE weight + bias gradient launch for all layers.
 * M == 0 is a valid call of both entries (x0, side, y, g, dy may then be NULL): the forward launches nothing; the backward leaves dx0
 * and every dside untouched and writes every dw and db as zeros (the gradient of an empty sum) - its weight-gradient launch alone. */
int mlhot_mlp_chain_bwd(const float* x0, int ldx0, int M, const mlhot_chain_layer* layers, const mlhot_chain_grads* grads,
                        int n_layers, const float* dy, int lddy, float* dx0, int lddx0, int dx0_accumulate, void* stream);

/* Up to 8 INDEPENDENT few-row Linear layers in one launch (the K / V / Q head stacks of the attention, ANP.py:80-93: one
 * Linear(256 -> 8 x 256) each over the stacked head weights): forward y = act(x w^T + b); backward dx (+)= (dy act'(y)) w,
 * dw = (dy act'(y))^T x, db.  M <= 512, K % 4 == 0, rows 16-byte aligned, ldy >= N; the backward needs N % 4 == 0, lddy >= N and all
 * of dy, dx, dw.  A job with M == 0 is valid (its x, x2, y, dy, dx, dx2 may be NULL): the forward skips it (a table of such jobs
 * launches nothing); the backward leaves its dx and dx2 untouched and writes its dw and db as zeros, as mlhot_linear_bwd does.  */
typedef struct {
  const float* x; int ldx; const float* w; const float* b; float* y; int ldy; int M, K, N, act;
  const float* dy; int lddy; float* dx; int lddx, dx_accumulate; float* dw; float* db;      /* backward only */
  /* two-source input (the reference's torch.cat([x, x2], -1) in front of the layer, folded): the LAST K2 of the layer's K input
   * columns come from x2 (NULL: all K from x; K2 % 4 == 0); dx2 receives their gradient (NULL: not wanted; dx may then be NULL too) */
  const float* x2; int ldx2, K2; float* dx2; int lddx2;
} mlhot_linear_job;
int mlhot_linear_multi_fwd(const mlhot_linear_job* jobs, int n_jobs, void* stream);
int mlhot_linear_multi_bwd(const mlhot_linear_job* jobs, int n_jobs, void* stream);

/* ---- G1: per-task aggregation over the shot axis ------------------------------------------
 * mean / max / Bayesian ("baco") over dim 1 of rs[T,Nc,R]   (CNPShapeNet1D.py:78-126,
 * CondNeuralProcess.py:59-108).  baco: `rs` holds mu, `lv` the pre-softplus variance logits;
 * var = 1e-5 + softplus(lv), sigma_z = 1/(1+sum 1/var), r = sigma_z * sum(mu/var).
 * amax[T,R] (int32) receives the arg-max shot for mode MAX.                                  */
int mlhot_agg_fwd(int mode, const float* rs, const float* lv, int T, int Nc, int R,
                  float* r, float* sigma_z, int32_t* amax, void* stream);
int mlhot_agg_bwd(int mode, const float* rs, const float* lv, const float* r, const float* sigma_z, const int32_t* amax,
                  const float* dr, int T, int Nc, int R, float* drs, float* dlv, void* stream);

/* ---- A2 / A3: FAVOR+ softmax-kernel features + non-causal linear attention ----------------
 * replaces FastAttention.forward = linear_attention(softmax_kernel(q,True),
 * softmax_kernel(k,False), v)   (networks/fast_attention.py:74-99,151-156,187-205), including
 * the batch-global key stabiliser torch.max(data_dash) (fast_attention.py:97).
 * Layouts: q[T,Nq,H,d], k[T,Nc,H,d], v[T,Nc,H,d] (token-major, head-minor rows - what the head
 * projections write), proj[m,d].  out[T,Nq,d*H] is already in the reference's merged order
 * out[t,n,e*H+h] (ANPShapeNet1D.py:113-114 permute(0,2,3,1).view).                           */
size_t mlhot_favor_ws_bytes(int T, int H, int Nq, int Nc, int d, int m);
int mlhot_favor_fwd(const float* q, const float* k, const float* v, const float* proj,
                    int T, int H, int Nq, int Nc, int d, int m, float* out,
                    void* ws, size_t ws_bytes, void* stream);
/* ws must be the workspace the matching forward filled. */
int mlhot_favor_bwd(const float* q, const float* k, const float* v, const float* proj,
                    int T, int H, int Nq, int Nc, int d, int m, const float* out, const float* dout,
                    float* dq, float* dk, float* dv, void* ws, size_t ws_bytes, void* stream);
/* Above 32 shots on either side the two calls above run favor.h's operator chain (quadratic in the shot counts); with the option
 * "favor_linear" = 1 (default 0) they run the linear form instead (csrc/favor_linear.h): Ctx = F_k^T (v - c) and
 * sum_n F_k on the matrix core, out = c + F_q Ctx / (F_q . ksum), and the backward through the same [m, d] sums.  Same operands,
 * same results within the tolerances of tests/favor_linear_cases.py, same workspace query.  mlhot_favor_linear_supported reports the
 * route's envelope - max(Nq, Nc) > 32, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, GPU build - whatever the option says; the
 * staged entries below keep the older routes.  The option must not change between a forward and the backward on its workspace.
 * Added within ABI 7: bindings look the symbol up. */
int mlhot_favor_linear_supported(int T, int H, int Nq, int Nc, int d, int m);

/* ---- every context prefix of one batch, forward only (the evaluator's loss-versus-context-size sweep) -------------------
 * Row k-1 of an output is what the plain operator returns for the first k shots of every task, k = 1..Nc.
 * mlhot_agg_prefix_fwd: rs[T,Nc,R] (and lv for baco) -> r[Nc,T,R], sigma_z[Nc,T,R] (may be NULL); one pass over rs, the
 * operations of mlhot_agg_fwd in the same order.
 * mlhot_favor_prefix_fwd: out[Nc,T,Nq,d*H] in the merged order of mlhot_favor_fwd.  The batch-global key stabiliser of prefix
 * k is the maximum over the first k shots of every task only (fast_attention.py:96-97 on a batch of k shots).  Shapes (favor2.h's):
 * Nq, Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536; mlhot_favor_prefix_ws_bytes returns 0 and the call MLHOT_ERR_UNSUPPORTED for others
 * (callers loop mlhot_favor_fwd over the prefixes).  Added within ABI 7: bindings look the symbols up. */
int mlhot_agg_prefix_fwd(int mode, const float* rs, const float* lv, int T, int Nc, int R,
                         float* r, float* sigma_z, void* stream);
size_t mlhot_favor_prefix_ws_bytes(int T, int H, int Nq, int Nc, int d, int m);
int mlhot_favor_prefix_fwd(const float* q, const float* k, const float* v, const float* proj,
                           int T, int H, int Nq, int Nc, int d, int m, float* out,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- the Linears and the loss behind the prefix operators, once for all prefixes (csrc/linear_rows.h) -----------------------
 * mlhot_linear_rows_fwd: y[M,N] = act([src_0 | src_1][M, k_0 + k_1] w[N, k_0 + k_1]^T + b) with a ROW-INVARIANCE guarantee: the
 * bits of output row i depend on the input rows that map to it, on w, b, k_0, k_1, N and act - not on M, on the row's index, on
 * the grid or on the other rows of the launch (one kernel, one k order; mlhot_linear_fwd picks its kernel by M).  Output row i
 * reads row (i / rep) % period of a source (period == 0: no wrap); `ld` is the source's row stride in floats.  b may be NULL.
 * Served: k_0 > 0, k_0 % 4 == 0, k_1 % 4 == 0, 16-byte aligned source rows and w, act 0..2, any M, N >= 1 -
 * mlhot_linear_rows_supported tells for a shape; other calls return MLHOT_ERR_UNSUPPORTED and write nothing.  GPU build only.
 * mlhot_loss_prefix_fwd: loss[p] = what mlhot_loss_fwd(kind, mu + p * rows * y_dim, gt, rows, ..) writes, p < P, in one launch
 * (the same reduction order per prefix); gt is shared by the prefixes.  Added within ABI 7: bindings look the symbols up. */
typedef struct { const float* x; int ld; int k; int rep; int period; } mlhot_rows_src;
int mlhot_linear_rows_supported(int k0, int k1, int N);
int mlhot_linear_rows_fwd(const mlhot_rows_src* src, int n_src /* 1 | 2 */, const float* w, const float* b,
                          float* y, int ldy, int M, int N, int act, void* stream);
int mlhot_loss_prefix_fwd(int kind, const float* mu, const float* gt, int P, int rows, int y_dim, int gt_dim,
                          float* loss /* [P] */, void* stream);

/* ---- cached context: the key side of FAVOR+ once, the query side for any number of rows (csrc/favor_cached.h) -------------------
 * mlhot_favor_keys_fwd: k[T,Nc,H,d] (what the head projections write), proj[m,d] -> state, mlhot_favor_keys_bytes(..) bytes:
 *   floats [0, T H Nc mp): the finished key features F_k[T,H,Nc,mp] = ratio (exp(dd_k - diag_k - M) + 1e-4), mp = m rounded up to 16,
 *   features >= m zeros; float T H Nc mp: M, the key stabiliser = the maximum of dd_k over ALL T tasks of this call
 *   (fast_attention.py:96-97); the rest is the call's scratch.  A state serves queries of the same T tasks only.
 * mlhot_favor_query_fwd: q[T,Nq,H,d], state, v[T,Nc,H,d], proj -> out[T,Nq,d*H] in mlhot_favor_fwd's merged order, for ANY Nq >= 1
 *   in one launch, with a ROW-INVARIANCE guarantee: the bits of out[t,n,:] depend on q[t,n], state, v, proj and the dimensions -
 *   not on Nq, on n, on the grid or on the other query rows (so a caller may chunk, pad or reorder the rows freely).
 * mlhot_favor_query_weights_fwd: mlhot_favor_query_fwd that also reads out FAVOR+'s implied attention,
 *   w[T,H,Nq,Nc] contiguous fp32 (row length Nc), w[t,h,n,n'] = S[n,n'] / D[n] with the S = F_q F_k^T and D = rowsum(S) the launch
 *   forms for out = S V / D: every w >= 0, sum_n' w = 1 and out[t,n,e*H+h] = sum_n' w[t,h,n,n'] v[t,n',h,e] up to rounding.  It is
 *   FAVOR+'s own weighting - the 1e-4 floors and the state's batch-global stabiliser included - not a softmax.  Against a masked
 *   state (mlhot_favor_keys_ragged_fwd) the columns n' >= lens[t] are exactly 0.0f.  w carries out's ROW-INVARIANCE guarantee (one
 *   IEEE divide per element, the same at every row of a tile), and out is BIT-EQUAL to mlhot_favor_query_fwd's on the same
 *   arguments.  Envelope, workspace (mlhot_favor_query_ws_bytes), alignment of q / state / v / proj / out and error codes are
 *   mlhot_favor_query_fwd's; w needs 4-byte alignment only; w == NULL is MLHOT_ERR_ARG; unsupported shapes write neither out nor w.
 * Shapes: Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536 (favor2.h's, on the context side), 16-byte aligned pointers; for others
 * the _bytes functions return 0 and the calls MLHOT_ERR_UNSUPPORTED, writing nothing (callers keep k and run mlhot_favor_fwd).
 * Forward only; GPU build only.  Added within ABI 7: bindings look the symbols up. */
size_t mlhot_favor_keys_bytes(int T, int H, int Nc, int d, int m);
int mlhot_favor_keys_fwd(const float* k, const float* proj, int T, int H, int Nc, int d, int m,
                         void* state, size_t state_bytes, void* stream);
size_t mlhot_favor_query_ws_bytes(int T, int H, int Nq, int Nc, int d, int m);
int mlhot_favor_query_fwd(const float* q, const void* state, const float* v, const float* proj,
                          int T, int H, int Nq, int Nc, int d, int m, float* out,
                          void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_weights_fwd(const float* q, const void* state, const float* v, const float* proj,
                                  int T, int H, int Nq, int Nc, int d, int m, float* out, float* w /* [T,H,Nq,Nc] */,
                                  void* ws, size_t ws_bytes, void* stream);

/* ---- cached context with per-task context sizes: the masked key state (csrc/favor_cached.h) ---------------------
 * mlhot_favor_keys_ragged_fwd: mlhot_favor_keys_fwd with lens[T] (int32, DEVICE memory, read on the device: no host synchronisation,
 *   the call stays capturable).  Row n of task t is a context shot iff n < lens[t], 1 <= lens[t] <= Nc (the caller's contract; the
 *   kernels hold a value outside it to that range).  Layout, mlhot_favor_keys_bytes and envelope are mlhot_favor_keys_fwd's: F_k first,
 *   then M.  M is the maximum of dd_k over the VALID rows of all T tasks; valid rows hold ratio (exp(dd_k - diag_k - M) + 1e-4), every
 *   feature (all mp) of an invalid row is exactly 0.0f.  An invalid row of k is never read - it may hold anything, NaN and Inf
 *   included.  With lens[t] == Nc for every t the state equals mlhot_favor_keys_fwd's bit for bit.
 * What a zero row means to the query kernels (mlhot_favor_query_fwd, mlhot_np_query_fwd, both unchanged): its column of
 *   S = F_q F_k^T is exactly 0, so it adds nothing to D = rowsum(S) nor to out = S V / D - the state serves them as any other, with
 *   the row invariance they guarantee.  v's invalid rows must be FINITE (callers zero-fill them): S is exactly 0 there, and
 *   0 x NaN is not.
 * lens == NULL: MLHOT_ERR_ARG.  Outside the envelope: MLHOT_ERR_UNSUPPORTED, nothing written (there is no masked form of
 * mlhot_favor_fwd to fall back on).  Forward only; GPU build only.  Added within ABI 7: bindings look the symbol up. */
int mlhot_favor_keys_ragged_fwd(const float* k, const float* proj, const int32_t* lens /* [T], device */,
                                int T, int H, int Nc, int d, int m, void* state, size_t state_bytes, void* stream);

/* ---- cached context of the vanilla family: everything behind the encoder that sees the targets, ONE launch (csrc/np_query.h) ------
 * mlhot_np_query_fwd: x_qry[T*Nq,dim_w] (the encoder's target rows) -> mu[T*Nq,y_dim] against a conditioned context, any Nq >= 1:
 *   attention models with d->Nc > 0: key_state = mlhot_favor_keys_fwd's state for (T, 8 heads, Nc, dim_w, m_feat) and vh[T,Nc,8,dim_w]
 *     (z NULL): per head the query projection, the query features, S V / D into the merged tile, then _W, r_to_z and decoder0;
 *   every other case: z[T,dim_z] (the aggregated context through r_to_z, or zeros without a context shot; key_state, vh NULL):
 *     decoder0([x | z[t]]).
 * Grid task x 16-row target tile, no workspace, with the ROW-INVARIANCE guarantee of mlhot_favor_query_fwd: the bits of mu[t,n,:]
 * depend on x_qry[t,n], the state, the parameters and the dimensions only.  d->Nq is ignored; of p the query-side fields are read
 * (wq_*, wo_*, r2z_*, dec_*, proj).  Served (mlhot_np_query_supported): dim_w % 16 == 0, dim_w <= 64, dim_z % 4 == 0, dim_z <= 64,
 * dec_hidden % 4 == 0, dec_hidden <= 128, y_dim <= 16 and, for the attention, dim_r == dim_w, Nc <= 32, 16 <= m_feat <= 272; 16-byte
 * aligned pointers.  Otherwise MLHOT_ERR_UNSUPPORTED, nothing written.  Forward only; GPU build only.  Added within ABI 7: bindings
 * look the symbols up.  (mlhot_np_dims / mlhot_np_params: "whole vanilla CNP/ANP model" below.) */
struct mlhot_np_dims;
struct mlhot_np_params;
int mlhot_np_query_supported(const struct mlhot_np_dims* d);
int mlhot_np_query_fwd(const struct mlhot_np_dims* d, const struct mlhot_np_params* p, const float* x_qry, int Nq,
                       const void* key_state, const float* vh, const float* z, float* mu, void* stream);

/* ---- the same tail against a FAVOR+ summary state: any number of context shots, ONE launch (csrc/np_query_summary.h)
 * mlhot_np_query_summary_fwd: x_qry[T*Nq,dim_w] -> mu[T*Nq,y_dim] for an attention model against summary_state, the state of
 *   mlhot_favor_summary_bytes(T, 8, dim_w, m_feat) bytes exactly as mlhot_favor_summary_absorb, _merge and _gather leave it: per head
 *   the query projection, the query features, (F_q A + eps vs sum F_q) / (F_q a + eps cnt sum F_q) with A streamed from memory into
 *   the merged tile, then _W, r_to_z and decoder0.  Launch label np.query.summary.
 * Grid task x 16-row target tile, no workspace, no atomics, with the ROW-INVARIANCE guarantee of mlhot_favor_query_fwd: the bits of
 * mu[t,n,:] depend on x_qry[t,n], the state, the parameters and the dimensions only.  d->Nc and d->Nq are ignored; of p the
 * query-side fields are read (wq_*, wo_*, r2z_*, dec_*, proj).  Served (mlhot_np_query_summary_supported): agg_mode attention and
 * mlhot_np_query_supported's conditions without the Nc clause - dim_w % 16 == 0, dim_w <= 64, dim_z % 4 == 0, dim_z <= 64,
 * dec_hidden % 4 == 0, dec_hidden <= 128, y_dim <= 16, dim_r == dim_w, 16 <= m_feat <= 272; 16-byte aligned pointers (mu included).
 * Otherwise MLHOT_ERR_UNSUPPORTED, nothing written; a NULL pointer or Nq < 1: MLHOT_ERR_ARG, nothing written.  A task whose cnt is 0
 * has no defined output (0 / 0), as for mlhot_favor_summary_query_fwd: the caller refuses it.  Forward only; GPU build only.  Added
 * within ABI 7: bindings look the symbols up. */
int mlhot_np_query_summary_supported(const struct mlhot_np_dims* d);
int mlhot_np_query_summary_fwd(const struct mlhot_np_dims* d, const struct mlhot_np_params* p, const float* x_qry, int Nq,
                               const void* summary_state, float* mu, void* stream);

/* ---- prefix sweep of the vanilla family: the query tail for K context prefixes in one launch (csrc/np_prefix.h) ---
 * mlhot_np_prefix_fwd: x_qry[T*Nq,dim_w] -> mu[K,T,Nq,y_dim]; mu[i] is mlhot_np_query_fwd's result against the first ks[i] of the
 *   d->Nc context shots of every task.  ks: K ints in HOST memory, strictly increasing, 1 <= ks[i] <= d->Nc (else MLHOT_ERR_ARG).
 *   attention models: kh, vh[T,Nc,8,dim_w] (the head projections of all shots; z NULL) and ws of mlhot_np_prefix_ws_bytes bytes; the
 *     call runs the key side itself (two launches into ws), then the sweep launch;
 *   every other model: z[K,T,dim_z] (the aggregate of each prefix through r_to_z; kh, vh, ws NULL): the sweep launch alone.
 * INVARIANCE: the bits of mu[i,t,n,:] depend on x_qry[t,n], the first ks[i] shots of the batch, the parameters and the dimensions
 * only - not on Nq, on n, on the other target rows or on which other prefixes were requested.  Served (mlhot_np_prefix_supported):
 * mlhot_np_query_supported(d), 1 <= K <= 32, 1 <= Nc <= 32; 16-byte aligned pointers.  Otherwise MLHOT_ERR_UNSUPPORTED, nothing
 * written.  d->Nq is ignored.  Forward only, test mode; GPU build only.  Added within ABI 7: bindings look the symbols up. */
int mlhot_np_prefix_supported(const struct mlhot_np_dims* d, int K);
size_t mlhot_np_prefix_ws_bytes(const struct mlhot_np_dims* d, int K);
int mlhot_np_prefix_fwd(const struct mlhot_np_dims* d, const struct mlhot_np_params* p, const float* x_qry, int Nq,
                        const int32_t* ks /* [K], host */, int K, const float* kh, const float* vh, const float* z,
                        float* mu, void* ws, size_t ws_bytes, void* stream);

/* ---- cached context beyond 32 shots: a fixed-size FAVOR+ summary state (csrc/favor_summary.h) ---------------------
 * FAVOR+ is a linear attention, so the context enters the output only through sums over the shots.  With dd[n,j] = (c k_n) . P_j,
 * diag[n] = |k_n|^2 c^2 / 2, c = d^-1/4, eps = 1e-4 and M = the maximum of dd over every valid shot of all T tasks, all heads and all
 * features absorbed so far (fast_attention.py:96-97), the state of mlhot_favor_summary_bytes(T, H, d, m) bytes holds, as floats:
 *   A   [T,H,mp,d]  at 0:                     A[j,e] = sum_n exp(dd[n,j] - diag[n] - M) v[n,e]    (mp = m rounded up to 16)
 *   a   [T,H,mp]    behind A:                 a[j]   = sum_n exp(dd[n,j] - diag[n] - M)
 *   vs  [T,H,d]     behind a:                 vs[e]  = sum_n v[n,e]
 *   M   one float, in a block of 16, behind vs   (kept ONCE per state)
 *   cnt [T,H] int32 behind M's block:         the shots absorbed by task t (the same for every head)
 * Features >= m of A and a are exact zeros.  The size does not depend on the number of shots.
 * mlhot_favor_summary_init: the fresh state - M = -inf, everything else 0.
 * mlhot_favor_summary_absorb: k, v [T,n,H,d] (n <= 32 NEW shots per task; callers chunk), proj[m,d]; lens[T] (int32, DEVICE memory,
 *   may be NULL = n for every task) = the valid new shots per task, 0 .. n (a value outside is held to that range).  A row at or
 *   behind lens[t] of k AND of v is never read - it may hold NaN or Inf.  M' = max(M, max dd of the valid new shots of ALL tasks and
 *   heads); A <- exp(M - M') A + sum_new exp(dd - diag - M') v, a likewise; vs += sum_new v; cnt += lens.  state_in and state_out may be
 *   the same pointer (otherwise state_in is left as it is).  ws: mlhot_favor_summary_ws_bytes(T, H, n, d, m) bytes.  Two launches, no
 *   atomics: every summation order is a function of the dimensions alone, so the same call sequence gives the same bits.
 * mlhot_favor_summary_query_fwd: q[T,Nq,H,d], state, proj -> out[T,Nq,d*H] in mlhot_favor_fwd's merged order, ONE launch for any Nq:
 *   out[q,e] = sum_j F_q[q,j] (A[j,e] + eps vs[e]) / sum_j F_q[q,j] (a[j] + eps cnt), F_q as mlhot_favor_query_fwd computes it - equal
 *   to mlhot_favor_fwd on the concatenated shots in exact arithmetic.  ROW-INVARIANCE guarantee of mlhot_favor_query_fwd: the bits
 *   of out[t,n,:] depend on q[t,n], the state, proj and the dimensions only.  A task with cnt == 0 has no defined output (0 / 0).
 * Shapes: d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, any number of shots; 16-byte aligned pointers.  For others the _bytes
 * functions return 0 and the calls MLHOT_ERR_UNSUPPORTED, writing nothing.  Forward only; GPU build only.  Added within ABI 7:
 * bindings look the symbols up. */
size_t mlhot_favor_summary_bytes(int T, int H, int d, int m);
size_t mlhot_favor_summary_ws_bytes(int T, int H, int n, int d, int m);
int mlhot_favor_summary_init(int T, int H, int d, int m, void* state, size_t state_bytes, void* stream);
int mlhot_favor_summary_absorb(const float* k, const float* v, const float* proj, const int32_t* lens /* [T], device, or NULL */,
                               int T, int H, int n, int d, int m, const void* state_in, void* state_out, size_t state_bytes,
                               void* ws, size_t ws_bytes, void* stream);
size_t mlhot_favor_summary_query_ws_bytes(int T, int H, int Nq, int d, int m);
int mlhot_favor_summary_query_fwd(const float* q, const void* state, const float* proj, int T, int H, int Nq, int d, int m,
                                  float* out, void* ws, size_t ws_bytes, void* stream);
/* mlhot_favor_summary_merge: n summary states of the same (T, H, d, m) that were absorbed apart -> out, the state
 *   of all their shots.  states: n device pointers in HOST memory, 1 <= n <= 8 (callers fold more in groups); m_floor: ONE float in
 *   DEVICE memory or NULL - "the stabiliser is at least this".  All fp32:  M' = max(M_0 .. M_{n-1}, *m_floor);  s_i = 1.0f exactly
 *   where M_i == M' (also when both are -inf), else expf(M_i - M') - 0 for a fresh state against a finite M';  A' = sum_i s_i A_i and
 *   a' likewise, ONE chain per element in the order i = 0, 1, .. (a function of n alone; no atomics);  vs' = sum_i vs_i and
 *   cnt' = sum_i cnt_i (int32) in the same order.  Features >= m come out as exact zeros and EVERY float of out is written (M's
 *   block and cnt's padding as mlhot_favor_summary_init leaves them), whatever out held.  The inputs are only read.  out must be a
 *   buffer of its own: one that overlaps an input is MLHOT_ERR_ARG.  state_bytes must equal mlhot_favor_summary_bytes(T, H, d, m)
 *   (else MLHOT_ERR_WORKSPACE).  One launch; equal to absorbing all the shots into one state in exact arithmetic, one stabiliser
 *   for the whole (fast_attention.py:96-97).  Outside the shapes above or 1 .. 8 states: MLHOT_ERR_UNSUPPORTED.  Whatever is
 *   refused writes nothing.  GPU build only.  Added within ABI 7: bindings look the symbol up. */
int mlhot_favor_summary_merge(const void* const* states /* host array of n device pointers */, int n,
                              const float* m_floor /* one float, DEVICE memory, may be NULL */,
                              int T, int H, int d, int m, void* out, size_t state_bytes, void* stream);
/* mlhot_favor_summary_gather: merge with a row per task.  n summary states of the same (H, d, m), 1 <= n <= 8, state i
 *   with its own task count state_tasks[i] (both arrays in HOST memory) -> out, a state of T_out tasks.  parts: int32 [T_out][P][2] in
 *   DEVICE memory, 1 <= P <= 8, 8-byte aligned; entry (i, u) of row t means "task u of state i is a part of output task t", i < 0 ends
 *   the row.  The kernel reads the table itself - no host synchronisation, the call can be captured - and holds i to 0 .. n - 1 and u
 *   to 0 .. state_tasks[i] - 1, so no table content reads out of bounds; whether the table means what the caller wants is the
 *   caller's to check.  M' = max(M_0 .. M_{n-1}, *m_floor) over EVERY state passed, whether a part names it or not;  s_i as in merge
 *   (1.0f exactly where M_i == M', also when both are -inf);  A'[t,h] = sum_p s_{i_p} A_{i_p}[u_p,h] and a' likewise, vs' and cnt'
 *   plain sums, ONE chain per element over the row's parts in table order, through the fold step of merge: the same parts in the
 *   same order give merge's bits.  A task without a part gets the rows of a fresh state (zeros, cnt 0).  EVERY float of out is
 *   written (features >= m zeros by index, M's block M' and zeros, cnt's padding zeros), whatever out held; an input's paddings are
 *   never trusted.  One launch over the slots of out.  MLHOT_ERR_ARG, nothing written: out overlaps an input, state_bytes is not
 *   mlhot_favor_summary_bytes(T_out, H, d, m), n or P outside 1 .. 8.  Outside the shapes above for T_out or a state_tasks[i]:
 *   MLHOT_ERR_UNSUPPORTED.  GPU build only.  Added within ABI 7: bindings look the symbol up. */
int mlhot_favor_summary_gather(const void* const* states /* host array of n device pointers */,
                               const int* state_tasks /* host array of n task counts */, int n,
                               const int32_t* parts /* [T_out][P][2], DEVICE memory */, int P,
                               const float* m_floor /* one float, DEVICE memory, may be NULL */,
                               int T_out, int H, int d, int m, void* out, size_t state_bytes, void* stream);
/* mlhot_favor_summary_retract: mlhot_favor_summary_absorb's argument list with the sign turned - k, v [T,n,H,d] are
 *   shots that were absorbed into state_in EARLIER (n <= 32 per task and call; lens as for absorb, 0 .. n) and are taken out again.
 *   M stays as it is (no rescale; the stabiliser of a summary never falls);  e[n,j] = exp(min(dd[n,j] - M, 0) - diag[n]) - for a shot
 *   that was absorbed dd <= M holds and the min does nothing;  A <- A - sum_n e v,  a <- max(a - sum_n e, 0),  vs -= sum_n v,
 *   cnt -= lens.  In exact arithmetic the result is the state absorbed from the remaining shots with the M of the larger set; in
 *   fp32 the subtraction rounds at the scale of the state BEFORE the retraction.  A shot that was never absorbed gives a result
 *   that is undefined in value but finite (e <= 1).  That cnt stays >= 0 is the caller's to see to.  state_in and state_out may be the
 *   same pointer (in place, bit-equal to the call with a buffer of its own; otherwise state_in is left as it is, and a partial
 *   overlap is MLHOT_ERR_ARG).  ws: mlhot_favor_summary_ws_bytes(T, H, n, d, m) bytes.  Two launches (labels favor.sum_retract1 - absorb's
 *   first launch as it is - and favor.sum_retract2), no atomics, every summation order a function of the dimensions alone.  Shapes and
 *   error codes as for absorb; whatever is refused writes nothing.  GPU build only.  Added within ABI 8: bindings look the symbol up. */
int mlhot_favor_summary_retract(const float* k, const float* v, const float* proj, const int32_t* lens /* [T], device, or NULL */,
                                int T, int H, int n, int d, int m, const void* state_in, void* state_out, size_t state_bytes,
                                void* ws, size_t ws_bytes, void* stream);

/* ---- prefix sweep beyond 32 context shots: chunked running FAVOR+ prefixes (csrc/favor_prefix_long.h) -------------
 * mlhot_favor_prefix_long_fwd: q[T,Nq,H,d], k, v[T,Nc,H,d], proj[m,d] -> out[K,T,Nq,d*H] in mlhot_favor_fwd's merged order; out[i]
 *   is mlhot_favor_fwd on the first ks[i] shots of every task in exact arithmetic, its batch-global key stabiliser included: prefix i
 *   uses M_i = the maximum of dd over the valid shots < ks[i] of ALL tasks, heads and features (fast_attention.py:96-97), and the key
 *   feature's +1e-4 floor relative to M_i.  ks: K ints in HOST memory, strictly increasing, 1 <= ks[i] <= Nc (else MLHOT_ERR_ARG).
 *   lens[T] (int32, DEVICE memory, read on the device; may be NULL = Nc for every task): task t's context is its first lens[t] shots,
 *   1 <= lens[t] <= Nc (the caller's contract; a value outside is held to 0 .. Nc, and a task without a shot has no defined output);
 *   a prefix size above lens[t] saturates at lens[t] for that task while M_i still follows every task's valid shots < ks[i].  A row at
 *   or behind lens[t] of k AND of v is never read - it may hold NaN or Inf.
 *   Three launches, no atomics, no [mp x d] state: the shots are walked in chunks of 32 with running sums relative to the running
 *   maximum (rescaled by exp(M_old - M_new) <= 1).  Every summation order is a function of the dimensions and of ks[i] alone, so
 *   out[i] has the same bits whichever other prefixes are asked for, and the ROW-INVARIANCE guarantee of mlhot_favor_query_fwd holds:
 *   the bits of out[i,t,n,:] depend on q[t,n], the first ks[i] shots of the batch, proj and the dimensions only.
 * Served (mlhot_favor_prefix_long_supported): d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, 1 <= K <= 64, any Nc >= 1, any Nq >= 1
 * (T H < 2^20; T H ceil(Nc / 32) and T H ceil(Nq / 16) below 2^31); 16-byte aligned pointers; ws of
 * mlhot_favor_prefix_long_workspace_bytes bytes (0 for a shape not served).  Otherwise MLHOT_ERR_UNSUPPORTED, nothing written.
 * Forward only; GPU build only.  Added within ABI 7: bindings look the symbols up. */
int mlhot_favor_prefix_long_supported(int T, int H, int Nq, int Nc, int d, int m, int K);
size_t mlhot_favor_prefix_long_workspace_bytes(int T, int H, int Nq, int Nc, int d, int m, int K);
int mlhot_favor_prefix_long_fwd(const float* q, const float* k, const float* v, const float* proj,
                                const int32_t* ks /* [K], host */, int K, const int32_t* lens /* [T], device, or NULL */,
                                int T, int H, int Nq, int Nc, int d, int m, float* out,
                                void* ws, size_t ws_bytes, void* stream);

/* ---- per-shot key states beyond 32 context slots: chunked keys and query with read-out (csrc/favor_long.h) ---------
 * The split of mlhot_favor_keys_fwd / mlhot_favor_query_fwd with the context slots walked in chunks of 32, 1 <= Nc <= 256 slots per
 * task.  The state keeps the finished key features of every slot, so the query can read out FAVOR+'s per-shot weights.
 * mlhot_favor_keys_long_fwd: k[T,Nc,H,d], proj[m,d], lens[T] (int32, DEVICE memory, read on the device; NULL = Nc for every task;
 *   1 <= lens[t] <= Nc is the caller's contract, a value outside is held to that range) -> state of mlhot_favor_keys_long_bytes bytes:
 *   floats [0, T H Nc mp): F_k[T,H,Nc,mp] as mlhot_favor_keys_fwd lays it out, float T H Nc mp: M, the maximum of dd_k over the VALID
 *   rows of all T tasks; the rest is the call's scratch.  Rows n >= lens[t] of k are never read and all mp features of such a row of
 *   F_k are exactly 0.0f; every float of F_k and M is written, whatever the buffer held.  Two launches.
 * mlhot_favor_query_long_fwd: q[T,Nq,H,d], that state, v[T,Nc,H,d], proj, the SAME lens (or NULL) -> out[T,Nq,d*H] in
 *   mlhot_favor_fwd's merged order, ONE launch for any Nq >= 1; with w != NULL also w[T,H,Nq,Nc] = S / D as
 *   mlhot_favor_query_weights_fwd defines it, columns n' >= lens[t] exactly 0.0f, and out BIT-EQUAL to the call with w == NULL.
 *   Rows n >= lens[t] of v are never read.  ROW-INVARIANCE guarantee of mlhot_favor_query_fwd for out and w.  Every summation order
 *   is a function of d, m and lens[t] alone (no atomics): the same shots kept at another capacity Nc give the same bits, and with
 *   Nc <= 32 state, out and w are BIT-EQUAL to mlhot_favor_keys_fwd / mlhot_favor_query_weights_fwd on the same operands.
 *   ws: at least 256 bytes (the kernel works in LDS alone).
 * Served (mlhot_favor_long_supported): 1 <= Nc <= 256, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, T H < 2^20,
 * T H ceil(Nq / 16) < 2^31, 16-byte aligned q, k, proj and state.  Otherwise mlhot_favor_keys_long_bytes returns 0 and the calls
 * MLHOT_ERR_UNSUPPORTED, writing nothing.  Forward only; GPU build only.  Added within ABI 7: bindings look the symbols up. */
int mlhot_favor_long_supported(int T, int H, int Nc, int d, int m);
size_t mlhot_favor_keys_long_bytes(int T, int H, int Nc, int d, int m);
int mlhot_favor_keys_long_fwd(const float* k, const float* proj, const int32_t* lens /* [T], device, or NULL */,
                              int T, int H, int Nc, int d, int m, void* state, size_t state_bytes, void* stream);
int mlhot_favor_query_long_fwd(const float* q, const void* state, const float* v, const float* proj,
                               const int32_t* lens /* [T], device, or NULL */, int T, int H, int Nq, int Nc, int d, int m,
                               float* out, float* w /* [T,H,Nq,Nc], or NULL */, void* ws, size_t ws_bytes, void* stream);

/* ---- per-target context masks: one query pass, G masked read-outs (csrc/favor_cached.h, csrc/favor_long.h) -------
 * mlhot_favor_query_masked_fwd serves a mlhot_favor_keys_fwd / _ragged_fwd state (Nc <= 32), mlhot_favor_query_long_masked_fwd a
 * mlhot_favor_keys_long_fwd state (Nc <= 256, the SAME lens or NULL).  The arguments are the unmasked entry's plus
 *   mask_words[T,G,Nq,W] (uint32, DEVICE memory, W = ceil(Nc / 32)): bit j of word c is context slot 32 c + j of that (task, group,
 *   target row); all heads share it; bits at slots >= Nc are ignored; a slot counts iff its bit is set AND it is a valid shot of
 *   the state (n' < lens[t]).  G >= 1 groups of masks over the same targets.
 * -> out[T,G,Nq,d*H] in mlhot_favor_fwd's merged order, out_g = (S o mask_g) V / D_g with D_g = rowsum(S o mask_g); with w != NULL
 *   also w[T,G,H,Nq,Nc] = (S o mask_g) / D_g, masked columns exactly 0.0f, and out BIT-EQUAL to the call with w == NULL.
 *   ONE launch for any Nq and G: q's features and S are formed once per 16-row tile, whatever G; the G read-outs loop inside the
 *   workgroup.  Every masked sum is the sum of the kept columns in the unmasked order (a dropped column adds +0.0f in its place) -
 *   never "full minus masked" - so one dominant shot cancels nothing.  No atomics; every summation order is a function of the
 *   dimensions (and of lens[t]) alone.  The mask does not move the key stabiliser: M stays the state's.
 *   A (row, group) whose mask keeps no valid slot gets exact zeros in out and w, never NaN.
 *   ROW and GROUP INVARIANCE: the bits of out[t,g,n,:] and w[t,g,:,n,:] depend on q[t,n], state, v, proj, the dimensions and the
 *   mask words of (t,g,n) - not on Nq, G, n, g, the grid or other rows or groups.  With every bit set, out and w of every group
 *   are BIT-EQUAL to mlhot_favor_query_weights_fwd / mlhot_favor_query_long_fwd on the same arguments.
 * Envelope, alignment, workspace (mlhot_favor_query_ws_bytes; 256 bytes for the long entry - no LDS or workspace beyond the
 * unmasked kernels') and error codes are the unmasked entry's; mask_words and w need 4-byte alignment; mask_words == NULL or G < 1
 * is MLHOT_ERR_ARG; unsupported shapes write nothing.  Forward only; GPU build only.  Added within ABI 7: bindings look the symbols up. */
int mlhot_favor_query_masked_fwd(const float* q, const void* state, const float* v, const float* proj,
                                 const uint32_t* mask_words /* [T,G,Nq,1], device */, int G,
                                 int T, int H, int Nq, int Nc, int d, int m, float* out /* [T,G,Nq,d*H] */,
                                 float* w /* [T,G,H,Nq,Nc], or NULL */, void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_long_masked_fwd(const float* q, const void* state, const float* v, const float* proj,
                                      const int32_t* lens /* [T], device, or NULL */,
                                      const uint32_t* mask_words /* [T,G,Nq,ceil(Nc/32)], device */, int G,
                                      int T, int H, int Nq, int Nc, int d, int m, float* out /* [T,G,Nq,d*H] */,
                                      float* w /* [T,G,H,Nq,Nc], or NULL */, void* ws, size_t ws_bytes, void* stream);

/* ---- per-shot key states beyond 256 context slots: the query walks PAGES of 256 slots (csrc/favor_paged.h) ---------
 * A form of its own beside the long entries, which keep their envelope: 1 <= Nc <= 4096 (csrc's FAVOR_PAGED_MAXNC - an envelope decision,
 * F_k and w grow linearly with Nc) slots per task.
 * mlhot_favor_keys_paged_fwd: arguments, state layout (mlhot_favor_keys_paged_bytes bytes), lens and contract are
 *   mlhot_favor_keys_long_fwd's - rows n >= lens[t] of k are never read and are exact zeros in F_k, every float of F_k and M is
 *   written, M is the maximum over the valid rows of all tasks.  The same two launches.
 * mlhot_favor_query_paged_fwd: mlhot_favor_query_long_fwd's arguments and contract - out[T,Nq,d*H], ONE launch for any Nq >= 1;
 *   with w != NULL also w[T,H,Nq,Nc] = S / D, columns n' >= lens[t] exactly 0.0f, out BIT-EQUAL to the call with w == NULL.  D and
 *   the chains of out run on over the pages, each ONE chain over the slots in ascending order (never a sum of page sums).
 * mlhot_favor_query_paged_masked_fwd: mlhot_favor_query_long_masked_fwd's arguments and contract - mask_words[T,G,Nq,ceil(Nc/32)],
 *   out[T,G,Nq,d*H], w[T,G,H,Nq,Nc]; D_g is the sum of the kept columns in the unmasked order (+0.0f in a dropped column's place);
 *   a (row, group) that keeps no valid slot gets exact zeros; with every bit set the result is BIT-EQUAL to the unmasked entry's.
 * ws: mlhot_favor_query_paged_bytes(T, H, Nq, Nc, d, m, G) bytes, G = 0 for the unmasked entry (256: the kernel works in LDS
 *   alone), G >= 1 for the masked one (D_g between the pages: T H ceil(Nq / 16) G 16 floats); 4-byte aligned; its contents are the
 *   call's scratch.  Between the pages the masked entry also keeps the unnormalised out_g in out and both entries the
 *   unnormalised S in w: both buffers hold their results when the call is done.
 * BITS: every summation order is a function of d, m and lens[t] alone (no atomics).  The bits of out[t,n] and w[t,:,n] (masked:
 *   of [t,g,n]) depend on q[t,n], the state, v, proj, the dimensions, lens[t] and that row's mask words - not on Nq, G, the other
 *   rows or groups, the grid or the capacity Nc the same shots are kept in.  With Nc <= 256 state, out and w are BIT-EQUAL to the
 *   long entries' on the same operands.
 * Served (mlhot_favor_paged_supported): 1 <= Nc <= 4096, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, T H < 2^20, T Nc < 2^31,
 * T H ceil(Nq / 16) < 2^31, 16-byte aligned q, k, proj and state.  Otherwise the _bytes entries return 0 and the calls
 * MLHOT_ERR_UNSUPPORTED, writing nothing; mask_words == NULL or G < 1 is MLHOT_ERR_ARG.  Forward only; GPU build only.  Added
 * within ABI 7: bindings look the symbols up. */
int mlhot_favor_paged_supported(int T, int H, int Nc, int d, int m);
size_t mlhot_favor_keys_paged_bytes(int T, int H, int Nc, int d, int m);
size_t mlhot_favor_query_paged_bytes(int T, int H, int Nq, int Nc, int d, int m, int G /* 0: the unmasked entry */);
int mlhot_favor_keys_paged_fwd(const float* k, const float* proj, const int32_t* lens /* [T], device, or NULL */,
                               int T, int H, int Nc, int d, int m, void* state, size_t state_bytes, void* stream);
int mlhot_favor_query_paged_fwd(const float* q, const void* state, const float* v, const float* proj,
                                const int32_t* lens /* [T], device, or NULL */, int T, int H, int Nq, int Nc, int d, int m,
                                float* out, float* w /* [T,H,Nq,Nc], or NULL */, void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_paged_masked_fwd(const float* q, const void* state, const float* v, const float* proj,
                                       const int32_t* lens /* [T], device, or NULL */,
                                       const uint32_t* mask_words /* [T,G,Nq,ceil(Nc/32)], device */, int G,
                                       int T, int H, int Nq, int Nc, int d, int m, float* out /* [T,G,Nq,d*H] */,
                                       float* w /* [T,G,H,Nq,Nc], or NULL */, void* ws, size_t ws_bytes, void* stream);

/* ---- attention mass per context slot: the read-out reduced over the targets inside the query launch (csrc/favor_mass.h)
 *     mass[t,h,c] = sum over targets n of  tw[t,n] * w[t,h,n,c],   w = S / D exactly as mlhot_favor_query_weights_fwd defines it,
 * without w[T,H,Nq,Nc] being allocated or written in any form.  mlhot_favor_query_mass_fwd serves a mlhot_favor_keys_fwd / _ragged_fwd
 * state (Nc <= 32), mlhot_favor_query_long_mass_fwd a mlhot_favor_keys_long_fwd state (Nc <= 256), mlhot_favor_query_paged_mass_fwd a
 * mlhot_favor_keys_paged_fwd state (Nc <= 4096).  The arguments are the unmasked entry's (mlhot_favor_query_fwd / _long_fwd /
 * _paged_fwd without w) plus
 *   tw[T,Nq] (fp32, DEVICE memory, finite and >= 0 - the caller's to check) or NULL: the plain column sum;
 *   mass and fold: fold != 0 -> mass[T,H,Nc], and ws (mlhot_favor_query_mass_bytes bytes) holds the tile partials;
 *                  fold == 0 -> mass IS the tile partials part[T,H,ceil(Nq/16),Nc], nothing is folded and ws is the 256-byte token
 *                  block: a caller that splits the targets at multiples of 16 concatenates the pieces' partials along the tile
 *                  axis and folds ONCE with mlhot_favor_mass_fold(part, T*H, tiles, Nc, mass) - the single call's bits.
 * out is BIT-EQUAL to the entry without mass on the same arguments: the mass is one more store behind D, as w is.
 * SUMMATION ORDER (no atomics): every (task, head, 16-row tile) workgroup adds its rows' terms per column in ascending row order from
 *   +0.0f into its tile partial; the fold adds the tile partials per column in ascending tile order from +0.0f.  A term is the
 *   read-out's own single IEEE divide S / D; with tw it is ONE rounded multiply tw * w, then ONE rounded add - no FMA contraction
 *   is used (the functions that add are compiled with `#pragma clang fp contract(off)`).  So with tw == NULL
 *   mass is the fp32 fold, in that order, of the bits the read-out entry stores into w on the same arguments.
 * Columns c >= lens[t] are exactly 0.0f; rows n >= lens[t] of v are never read by the long and paged entries (the keys entry reads
 *   v as mlhot_favor_query_fwd does: zero-fill them).  The bits do not depend on the capacity Nc the same shots are kept in
 *   (long, paged); a paged state of at most 256 slots gives the long entry's bits, a long state of at most 32 the keys entry's.
 * The paged entry walks the pages twice: D is final behind the last page only, so S of every page but the last is formed again
 *   and reduced with the final D (the last page is reduced from LDS).
 * MEMORY: mlhot_favor_query_mass_bytes(T, H, Nq, Nc, d, m) = T H ceil(Nq/16) Nc floats (in blocks of 256 bytes), 1/16 of w - everything this
 *   path writes beside out and mass.  0 for a shape none of the three serves.
 * Envelope, alignment and error codes are those of the entry each one extends; tw, mass and ws need 4-byte alignment; mass == NULL is
 * MLHOT_ERR_ARG; unsupported shapes write nothing.  Forward only; GPU build only.  Added within ABI 8: bindings look the symbols up. */
size_t mlhot_favor_query_mass_bytes(int T, int H, int Nq, int Nc, int d, int m);
int mlhot_favor_query_mass_fwd(const float* q, const void* state, const float* v, const float* proj,
                               const float* tw /* [T,Nq], device, or NULL */, int T, int H, int Nq, int Nc, int d, int m,
                               float* out, float* mass /* [T,H,Nc]; fold == 0: [T,H,ceil(Nq/16),Nc] */, int fold,
                               void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_long_mass_fwd(const float* q, const void* state, const float* v, const float* proj,
                                    const int32_t* lens /* [T], device, or NULL */, const float* tw /* [T,Nq], device, or NULL */,
                                    int T, int H, int Nq, int Nc, int d, int m, float* out,
                                    float* mass /* [T,H,Nc]; fold == 0: [T,H,ceil(Nq/16),Nc] */, int fold,
                                    void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_paged_mass_fwd(const float* q, const void* state, const float* v, const float* proj,
                                     const int32_t* lens /* [T], device, or NULL */, const float* tw /* [T,Nq], device, or NULL */,
                                     int T, int H, int Nq, int Nc, int d, int m, float* out,
                                     float* mass /* [T,H,Nc]; fold == 0: [T,H,ceil(Nq/16),Nc] */, int fold,
                                     void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_mass_fold(const float* part /* [TH,ntile,Nc] */, int TH, int ntile, int Nc, float* mass /* [TH,Nc] */, void* stream);

/* ---- top-k attention read-out: the k heaviest context slots per target row inside the query launch (csrc/favor_topk.h)
 * Per (task, head, target row n) the valid slots are ranked by the UN-NORMALISED score S[n,c] - the bits the read-out divides - in
 * descending order, ties to the lower slot index:
 *     idx[t,h,n,j] = the j-th slot of that ranking,     wk[t,h,n,j] = S[n,idx] / D[n],
 * the read-out's own single IEEE divide with the row's final D: the bits mlhot_favor_query_weights_fwd (or its long / paged sibling)
 * stores into w[t,h,n,idx].  D > 0 is one number per row and IEEE division is monotone, so the order of S is an order of w; where
 * two different S round to one w the VALUES agree with a top-k over w, the indices need not.  w[T,H,Nq,Nc] is never allocated or
 * written.  mlhot_favor_query_topk_fwd serves a mlhot_favor_keys_fwd / _ragged_fwd state (Nc <= 32), mlhot_favor_query_long_topk_fwd a
 * mlhot_favor_keys_long_fwd state (Nc <= 256), mlhot_favor_query_paged_topk_fwd a mlhot_favor_keys_paged_fwd state (Nc <= 4096).  The
 * arguments are the unmasked entry's (mlhot_favor_query_fwd / _long_fwd / _paged_fwd without w; ws is the 256-byte token block) plus
 *   k, 1 <= k <= 16; idx[T,H,Nq,k] int32 and wk[T,H,Nq,k] fp32, DEVICE memory, 4-byte aligned.
 * Valid slots: c < lens[t] (long, paged; lens NULL: all Nc).  The keys entry takes no lens, like the entry it extends: a column whose
 *   S is exactly +0 is a zero row of F_k and counts as absent.  Entries j >= the number of valid slots are idx = -1, wk = +0.0f.
 * out is BIT-EQUAL to the entry without top-k on the same arguments.  Rows n >= lens[t] of v are never read by the long and paged
 *   entries (the keys entry reads v as mlhot_favor_query_fwd does).  The bits of a row depend neither on the other rows of the call
 *   nor on the capacity Nc the same shots are kept in; a paged state of at most 256 slots gives the long entry's bits, a long state
 *   of at most 32 the keys entry's.
 * The paged entry walks the pages ONCE: the order of S needs no D, so each page joins the running k best (kept in registers) while
 *   its S lies in LDS, and k numbers per row are divided behind the last page.  (S descending, slot ascending) is a total order: the
 *   result does not depend on how the slots fall into pages.  No atomics, no workspace beyond the token block.
 * Envelope, alignment and error codes are those of the entry each one extends; idx == NULL, wk == NULL or k outside 1 .. 16 is
 * MLHOT_ERR_ARG; unsupported shapes write nothing.  Forward only; GPU build only.  Added within ABI 8: bindings look the symbols up. */
int mlhot_favor_query_topk_fwd(const float* q, const void* state, const float* v, const float* proj,
                               int T, int H, int Nq, int Nc, int d, int m, float* out,
                               int k, int32_t* idx /* [T,H,Nq,k] */, float* wk /* [T,H,Nq,k] */,
                               void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_long_topk_fwd(const float* q, const void* state, const float* v, const float* proj,
                                    const int32_t* lens /* [T], device, or NULL */, int T, int H, int Nq, int Nc, int d, int m,
                                    float* out, int k, int32_t* idx /* [T,H,Nq,k] */, float* wk /* [T,H,Nq,k] */,
                                    void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_paged_topk_fwd(const float* q, const void* state, const float* v, const float* proj,
                                     const int32_t* lens /* [T], device, or NULL */, int T, int H, int Nq, int Nc, int d, int m,
                                     float* out, int k, int32_t* idx /* [T,H,Nq,k] */, float* wk /* [T,H,Nq,k] */,
                                     void* ws, size_t ws_bytes, void* stream);

/* ---- shared targets: one set of query rows against every stored context (csrc/favor_shared.h) --------------------
 * q[Nq,H,d] carries NO task axis: the same Nq rows are asked of all T tasks of the state.  mlhot_favor_query_shared_fwd serves a
 * mlhot_favor_keys_fwd / _ragged_fwd state (Nc <= 32; no lens, like the entry it extends: a masked slot is a zero row of F_k and v is
 * read there as mlhot_favor_query_fwd reads it - zero-fill it), mlhot_favor_query_long_shared_fwd a mlhot_favor_keys_long_fwd state
 * (Nc <= 256, the SAME lens or NULL; rows n >= lens[t] of v are never read).  v[T,Nc,H,d], proj[m,d] as in the per-task entries.
 * -> out[T,Nq,d*H] in mlhot_favor_fwd's merged order and, with w != NULL, w[T,H,Nq,Nc] = S / D as mlhot_favor_query_weights_fwd
 *   defines it, columns n' >= lens[t] exactly 0.0f.  w == NULL means no read-out (unlike _weights_fwd: one entry serves both), and out
 *   is BIT-EQUAL with and without it.  ONE launch for any Nq and T.
 * A workgroup owns one (head, 16-row target tile) and a contiguous group of tasks: it forms the query features F_q ONCE - they read
 *   the query row, proj and the row's own maximum, nothing of a task - keeps them in LDS and runs the per-task entry's own steps
 *   against each task's F_k, lens[t] and v.  out and w are BIT-EQUAL to mlhot_favor_query_fwd / _weights_fwd / _long_fwd on q
 *   replicated to [T,Nq,H,d], and carry their ROW-INVARIANCE guarantee.  No atomics; every store is a vector store.
 * task_group: tasks per workgroup, held to 1 .. T; 0: the library picks it so that the grid ceil(T / task_group) H ceil(Nq / 16)
 *   covers the 256 CUs about once.  A task's sums never see another task's: the bits of out and w do not depend on task_group.
 * ws: mlhot_favor_query_shared_ws_bytes / _long_shared_ws_bytes (256, the token block: the kernels work in LDS alone - the per-task
 *   kernels' 124 KB / 140 KB); 0 for a shape the entry does not serve.
 * Envelope, alignment rules and error codes are those of the per-task entry each one extends (task_group < 0 is MLHOT_ERR_ARG); an
 * unsupported shape returns MLHOT_ERR_UNSUPPORTED and writes nothing.  Forward only; GPU build only.  Added within ABI 8: bindings look the symbols up. */
size_t mlhot_favor_query_shared_ws_bytes(int T, int H, int Nq, int Nc, int d, int m);
size_t mlhot_favor_query_long_shared_ws_bytes(int T, int H, int Nq, int Nc, int d, int m);
int mlhot_favor_query_shared_fwd(const float* q /* [Nq,H,d] */, const void* state, const float* v, const float* proj,
                                 int T, int H, int Nq, int Nc, int d, int m, int task_group /* 0: the library's choice */,
                                 float* out /* [T,Nq,d*H] */, float* w /* [T,H,Nq,Nc], or NULL */,
                                 void* ws, size_t ws_bytes, void* stream);
int mlhot_favor_query_long_shared_fwd(const float* q /* [Nq,H,d] */, const void* state, const float* v, const float* proj,
                                      const int32_t* lens /* [T], device, or NULL */,
                                      int T, int H, int Nq, int Nc, int d, int m, int task_group /* 0: the library's choice */,
                                      float* out /* [T,Nq,d*H] */, float* w /* [T,H,Nq,Nc], or NULL */,
                                      void* ws, size_t ws_bytes, void* stream);

/* ---- cached contexts that let shots go: the per-shot rows moved by a plan (csrc/rows_compact.h) ------------------
 * mlhot_rows_compact: `sets` row sets, 1 <= sets <= 4, that share one plan.  Row set i is (src[i], dst[i], W[i]): fp32 rows of W[i]
 *   floats in [T][cap][W[i]]; src, dst and W are arrays of `sets` entries in HOST memory.  plan[T][cap] (int32, DEVICE memory, read by
 *   the kernel alone - no host synchronisation):  dst_i[t][s][:] = src_i[t][plan[t][s]][:],  and a row of exact zeros - src is not
 *   read - where plan[t][s] is -1.  A plan value outside -1 .. cap - 1 is held to -1, so no plan content reads or writes out of
 *   bounds.  Rows are selected by index, never by a product with a mask: a NaN or Inf in a row that no plan entry names does not reach
 *   dst.  EVERY row of every dst is written, whatever it held.  ONE launch (label rows.compact), float4 loads and stores, no atomics.
 *   Served: W[i] % 4 == 0, 16-byte aligned src and dst, 1 <= cap <= 4096 (and fewer than 2^31 float4 per task over all sets);
 *   otherwise MLHOT_ERR_UNSUPPORTED.  A dst that overlaps any src, or another dst: MLHOT_ERR_ARG.  Whatever is refused writes nothing.
 *   GPU build only (the host build returns MLHOT_ERR_UNSUPPORTED).  Added within ABI 8: bindings look the symbol up. */
int mlhot_rows_compact(const float* const* src /* host array of `sets` device pointers */,
                       float* const* dst /* host array of `sets` device pointers */, const int* W /* host array */, int sets,
                       const int32_t* plan /* [T][cap], DEVICE memory */, int T, int cap, void* stream);

/* ---- cached contexts joined or regrouped across states: per-shot rows gathered from several sources (csrc/rows_gather.h)
 * mlhot_rows_gather: `sets` row sets, 1 <= sets <= 2, filled from `nsrc` sources, 1 <= nsrc <= 8, by one plan.  Row set i holds fp32
 *   rows of W[i] floats.  Source j is a flat list of rows[j] rows per set (a state's [T_j][cap_j] slots; the sources may differ in
 *   both): src[i * nsrc + j] is set i of source j.  dst[i] is [T][cap][W[i]].  src, rows, dst and W are arrays in HOST memory.
 *   plan[T][cap][2] (int32, DEVICE memory, read by the kernel alone - no host synchronisation) = (source, flat row in it):
 *       dst_i[t][s][:] = src_{ps,i}[pr][:]  with (ps, pr) = plan[t][s],
 *   and a row of exact zeros - no source is read - where ps is outside 0 .. nsrc - 1 or pr outside 0 .. rows[ps] - 1; (-1, -1) is
 *   the fill.  No plan content reads or writes out of bounds.  Rows are selected by index, never by a product with a mask: a NaN
 *   or Inf in a row that no plan entry names does not reach dst.  One source row may be named by several destination rows.  EVERY
 *   row of every dst is written, whatever it held.  ONE launch (label rows.gather), float4 loads and stores, no atomics.
 *   Served: W[i] % 4 == 0, 16-byte aligned src and dst, 8-byte aligned plan, sets, nsrc as above, 1 <= cap <= 4096, fewer than
 *   2^31 float4 per task over all sets and rows[j] < 2^31; otherwise MLHOT_ERR_UNSUPPORTED.  A NULL pointer, rows[j] < 1, or a dst
 *   that overlaps any src or another dst: MLHOT_ERR_ARG.  Whatever is refused writes nothing.  GPU build only (the host build
 *   returns MLHOT_ERR_UNSUPPORTED).  Added within ABI 8: bindings look the symbol up. */
int mlhot_rows_gather(const float* const* src /* host array of sets * nsrc device pointers */,
                      const int64_t* rows /* host array of nsrc row counts */, int nsrc,
                      float* const* dst /* host array of `sets` device pointers */, const int* W /* host array */, int sets,
                      const int32_t* plan /* [T][cap][2], DEVICE memory */, int T, int cap, void* stream);

/* ---- strict sharded parity of the key stabiliser -------------------------
 * fast_attention.py:96-97 takes torch.max over the keys of the WHOLE batch.  When a caller shards the meta-batch over
 * ranks, each rank's launch sequence can be run in two halves around the caller's own collectives on `xchg`
 * (device memory, 4 floats, caller-owned):
 *   forward  stage 0: everything up to the rank-local key maximum           -> xchg[0] = that maximum
 *            (caller: xchg[0] = MAX over ranks; xchg[1] = 1 on the lowest rank whose maximum equals it, else 0)
 *            stage 1: the rest of the forward, with xchg[0] as the stabiliser
 *   backward stage 0: everything up to the rank-local sum of dL/d(stabiliser) -> xchg[2] = that sum
 *            (caller: xchg[2] = SUM over ranks)
 *            stage 1: the rest; the rank with xchg[1] = 1 routes the batch-wide sum to its arg-max key, the others to none
 * The same saved / scratch / ws buffers must be passed to both stages; a world of one (xchg[1] = 1, xchg untouched) reproduces
 * the unstaged call.  No communication library is linked: the collective is the caller's (mlhot/dist.py: StabiliserExchange).  */
int mlhot_favor_fwd_staged(const float* q, const float* k, const float* v, const float* proj,
                           int T, int H, int Nq, int Nc, int d, int m, float* out,
                           void* ws, size_t ws_bytes, int stage, float* xchg, void* stream);
int mlhot_favor_bwd_staged(const float* q, const float* k, const float* v, const float* proj,
                           int T, int H, int Nq, int Nc, int d, int m, const float* out, const float* dout,
                           float* dq, float* dk, float* dv, void* ws, size_t ws_bytes, int stage, float* xchg, void* stream);

/* ---- L1: losses --------------------------------------------------------------------------
 * LossFunc.calc_loss (trainer/losses.py:32-80).  mu[rows,y_dim], gt[rows,gt_dim];
 * loss / dloss are device scalars.                                                            */
int mlhot_loss_fwd(int kind, const float* mu, const float* gt, int rows, int y_dim, int gt_dim, float* loss, void* stream);
int mlhot_loss_bwd(int kind, const float* mu, const float* gt, int rows, int y_dim, int gt_dim,
                   const float* dloss, float* dmu, void* stream);
/* ABI 7: the trainer's objective `losses = loss + kl * beta` (trainer/model_trainer.py:77-78) inside the loss's own launches - in a
 * replayed step every dependent launch costs ~4.7 us whatever it computes, and this pair of scalars was four of them.
 *   fwd: loss[0] (may be NULL) as mlhot_loss_fwd; total[0] = loss + alpha * x[0], product and sum rounded separately (mlhot_axpy's bits)
 *   bwd: dmu as mlhot_loss_bwd(dloss = dtotal); dx[0] (may be NULL) = alpha * dtotal[0]
 * x, total, dtotal, dx: device scalars.                                                                                               */
int mlhot_loss_plus_fwd(int kind, const float* mu, const float* gt, int rows, int y_dim, int gt_dim, const float* x, float alpha,
                        float* loss, float* total, void* stream);
int mlhot_loss_plus_bwd(int kind, const float* mu, const float* gt, int rows, int y_dim, int gt_dim, const float* dtotal, float alpha,
                        float* dmu, float* dx, void* stream);

/* ---- E2 / D2: ResNet encoder building blocks --------------------------------------------------
 * nn.Conv2d (cross-correlation, zero padding, NCHW, weight [Cout,Cin,k,k], optional fused ReLU) for
 * the 5x5 s2 p2 stem, the 3x3 s2 / s1 p1 block convs and the 1x1 s2 (3x3 in the BBB twin) skip of
 * ImageEncoder / NPDecoder (networks/models.py:63-192, networks/ResNet.py:25-74).  Backward: `y` is
 * the forward output (used for the ReLU mask when relu=1); dx / dw / db may be NULL.  A shape with
 * a non-positive extent or a kernel larger than the padded image (H + 2 pad < k or W + 2 pad < k) is
 * MLHOT_ERR_ARG in fwd and bwd before anything is launched, and 0 scratch bytes.  db is computed as
 * a column of the dw problem: db without dw is MLHOT_ERR_ARG; dw NULL needs no scratch.             */
size_t mlhot_conv2d_bwd_scratch_bytes(int N, int Cin, int H, int W, int Cout, int k, int stride, int pad);
int mlhot_conv2d_fwd(const float* x, const float* w, const float* b, float* y, int N, int Cin, int H, int W, int Cout, int k,
                     int stride, int pad, int relu, void* stream);
int mlhot_conv2d_bwd(const float* x, const float* w, const float* y, const float* dy, int N, int Cin, int H, int W, int Cout, int k,
                     int stride, int pad, int relu, float* dx, float* dw, float* db, void* scratch, size_t scratch_bytes, void* stream);
/* residual join y = relu(a + b) (ResNet.py:69-72); backward g = dy * (y > 0) is the gradient of both inputs */
/* y[i] = a[i] + alpha * x[i] (a NULL: alpha * x[i]); product and sum rounded separately.  The trainer's `loss + kl * beta`
 * (trainer/model_trainer.py:77-78) as one launch per direction instead of two elementwise torch operators.                   */
int mlhot_axpy(const float* a, const float* x, float alpha, float* y, size_t n, void* stream);
int mlhot_add_relu_fwd(const float* a, const float* b, float* y, size_t n, void* stream);
int mlhot_add_relu_bwd(const float* y, const float* dy, float* g, size_t n, void* stream);
/* 2x2 max-pool over `planes` maps of H x W (nn.AdaptiveMaxPool2d((2,2)) on 4x4 maps, models.py:107-110) */
int mlhot_pool2_fwd(const float* x, float* y, uint8_t* amax, int planes, int H, int W, void* stream);
int mlhot_pool2_bwd(const float* dy, const uint8_t* amax, float* dx, int planes, int H, int W, void* stream);

/* ---- E2 / D2 / B1: whole ResNet trunks in one call -------------------------------------------------------------------
 * The 5x5 s2 stem (+ReLU) and the four BN-free BasicBlocks {conv3x3 s2 + ReLU; conv3x3 s1; skip conv (1x1 s2 in ImageEncoder /
 * NPDecoder, networks/ResNet.py:32-34,58-74; 3x3 s2 p1 in the Bayes-by-backprop twin, networks/ANPMRShapeNet3D.py:48-51,85);
 * add; ReLU} of networks/models.py:63-117,156-182 - for EVERY pass of a model step at once (context images, target images,
 * decoder images; each pass names its weight set, passes may share one).  Weight-stationary fp32-MFMA kernels (csrc/resnet_ws.h);
 * supported inputs: 3 x 64 x 64 (ShapeNet3D) and 1 x 128 x 128 (Distractor), MLHOT_ERR_UNSUPPORTED otherwise (callers then
 * compose mlhot_conv2d_* instead).
 *   w / b [13]: stem, then (conv1, conv2, skip) of blocks 1..4, in the reference's own layouts [Cout][Cin][k][k] / [Cout];
 *   act [9]   : saved activations, written by the forward, read by the backward: a0 = stem output, then (mid_i, y_i) of the
 *               blocks (post-ReLU); act[8] is the trunk's output map [n][64][H/32][H/32];
 *   dfeat     : backward: gradient wrt act[8];  dw / db: gradients (overwritten; summed over the passes that share the set).  */
#define MLHOT_TRUNK_MAX_PASS 6
#define MLHOT_TRUNK_MAX_WSET 4
typedef struct mlhot_trunk_wset { const float* w[13]; const float* b[13]; float* dw[13]; float* db[13]; int skip_k; } mlhot_trunk_wset;
typedef struct mlhot_trunk_pass { const float* img; int n_img; int wset; float* act[9]; const float* dfeat; } mlhot_trunk_pass;
size_t mlhot_trunk_act_floats(int C, int H, int n_img, int k);
size_t mlhot_trunk_scratch_bytes(const mlhot_trunk_pass* passes, int n_pass, const mlhot_trunk_wset* wsets, int n_wset, int C, int H, int backward);
int mlhot_trunk_fwd(const mlhot_trunk_pass* passes, int n_pass, const mlhot_trunk_wset* wsets, int n_wset, int C, int H,
                    void* scratch, size_t scratch_bytes, void* stream);
int mlhot_trunk_bwd(const mlhot_trunk_pass* passes, int n_pass, const mlhot_trunk_wset* wsets, int n_wset, int C, int H,
                    void* scratch, size_t scratch_bytes, void* stream);

/* ---- B1: Bayes-by-backprop weight sample + KL (bbb/BBBConv.py:86-108, bbb/BBBLinear.py:79-101) ----
 * w = mu + eps * log1p(exp(rho)); kl = sum 0.5*(2 log(sigma/0.1) - 1 + (0.1/sigma)^2 + (mu/sigma)^2).
 * eps is drawn by the caller on the torch CPU generator (parity with BBBConv.py:88). klterm: n floats. */
int mlhot_bbb_sample_fwd(const float* mu, const float* rho, const float* eps, float* w, float* klterm, float* kl, size_t n, void* stream);
int mlhot_bbb_sample_bwd(const float* mu, const float* rho, const float* eps, const float* dw, const float* dkl, float* dmu, float* drho,
                         size_t n, void* stream);

/* The same for up to MLHOT_BBB_MAX_ITEMS tensors in one launch pair (a Bayes-by-backprop encoder samples every layer's weight
 * and bias once per forward: 26 tensors for ANPMRShapeNet3D.py:40-90): w_i = mu_i + eps_i * softplus(rho_i) for every item,
 * kl = the sum of ALL items' KL terms.  `partial`: mlhot_bbb_sample_multi_scratch_floats() floats of scratch.  Backward: items
 * carry dw (may be NULL: no gradient reached that sample), dmu, drho (overwritten); dkl as above.
 * An item may carry a SECOND independent sample of the same posterior (eps2 -> w2; backward dw2): the model encodes the context
 * and the target images with two samples per step (ANPMRShapeNet3D.py:198-199); both come out of one launch, the KL (which does
 * not depend on eps) is computed once, and the backward adds both samples' contributions into dmu / drho in one pass. */
#define MLHOT_BBB_MAX_ITEMS 32
typedef struct {
  const float* mu; const float* rho; const float* eps;
  float* w;                       /* forward output */
  const float* dw; float* dmu; float* drho;   /* backward */
  size_t n;
  const float* eps2; float* w2; const float* dw2;   /* optional second sample (all NULL when unused) */
} mlhot_bbb_item;
size_t mlhot_bbb_sample_multi_scratch_floats(const mlhot_bbb_item* items, int n_items);
int mlhot_bbb_sample_multi_fwd(const mlhot_bbb_item* items, int n_items, float* partial, float* kl, void* stream);
int mlhot_bbb_sample_multi_bwd(const mlhot_bbb_item* items, int n_items, const float* dkl, void* stream);

/* ---- batch ingest: the host-side image conversion of the data loaders, on the device ----
 * dst[n][c][y][x] = (float)src[n][y][x][c] / div, i.e. dataset/shapenet_1d.py:189-190 (`xs.astype(np.float32) / 255.0`;
 * same in dataset/pascal_1d.py, shapenet_3d.py, distractor.py) followed by utils/utils.py:26-30
 * (convert_channel_last_np_to_tensor: permute(0,1,4,2,3).contiguous()).  Bit-identical to that host arithmetic (IEEE
 * fp32 divide).  src: n_img*H*W*C bytes packed channel-last (4-byte aligned for the fast path), dst: n_img*C*H*W floats. */
int mlhot_ingest_u8_nhwc(const uint8_t* src, float* dst, long n_img, int H, int W, int C, float div, void* stream);

/* ---- device data augmentation fused into the batch ingest (DESIGN.md "Device augmentation") ----
 * The reference's "data_aug" (config aug_list) runs an imgaug Sequential per image on the host inside get_batch
 * (dataset/shapenet_1d.py:174-176, dataset/pascal_1d.py:116-118).  Here it runs on the staged bytes, one workgroup per image, with
 * the divide of mlhot_ingest_u8_nhwc behind it.  Scope: C = 1, 1 <= H, W <= 128, the two single-channel sequences
 *   shapenet_1d (dataset/shapenet_1d.py:34-72): CropAndPad, Affine, OneOf(Dropout, CoarseDropout)
 *   pascal_1d   (utils/augment.py:83-122):      CropAndPad, GammaContrast, AverageBlur, Affine, OneOf(Dropout, CoarseDropout)
 * Every step sits in Sometimes(0.5) and the Sequential has random_order=True; the host (mlhot/augment.py) draws all of it and
 * hands the kernel one record per image.  The ops, restated from imgaug 0.4 / cv2 (bit-exact to this spec, not to imgaug):
 *   CROP_PAD  CropAndPad(percent=(0, 0.05), pad_mode=ALL, pad_cval=(0, 255)), keep_size (shapenet_1d.py:50, augment.py:96):
 *             pad[] = round(U(0, 0.05) * H or W) per side; np.pad on uint8 in `pad_mode` (MLHOT_PAD_*; constant_values and
 *             linear_ramp's end_values = pad_cval); then cv2.resize INTER_CUBIC back to H x W: A = -0.75, half-pixel centres,
 *             src = (float)((d + 0.5) * n_src / n_dst - 0.5), coefficients in fp32 rounded (half even) to 1/2048, replicated
 *             border, sum rounded at 2^22 and saturated.  No pad on any side: no resize.
 *   GAMMA     GammaContrast((0.5, 2.0)) (augment.py:98): luts[lut] = round(255 * (v / 255) ** g), built on the host in float64.
 *   BLUR      AverageBlur(k=(1, 3)) (augment.py:102): k in {1, 2, 3}; k x k box mean, anchor k / 2 (k = 2: [x-1, x]),
 *             BORDER_REFLECT_101, rounded half to even.
 *   AFFINE    Affine(scale (0.8, 1.2) per axis, translate_percent (-0.1, 0.1) per axis, order [0, 1], cval (0, 255),
 *             mode ALL) (shapenet_1d.py:52-58, augment.py:104-110) about the centre (W/2 - 0.5, H/2 - 0.5).  The inverse map in
 *             1/65536 px: src_x = (aff_ax * x + aff_bx) / 2^16, src_y likewise.  order 0: nearest, (X + 2^15) >> 16; order 1:
 *             cv2's fixed-point bilinear, coordinates (X + 2^10) >> 11 in 1/32 px, weights (32 - f) * (32 - g) * 32 etc. in
 *             1/32768, sum rounded at 2^15.  aff_mode = MLHOT_BORDER_*: constant (aff_cval), edge = REPLICATE,
 *             symmetric = REFLECT, reflect = REFLECT_101, wrap = WRAP.
 *   DROPOUT   Dropout(p=(0.01, 0.1)) (shapenet_1d.py:62, augment.py:114): pixel i -> 0 when hash(i) < drop_thresh (= p * 2^32).
 *   COARSE_DROPOUT  CoarseDropout(p=(0, 0.05), size_percent=(0.02, 0.25)) (shapenet_1d.py:63-66, augment.py:115-118): a
 *             coarse_h x coarse_w mask (max(3, round(sp * H or W))), cell c dropped when hash(2^30 + c) < coarse_thresh, upscaled by
 *             nearest neighbour (cell row = y * coarse_h / H).  per_channel has no effect at C = 1.
 *   hash(item) = fmix32(key ^ item * 0x9E3779B1), key = fmix32 chained over (seed + 0x9E3779B9, counter, side, image)
 *   (fmix32 = murmur3's 32-bit finaliser; all arithmetic mod 2^32).
 * Record: op[0 .. n_steps) = the steps in this image's application order (OneOf already resolved to DROPOUT or COARSE_DROPOUT);
 * a step runs when bit (1 << op) of `on` is set.  Out-of-range fields are clamped (never read or written out of bounds).
 * Added within ABI 7 (a pure addition): the binding looks for the symbol and checks mlhot_augment_record_bytes() before its first
 * call.                                                                                                                     */
enum { MLHOT_AUG_CROP_PAD = 0, MLHOT_AUG_GAMMA = 1, MLHOT_AUG_BLUR = 2, MLHOT_AUG_AFFINE = 3, MLHOT_AUG_DROPOUT = 4,
       MLHOT_AUG_COARSE_DROPOUT = 5 };
/* numpy's ten pad modes (imgaug's pad_mode=ALL) */
enum { MLHOT_PAD_CONSTANT = 0, MLHOT_PAD_EDGE = 1, MLHOT_PAD_LINEAR_RAMP = 2, MLHOT_PAD_MAXIMUM = 3, MLHOT_PAD_MEAN = 4,
       MLHOT_PAD_MEDIAN = 5, MLHOT_PAD_MINIMUM = 6, MLHOT_PAD_REFLECT = 7, MLHOT_PAD_SYMMETRIC = 8, MLHOT_PAD_WRAP = 9 };
/* imgaug Affine's modes = cv2 borders CONSTANT, REPLICATE, REFLECT, REFLECT_101, WRAP */
enum { MLHOT_BORDER_CONSTANT = 0, MLHOT_BORDER_EDGE = 1, MLHOT_BORDER_SYMMETRIC = 2, MLHOT_BORDER_REFLECT = 3, MLHOT_BORDER_WRAP = 4 };
typedef struct {
  int32_t n_steps, op[7], on;
  int32_t pad[4];                 /* top, right, bottom, left (px) */
  int32_t pad_mode, pad_cval;
  int32_t lut;                    /* row of `luts` (GAMMA) */
  int32_t blur_k;
  int32_t aff_order, aff_mode, aff_cval, aff_ax, aff_bx, aff_ay, aff_by;
  uint32_t drop_thresh, coarse_thresh;
  int32_t coarse_h, coarse_w;
  uint32_t seed, counter, side, image;    /* hash inputs: stream seed, batch counter, 0 context / 1 target, image of the side */
} mlhot_aug_record;               /* 128 bytes */
size_t mlhot_augment_record_bytes(void);   /* sizeof(mlhot_aug_record): binding self-check */
/* src: n_img * H * W bytes (C = 1); dst: n_img * H * W floats = augmented byte / div; rec: n_img records; luts: n_luts x 256
 * bytes (may be NULL when n_luts = 0).  All device pointers; rec and luts are read on the device only. */
int mlhot_augment_ingest_u8(const uint8_t* src, float* dst, long n_img, int H, int W, int C, float div,
                            const mlhot_aug_record* rec, const uint8_t* luts, int n_luts, void* stream);

/* ---- device data augmentation of the IMAGE tasks (csrc/augment_img.h) ----
 * The base Augmenter (utils/augment.py:22-63: shapenet_3d) and AugmenterDistractor (dataset/shapenet_distractor.py:54-81), one
 * workgroup per image over planar LDS.  Scope: C in {1, 3}; H, W <= 64 for C = 3, <= 128 for C = 1; anything else is
 * MLHOT_ERR_UNSUPPORTED.  src: channel-last bytes [n_img, H, W, C]; dst: fp32 [n_img, C, H, W].
 *   pre_op  what the loader's `(images * 255).astype(uint8)` does to a byte b before the ops: 0 = b (shapenet_3d: float32(k) / 255
 *           * 255 truncates back to k for every byte), 1 = (256 - b) mod 256 (distractor: uint8 * 255 wraps; a reproduced quirk).
 *   output  (float)byte / div, then / div2: two IEEE fp32 divisions in that order.  shapenet_3d: div = 255, div2 = 1; distractor:
 *           div = div2 = 255 (generate() divides, then shapenet_distractor.py:256 divides again; a reproduced quirk).
 * CROP_PAD, GAMMA, BLUR, AFFINE: the op of mlhot_aug_record on every channel with the image's ONE parameter set - np.pad with
 *   ((t, b), (l, r), (0, 0)): statistic modes per channel and line; linear_ramp's zero-step rule over all channels of a side.
 * DROPOUT / COARSE_DROPOUT: drop_per_channel / coarse_per_channel = 0: one mask for all channels (items as in mlhot_aug_record);
 *   != 0: item = c * H * W + pixel, or 2^30 + c * cells + cell.  C = 1: no effect.
 * BRIGHTNESS  AddToBrightness((-30, 30)): bright_add in -30 .. 30, bright_space = MLHOT_CS_*.  C = 1: sat_u8(v + add).  C = 3: RGB ->
 *   8-bit values of the space -> brightness channel b = sat_u8(b + add) -> RGB.  sat = clamp to 0 .. 255; `>>` floors.
 *   YCRCB  Y = (4899 R + 9617 G + 1868 B + 2^13) >> 14; Cr = sat(((R - Y) * 11682 + 128 * 2^14 + 2^13) >> 14); Cb likewise with
 *          (B - Y) * 9241.  Back: R = sat(Y + ((Cr - 128) * 22987 + 2^13 >> 14)), G = sat(Y + ((Cr - 128) * -11698 + (Cb - 128) * -5636
 *          + 2^13 >> 14)), B = sat(Y + ((Cb - 128) * 29049 + 2^13 >> 14)).  Coefficients = round(c * 2^14) of 0.299 0.587 0.114 0.713
 *          0.564 | 1.403 0.714 0.344 1.773.
 *   YUV    the same Y; U = (B - Y) * 8061, V = (R - Y) * 14369; back R: (V - 128) * 18678, G: (U - 128) * -6472 + (V - 128) * -9519,
 *          B: (U - 128) * 33292.  Real coefficients 0.492 0.877 | 1.140 0.395 0.581 2.032.
 *   HSV    V = max, d = max - min; S = V ? (510 d + V) / (2 V) : 0; H (degrees / 2, 0 .. 179): d = 0: 0; else n = 30 (G - B) if
 *          V = R, else 30 (B - R) + 60 d if V = G, else 30 (R - G) + 120 d; n < 0: n += 180 d; H = (2 n + d) / (2 d), 180 -> 0.
 *          Back: i = H / 30, f = H - 30 i; p = (2 V (255 - S) + 255) / 510, q = (2 V (7650 - S f) + 7650) / 15300,
 *          t = (2 V (7650 - S (30 - f)) + 7650) / 15300; (R, G, B) = (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q) for i = 0 .. 5.
 *   HLS    L = (max + min + 1) >> 1; S = 0 if d = 0, else with m = max + min (m <= 255) or 510 - max - min: (510 d + m) / (2 m),
 *          saturated; H as HSV.  Back (units of 1 / 65025): P2 = L (255 + S) if L <= 127 else 255 L + 255 S - L S; P1 = 510 L - P2;
 *          channel at hue h (R: H + 60, G: H, B: H - 60, mod 180): N = 30 P1 + (P2 - P1) h if h < 30, 30 P2 if h < 90,
 *          30 P1 + (P2 - P1)(120 - h) if h < 120, else 30 P1; value = sat((2 N + 7650) / 15300).
 *   LAB, LUV  through the tables of mlhot_colour_tabs - built once on the host in float64 by mlhot.augment.colour_tables - linear light on the
 *          integer grid 0 .. Q = 4080:
 *            lin[256]   round(Q * (v / 255 <= 0.04045 ? (v / 255) / 12.92 : ((v / 255 + 0.055) / 1.055) ^ 2.4))
 *            m[9]       sRGB -> XYZ (D65: 0.412453 0.357580 0.180423 / 0.212671 0.715160 0.072169 / 0.019334 0.119193 0.950227), each
 *                       row divided by its sum (its white), times 2^12, rounded; the row's largest entry then takes the remainder
 *                       so that the row sums to exactly 2^12 (grey stays grey); minv[9]: the inverse of the row-normalised real
 *                       matrix, treated the same way
 *            f[Q + 1]   round(2^15 * (t / Q > 216 / 24389 ? cbrt(t / Q) : (24389 / 27 * t / Q + 16) / 116))
 *            s8[Q + 1]  round(255 * (u <= 0.0031308 ? 12.92 u : 1.055 u ^ (1 / 2.4) - 0.055)), u = t / Q
 *            xn, zn     round(2^12 * 0.950456), round(2^12 * 1.088754); w = xn + 15 * 2^12 + 3 zn; un = (2 * 4 xn 2^16 + w) / (2 w),
 *                       vn = (2 * 9 * 2^12 * 2^16 + w) / (2 w); wz = 12 * 2^16 - 3 un - 20 vn
 *          x, y, z = (m row . lin[R G B] + 2^11) >> 12; F. = f[.]; Ln = 116 Fy - 16 * 2^15;
 *          L8 = sat((2 * 255 Ln + 100 * 2^15) / (200 * 2^15)).
 *          LAB: a8 = sat(128 + ((500 (Fx - Fy) + 2^14) >> 15)), b8 = sat(128 + ((200 (Fy - Fz) + 2^14) >> 15)).
 *          LUV (neutral codes 97 and 136 are integers so that grey stays grey - own choice): d = xn x + 15 * 2^12 y + 3 zn z;
 *            d = 0: u' = un, v' = vn; else u' = (2 * 4 xn x 2^16 + d) / (2 d), v' = (2 * 9 * 2^12 y 2^16 + d) / (2 d);
 *            u8 = sat(97 + rdiv(255 * 13 Ln (u' - un), 354 * 2^31)), v8 = sat(136 + rdiv(255 * 13 Ln (v' - vn), 262 * 2^31)),
 *            rdiv(a, b) = floor((2 a + b) / (2 b)).
 *          Back, exact integer cubes: D = 1479000, Ny = 5000 L8 + 204000 (f = N / D);
 *            lin(N) = 29 N > 6 D ? (N^3 + K / 2) / K, K = D^3 / Q : max(0, rdiv(Q * 108 (29 N - 4 D), 24389 D)), clamped to 0 .. 2 Q.
 *          LAB: x = lin(Ny + 2958 (a8 - 128)), y = lin(Ny), z = lin(Ny - 7395 (b8 - 128)).
 *          LUV: y = lin(Ny); L8 = 0: x = z = 0; else u' = un + rdiv(354 * 2^16 (u8 - 97), 1300 L8), v' = max(1, vn +
 *            rdiv(262 * 2^16 (v8 - 136), 1300 L8)); x = rdiv(y max(0, u') vn, v' un), z = rdiv(y max(0, 12 * 2^16 - 3 u' - 20 v') vn,
 *            v' wz), both clamped to 0 .. 2 Q.
 *          R, G, B = s8[clamp((minv row . (x y z) + 2^11) >> 12, 0, Q)].                                                        */
enum { MLHOT_AUG_BRIGHTNESS = 6 };
enum { MLHOT_CS_YCRCB = 0, MLHOT_CS_HSV = 1, MLHOT_CS_HLS = 2, MLHOT_CS_LAB = 3, MLHOT_CS_LUV = 4, MLHOT_CS_YUV = 5 };
#define MLHOT_CS_Q 4080
typedef struct {
  mlhot_aug_record base;          /* op[] may hold MLHOT_AUG_BRIGHTNESS; `on` bit 6 */
  int32_t bright_add, bright_space;
  int32_t drop_per_channel, coarse_per_channel;
  int32_t reserved[4];
} mlhot_aug_record_img;           /* 160 bytes */
typedef struct {
  int32_t m[9], minv[9];
  int32_t xn, zn, un, vn, wz, reserved;
  uint16_t lin[256];
  uint16_t f[4096];               /* entries above Q repeat f[Q] */
  uint8_t s8[4096];               /* likewise */
} mlhot_colour_tabs;              /* 12896 bytes */
size_t mlhot_augment_img_record_bytes(void);     /* sizeof(mlhot_aug_record_img): binding self-check */
size_t mlhot_colour_tabs_bytes(void);
/* rec: n_img records; luts as in mlhot_augment_ingest_u8; colour_tabs: one mlhot_colour_tabs struct, or NULL (when no record asks for
 * LAB / LUV - such a step is then skipped).  All device pointers. */
int mlhot_augment_ingest_u8_img(const uint8_t* src, float* dst, long n_img, int H, int W, int C, int pre_op, float div, float div2,
                                const mlhot_aug_record_img* rec, const uint8_t* luts, int n_luts, const void* colour_tabs,
                                void* stream);

/* ---- resident image pool: a batch described by image ids, gathered and composed on the device (csrc/pool_ingest.h) ----
 * pool: uint8 [n_pool, H, W, 4], channel-last RGBA; bank: uint8 [n_bank, H, W, 3] backgrounds (NULL when n_bank is 0).  Per output
 * image i: ids[i] in [0, n_pool) and bg[i] = -1 (no composition) or in [0, n_bank).  Per pixel p and channel c < 3
 *     byte = (bg[i] >= 0 && pool[ids[i]][p][3] == 255) ? bank[bg[i]][p][c] : pool[ids[i]][p][c]
 * (dataset/shapenet_3d.py:235-239: rgb * mask + bg * (1 - mask) with mask = alpha < 1.0 on k / 255 floats - a 0/1 mask makes that a
 * select), dst: fp32 [n_img, 3, H, W] = (float)byte / div, the divide of mlhot_ingest_u8_nhwc.  Any H, W.  The entries check n_bank
 * against NULL and nothing else about the indices: the caller range-checks ids and bg on the host before it ships them
 * (mlhot.ingest.BatchIngest.stage_ids).  Added within ABI 7 (a pure addition).  All device pointers. */
int mlhot_pool_ingest_u8(const uint8_t* pool, long n_pool, const int* ids, const uint8_t* bank, long n_bank, const int* bg, float* dst,
                         long n_img, int H, int W, float div, void* stream);
/* The composed bytes as the input of mlhot_augment_ingest_u8_img's op sequence with C = 3, pre_op = 0, div2 = 1: same records, LUTs and
 * colour tables.  H, W <= 64, MLHOT_ERR_UNSUPPORTED otherwise. */
int mlhot_pool_augment_ingest_u8_img(const uint8_t* pool, long n_pool, const int* ids, const uint8_t* bank, long n_bank, const int* bg,
                                     float* dst, long n_img, int H, int W, float div, const mlhot_aug_record_img* rec,
                                     const uint8_t* luts, int n_luts, const void* colour_tabs, void* stream);

/* ---- resident grey pool: the single-channel tasks (shapenet_1d, pascal_1d, distractor) by image ids ----
 * pool: uint8 [n_pool, H, W, 1] - the bytes the loader's byte batch carries (Distractor: 255 - images, inverted once by the loader);
 * ids[i] in [0, n_pool).  Each entry gives, bit for bit, what its byte twin gives on the gathered images pool[ids] with the same
 * remaining arguments: no alpha, no bank, no new semantics.  dst: fp32 [n_img, 1, H, W].  As above the entries check nothing about the
 * indices - the caller range-checks them on the host - and the image's byte offset ids[i] * H * W is taken in 64 bits (a pool may
 * exceed 2 GiB).  Added within ABI 7 (pure additions).  All device pointers. */
/* = mlhot_ingest_u8_nhwc(pool[ids], C = 1, div).  Any H, W. */
int mlhot_pool1_ingest_u8(const uint8_t* pool, long n_pool, const int* ids, float* dst, long n_img, int H, int W, float div, void* stream);
/* = mlhot_augment_ingest_u8(pool[ids], C = 1, div, rec, luts).  H, W <= 128, MLHOT_ERR_UNSUPPORTED otherwise. */
int mlhot_pool1_augment_ingest_u8(const uint8_t* pool, long n_pool, const int* ids, float* dst, long n_img, int H, int W, float div,
                                  const mlhot_aug_record* rec, const uint8_t* luts, int n_luts, void* stream);
/* = mlhot_augment_ingest_u8_img(pool[ids], C = 1, pre_op, div, div2, rec, luts, colour_tabs).  H, W <= 128, MLHOT_ERR_UNSUPPORTED otherwise. */
int mlhot_pool1_augment_ingest_u8_img(const uint8_t* pool, long n_pool, const int* ids, float* dst, long n_img, int H, int W, int pre_op,
                                      float div, float div2, const mlhot_aug_record_img* rec, const uint8_t* luts, int n_luts,
                                      const void* colour_tabs, void* stream);

/* ---- optimizer: torch.optim.Adam (train.py:52-56) as ONE launch over flat buffers -------------------
 * param / grad / exp_avg / exp_avg_sq: n floats each, laid out alike (e.g. mlhot_np_grads_flat_layout).
 * step >= 1 is the 1-based update count (bias correction); grad_scale multiplies the gradient first
 * (1/world after a sum all-reduce); weight_decay is torch's L2 form (added to the gradient); amsgrad off.
 * beta1 / beta2 are doubles: 1 - beta and the bias corrections 1 - beta^step are formed in double from the caller's values and
 * rounded once (formed from a float beta2 = 0.999f, 1 - beta2 is off by 1.3e-5 of itself, and exp_avg_sq with it). */
int mlhot_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, double beta1, double beta2,
                    float eps, float weight_decay, float grad_scale, int step, void* stream);

/* The same update with the 1-based step count kept in device memory: *step_counter is incremented on the device first, then
 * used for the bias corrections.  Capture-safe - a replayed hipGraph of a whole training step advances the count by itself. */
int mlhot_adam_step_counter(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, double beta1,
                            double beta2, float eps, float weight_decay, float grad_scale, int* step_counter, void* stream);

/* ---- X1: ConvEmbeddingModel building blocks (networks/conv_embedding_model.py:99-184) -------------
 * Train-mode batch norm over the shots of ONE task, fused with the ReLU that follows it:
 * y = relu(gamma * (x - mean_c) / sqrt(var_c + eps) + beta) with per-channel batch statistics; like
 * F.batch_norm(training=True) it updates run_mean / run_var in place (momentum, unbiased variance).
 * mean / var [C] are returned for the backward.  x, y: [N, C, HW].                                 */
int mlhot_bn_relu_fwd(const float* x, const float* gamma, const float* beta, float* run_mean, float* run_var, float momentum, float eps,
                      int N, int C, int HW, float* y, float* mean, float* var, void* stream);
int mlhot_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* mean, const float* var, float eps,
                      int N, int C, int HW, float* dx, float* dgamma, float* dbeta, void* stream);
/* mean over the HW axis of `planes` maps (torch.mean(x.view(n, c, -1), dim=2), conv_embedding_model.py:119-123) */
int mlhot_spatial_mean_fwd(const float* x, float* y, int planes, int HW, void* stream);
int mlhot_spatial_mean_bwd(const float* dy, float* dx, int planes, int HW, void* stream);

/* ---- whole vanilla CNP/ANP model: forward + backward in one call each --------------------
 * replaces <Model>.forward for CNPVanillaPascal1D / CNPShapeNet1D / ANPVanillaPascal1D /
 * ANPShapeNet1D (CNPShapeNet1D.py:96-140, ANPShapeNet1D.py:93-157) and its autograd backward. */
#define MLHOT_MAX_HIDDEN 4
#define MLHOT_HEADS 8
typedef struct mlhot_np_dims {
  int T, Nc, Nq;              /* tasks, context shots, target shots (Nc may be 0)             */
  int label_dim, y_dim;       /* config.input_dim, config.output_dim                           */
  int dim_w, dim_r, dim_z;    /* 64, 64|100|256, 64                                            */
  int n_hidden;               /* len(n_hidden_units_r)                                         */
  int hidden[MLHOT_MAX_HIDDEN];
  int dec_hidden;             /* 100                                                           */
  int agg_mode;               /* MLHOT_AGG_*                                                   */
  int out_tanh;               /* 1 for the ShapeNet1D classes                                  */
  int m_feat;                 /* FAVOR+ features (attention only)                              */
} mlhot_np_dims;

typedef struct mlhot_np_params {
  mlhot_enc_params enc;
  const float *ty_w, *ty_b;                                   /* transform_y                  */
  const float *er_w[MLHOT_MAX_HIDDEN + 1], *er_b[MLHOT_MAX_HIDDEN + 1]; /* encoder_r.layers.{0,2,..} */
  const float *r2z_w, *r2z_b;                                 /* r_to_z                       */
  const float *dec_w[3], *dec_b[3];                           /* decoder0.{0,2,4}             */
  const float *mu_w, *mu_b, *var_w, *var_b;                   /* rs_to_mu / rs_to_var (baco)  */
  const float *wk_w[MLHOT_HEADS], *wk_b[MLHOT_HEADS];         /* _W_k.i.linear                */
  const float *wv_w[MLHOT_HEADS], *wv_b[MLHOT_HEADS];         /* _W_v.i.linear                */
  const float *wq_w[MLHOT_HEADS], *wq_b[MLHOT_HEADS];         /* _W_q.i.linear                */
  const float *wo_w, *wo_b;                                   /* _W.linear                    */
  const float *proj;                                          /* attn.projection_matrix       */
} mlhot_np_params;

typedef struct mlhot_np_grads {
  mlhot_enc_grads enc;
  float *ty_w, *ty_b;
  float *er_w[MLHOT_MAX_HIDDEN + 1], *er_b[MLHOT_MAX_HIDDEN + 1];
  float *r2z_w, *r2z_b;
  float *dec_w[3], *dec_b[3];
  float *mu_w, *mu_b, *var_w, *var_b;
  float *wk_w[MLHOT_HEADS], *wk_b[MLHOT_HEADS];
  float *wv_w[MLHOT_HEADS], *wv_b[MLHOT_HEADS];
  float *wq_w[MLHOT_HEADS], *wq_b[MLHOT_HEADS];
  float *wo_w, *wo_b;
} mlhot_np_grads;

size_t mlhot_np_struct_bytes(int which); /* 0 dims, 1 params, 2 grads, 3 chain_layer, 4 chain_grads, 5 linear_job: binding self-check */
size_t mlhot_np_saved_bytes(const mlhot_np_dims* d);
size_t mlhot_np_scratch_bytes(const mlhot_np_dims* d);
/* Recommended gradient layout: ONE flat fp32 buffer (what torch.optim / an all-reduce bucket want anyway,
 * train.py:52-56).  Fills the pointer fields of `offsets` with BYTE offsets into that buffer (null for parameters the
 * configuration does not have) and returns its size in floats.  mlhot_np_vanilla_bwd accepts any destination
 * pointers; when they follow this layout the per-task slab reduce of the fused tails is one contiguous sum. */
size_t mlhot_np_grads_flat_layout(const mlhot_np_dims* d, mlhot_np_grads* offsets);
/* ctx_x[T,Nc,1,128,128], ctx_y[T,Nc,label_dim], qry_x[T,Nq,1,128,128] -> mu[T,Nq,y_dim] */
int mlhot_np_vanilla_fwd(const mlhot_np_dims* d, const mlhot_np_params* p,
                         const float* ctx_x, const float* ctx_y, const float* qry_x, float* mu,
                         void* saved, void* scratch, size_t scratch_bytes, void* stream);
/* Every gradient buffer in g is OVERWRITTEN (parameters the forward did not use get zeros). */
int mlhot_np_vanilla_bwd(const mlhot_np_dims* d, const mlhot_np_params* p,
                         const float* ctx_x, const float* ctx_y, const float* qry_x,
                         const float* mu, const float* dmu, const mlhot_np_grads* g,
                         const void* saved, void* scratch, size_t scratch_bytes, void* stream);
/* The same backward taking the loss's gradient itself: trainer/model_trainer.py:77-79 computes `loss = calc_loss(mu, ., y)` and
 * calls loss.backward(); d loss / d mu of trainer/losses.py:32-80 needs no reduction, so the model's first backward kernel derives
 * it from (mu, gt) instead of reading a dmu that a separate launch wrote (the fused attention tail's specialised kernel does it in
 * its prologue; every other configuration materialises it first - same result either way):
 *   dmu_total = (dmu ? dmu : 0) + d loss(kind; mu, gt) / d mu * dloss[0]
 * kind: MLHOT_LOSS_* with a gradient (0 azimuth, 1 mse, 2 quaternion, 4 distractor); gt[T*Nq, gt_dim]; dloss: device scalar. */
typedef struct { int kind; const float* gt; int gt_dim; const float* dloss;
                 float* value;   /* ABI 5: NULL, or where this call also leaves the loss VALUE (what mlhot_loss_fwd(kind, mu, gt) writes, same
                                  * bits): one more workgroup of the first backward kernel instead of a launch between forward and backward */
} mlhot_loss_desc;
int mlhot_np_vanilla_bwd_loss(const mlhot_np_dims* d, const mlhot_np_params* p,
                              const float* ctx_x, const float* ctx_y, const float* qry_x,
                              const float* mu, const float* dmu, const mlhot_loss_desc* loss, const mlhot_np_grads* g,
                              const void* saved, void* scratch, size_t scratch_bytes, void* stream);
/* Staged variants (see "strict sharded parity" above).  Built on the fused attention tail's launch boundaries: attention
 * aggregation with Nc, Nq <= 16 (every shipped ANP configuration); MLHOT_ERR_UNSUPPORTED otherwise. */
int mlhot_np_vanilla_fwd_staged(const mlhot_np_dims* d, const mlhot_np_params* p,
                                const float* ctx_x, const float* ctx_y, const float* qry_x, float* mu,
                                void* saved, void* scratch, size_t scratch_bytes, int stage, float* xchg, void* stream);
int mlhot_np_vanilla_bwd_staged(const mlhot_np_dims* d, const mlhot_np_params* p,
                                const float* ctx_x, const float* ctx_y, const float* qry_x,
                                const float* mu, const float* dmu, const mlhot_np_grads* g,
                                const void* saved, void* scratch, size_t scratch_bytes, int stage, float* xchg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MLHOT_H */
