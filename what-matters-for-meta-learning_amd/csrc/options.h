// Run-time switches (mlhot_set_option): which implementation of a hot-path row runs.  The generic igemm problems are always
// available as the A/B reference of the specialised kernels.  Every switch lives here, with its default; mlhot_set_option's table
// (mlhot.hip) is the only writer.  Readers: enc_route() (encoder.h) for the encoder's, np_route() (np_vanilla.h) for the tail's,
// trunk_route() (resnet_trunk.h) for the three trunk_* ones, favor2.h for its own and favor_linear's.
#pragma once

namespace mlhot {

// Option "tail_spec": which parts of a fused tail run the kernels specialised for the shipped dimensions (csrc/tail_spec.h,
// cnp_spec.h) instead of the run-time-shaped ones (tail_fused.h, tail_cnp.h).  A clear bit is the A/B reference of a set one.  The
// CNP tail is one kernel per direction: it reads FWD_A / BWD_C as "forward" / "backward", and ENC_FOLD, LOSS, BWD_C_WG2, WG4 with them.
// np_route() (np_vanilla.h) is the only reader.
enum TailSpec : int {
  TAIL_SPEC_FWD_A = 1,         // forward phase A (transform_y, EncoderFC, K projection)
  TAIL_SPEC_FWD_B = 2,         // forward phase B (V / Q projections, FAVOR+, the heads' _W shares)
  TAIL_SPEC_FWD_C = 4,         // forward phase C (_W, r_to_z, decoder0)
  TAIL_SPEC_BWD_C = 8,         // backward phase C'
  TAIL_SPEC_BWD_B = 16,        // backward phase B'
  TAIL_SPEC_BWD_A = 32,        // backward phase A'
  TAIL_SPEC_ENC_FOLD = 64,     // phase A also folds the encoder Linear's split-K partial results
  TAIL_SPEC_LOSS = 128,        // phase C' takes the loss's gradient itself when handed a loss descriptor
                               // (256: unassigned)
  TAIL_SPEC_BWD_B_SPLIT = 512, // phase B' as two workgroups per (task, head): query side | key / value side
  TAIL_SPEC_BWD_C_WG2 = 1024,  // phase C' as two workgroups per task sharing the weight-gradient tiles
  TAIL_SPEC_BWD_A_WG2 = 2048,  // phase A' likewise
  TAIL_SPEC_WG4 = 4096,        // four workgroups instead of two, wherever one of the two bits above is set
  TAIL_SPEC_DEFAULT = TAIL_SPEC_FWD_A | TAIL_SPEC_FWD_B | TAIL_SPEC_FWD_C | TAIL_SPEC_BWD_C | TAIL_SPEC_BWD_B | TAIL_SPEC_BWD_A |
                      TAIL_SPEC_ENC_FOLD | TAIL_SPEC_LOSS | TAIL_SPEC_BWD_B_SPLIT | TAIL_SPEC_BWD_C_WG2 | TAIL_SPEC_BWD_A_WG2 |
                      TAIL_SPEC_WG4,
};
static_assert(TAIL_SPEC_DEFAULT == 7935, "the numeric values are public: tests, scripts and MLHOT_OPTS pass numbers");

struct Options {
  int conv2_tc = 1;          // the encoder's weight-stationary kernels (conv_tc.h, conv3_tc.h, enc_linear.h); 0: the generic igemm chain
  int conv2_split = 0;       // bits: 1 forward, 2 data gradient, 4 weight gradient of conv2 on the bf16 pipe over split operands (conv_split.h)
  int tail_fused = 1;        // the fused tails (tail_fused.h, tail_cnp.h); 0: the operator chain
  int tail_spec = TAIL_SPEC_DEFAULT;      // bit mask, enum TailSpec
  int conv3_bwd_merged = 1;  // 0: two launches; 1: one launch, 128 + 128 workgroups; n > 1: n weight-gradient workgroups of 256
  int materialize_a1 = 0;    // the fused conv1 + conv2 forward never stores conv1's output; 1: a launch of its own keeps it (tests)
  int dbg = 0;               // timing experiments only (results become wrong)
  int favor2 = 1;            // FAVOR+: the two-launch kernels (favor2.h); 0: favor.h's chain
  int favor_linear = 0;      // FAVOR+ above 32 shots on either side: 1 the linear form (favor_linear.h), 0 favor.h's chain.  As with favor2, it
                             // must not change between a forward and the backward that reuses its workspace: the routes carve differently
  int trunk_dual_dgrad = 1;  // a 3x3-skip block's two stride-2 data gradients in one 512-thread launch (resnet_ws.h dgrad2_dual_kernel)
  int trunk_wg_rows = 128;   // slab rows (x 4 channel tiles = workgroups) a trunk weight-gradient launch is planned against; 16 .. 128
  int trunk_fuse34 = 1;      // blocks 3-4 of a 64 x 64 trunk as one launch per direction (resnet_ws.h tail34_*)
};
extern Options g_opt;

}  // namespace mlhot
