// Resident image pool: a training batch described by image ids, expanded on the device.
//
// The ShapeNet3D loader keeps an RGBA pool that never changes (dataset/shapenet_3d.py:113) and, every bg_gen_freq iterations, pastes a
// random background behind every object on the host (:235-239: rgb * mask + bg * (1 - mask), mask = alpha < 1.0).  Here the pool
// (uint8 [N, H, W, 4]) and the background bank (uint8 [B, H, W, 3]) live on the device, a batch crosses PCIe as its ids, and one
// kernel gathers image id[i], selects per pixel and channel c < 3
//     byte = (bg[i] >= 0 && pool[id][p][3] == 255) ? bank[bg[i]][p][c] : pool[id][p][c]
// and writes (float)byte / div as fp32 NCHW - the divide of ingest.h, so with bg = -1 the bits of mlhot_ingest_u8_nhwc(pool[ids, :, :, :3]).
//
// HBM-bound byte work like ingest.h's streaming kernel, which this follows: a lane owns a quad of 4 consecutive pixels = ONE 16-byte
// RGBA load (a wave reads 1 KiB of one image, or of a few small ones), three bank dwords only when some alpha of the quad is 255,
// three float4 stores; QPT quads in flight per lane.  Image and quad come from the flat quad index, so the grid fills the chip at any
// batch size; id and bg are per-lane loads (wave-uniform only when an image has >= 64 quads).  Ids and bg indices are range-checked
// on the host before they are shipped (mlhot/ingest.py); the kernels trust them.
//
// Below it, namespace pool1: the single-channel ("grey") pools of the 1D tasks and Distractor - a plain gather + divide.
#pragma once
#include "ingest.h"

namespace mlhot {
namespace pool {

// the rule, one byte at a time: what the any-size functor and the host build run, and what the augmenting ingest's source uses
MLHOT_HD uint8_t composed_byte(const uint8_t* __restrict__ px, const uint8_t* __restrict__ bank_px, int bg, int c) {
  return (bg >= 0 && px[3] == 255) ? bank_px[c] : px[c];
}

#ifndef MLHOT_HOSTSIM

using ingest::NT;
using ingest::QPT;
using ingest::QuadBytes;
using ingest::quad_byte;

__global__ __launch_bounds__(NT) void pool_gather_compose_kernel(const uint8_t* __restrict__ pool, const int* __restrict__ ids,
                                                                 const uint8_t* __restrict__ bank, const int* __restrict__ bg,
                                                                 float* __restrict__ dst, long n_quads, int quads_per_img, int HW, float div) {
  const long stride = (long)gridDim.x * NT;
  const long q0 = (long)blockIdx.x * NT + threadIdx.x;
  QuadBytes<4> px[QPT];          // 4 RGBA pixels
  QuadBytes<3> bk[QPT];          // the bank's 4 RGB pixels behind them
  int b[QPT];
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const long q = q0 + u * stride;
    b[u] = -1;
    px[u] = QuadBytes<4>{{0u, 0u, 0u, 0u}};
    if (q < n_quads) {
      const long img = q / quads_per_img;
      const int qi = (int)(q - img * quads_per_img);
      b[u] = bg[img];
      px[u] = *reinterpret_cast<const QuadBytes<4>*>(pool + ((long)ids[img] * HW + 4 * qi) * 4);
    }
  }
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const long q = q0 + u * stride;
    bk[u] = QuadBytes<3>{{0u, 0u, 0u}};
    // alpha = the top byte of a pixel's dword; an out-of-range quad has b = -1
    const bool any = (px[u].w[0] >> 24) == 255u || (px[u].w[1] >> 24) == 255u || (px[u].w[2] >> 24) == 255u || (px[u].w[3] >> 24) == 255u;
    if (b[u] >= 0 && any) {
      const long img = q / quads_per_img;
      const int qi = (int)(q - img * quads_per_img);
      bk[u] = *reinterpret_cast<const QuadBytes<3>*>(bank + ((long)b[u] * HW + 4 * qi) * 3);
    }
  }
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const long q = q0 + u * stride;
    if (q >= n_quads) continue;
    const long img = q / quads_per_img;
    const int p = (int)(q - img * quads_per_img) * 4;
    float* o = dst + img * 3L * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool sel = b[u] >= 0 && (px[u].w[j] >> 24) == 255u;
        const uint8_t byte = sel ? quad_byte<3>(bk[u], 3 * j + c) : (uint8_t)(px[u].w[j] >> (8 * c));
        v[j] = (float)byte / div;
      }
      *reinterpret_cast<float4*>(o + (long)c * HW) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

#endif  // !MLHOT_HOSTSIM

// any H * W and any alignment: one index per destination float
struct PoolAny {
  const uint8_t* pool; const int* ids; const uint8_t* bank; const int* bg; float* dst; int HW; float div;
  MLHOT_HD void operator()(size_t i) const {
    const size_t img = i / ((size_t)3 * HW);
    const int r = (int)(i - img * (size_t)3 * HW), c = r / HW, p = r - c * HW;
    const int b = bg[img];
    const uint8_t* px = pool + ((size_t)ids[img] * HW + p) * 4;
    dst[i] = (float)composed_byte(px, b >= 0 ? bank + ((size_t)b * HW + p) * 3 : px, b, c) / div;
  }
};

inline int run(const uint8_t* pool, const int* ids, const uint8_t* bank, const int* bg, float* dst, long n_img, int H, int W, float div,
               hipStream_t s) {
  const int HW = H * W;
  if (n_img == 0) return MLHOT_OK;
#ifndef MLHOT_HOSTSIM
  if ((HW & 3) == 0 && (reinterpret_cast<uintptr_t>(pool) & 3) == 0 && (reinterpret_cast<uintptr_t>(bank) & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const long n_quads = n_img * (long)(HW / 4);
    const int grid = (int)((n_quads + (long)NT * QPT - 1) / ((long)NT * QPT));
    ProfScope ps("pool.ingest.u8", s);
    hipLaunchKernelGGL(pool_gather_compose_kernel, dim3(grid), dim3(NT), 0, s, pool, ids, bank, bg, dst, n_quads, HW / 4, HW, div);
    return check_launch("pool.ingest.u8");
  }
#endif
  return run_foreach(PoolAny{pool, ids, bank, bg, dst, HW, div}, (size_t)n_img * 3 * HW, s, "pool.ingest.u8.any");
}

// ---- single-channel ("grey") pool: the 1D tasks and Distractor ----------------------------------------------------------
// pool: uint8 [N, H, W, 1] - the bytes the loaders' byte batches carry; no alpha, no bank.  Gather + the divide of ingest.h, so the bits
// of mlhot_ingest_u8_nhwc(pool[ids], C = 1).  ingest.h's C = 1 kernel with a gathered source: a lane owns a quad of 4 consecutive
// pixels of ONE image = one dword load and one float4 store, so a wave's store instruction writes 1 KiB in one piece; QPT quads in
// flight per lane; image and quad from the flat quad index, ids loaded per lane; the image's byte offset ids[img] * HW in 64 bits - a
// ShapeNet1D pool can exceed 2 GiB.  (A lane owning 16 bytes - one 16-byte load, four float4 stores - was measured first: 1.46 x the
// plain ingest, because each of its store instructions scatters 64 pieces of 16 bytes at a 64-byte stride)
namespace pool1 {

#ifndef MLHOT_HOSTSIM

__global__ __launch_bounds__(NT) void pool1_gather_kernel(const uint8_t* __restrict__ pool, const int* __restrict__ ids,
                                                          float* __restrict__ dst, long n_quads, int quads_per_img, int HW, float div) {
  const long stride = (long)gridDim.x * NT;
  const long q0 = (long)blockIdx.x * NT + threadIdx.x;
  uint32_t px[QPT];              // 4 grey pixels each
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const long q = q0 + u * stride;
    px[u] = 0u;
    if (q < n_quads) {
      const long img = q / quads_per_img;
      const int qi = (int)(q - img * quads_per_img);
      px[u] = *reinterpret_cast<const uint32_t*>(pool + (long)ids[img] * HW + 4 * qi);
    }
  }
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const long q = q0 + u * stride;
    if (q >= n_quads) continue;
    const uint32_t w = px[u];
    float4 v;
    v.x = (float)(uint8_t)(w) / div;
    v.y = (float)(uint8_t)(w >> 8) / div;
    v.z = (float)(uint8_t)(w >> 16) / div;
    v.w = (float)(uint8_t)(w >> 24) / div;
    reinterpret_cast<float4*>(dst)[q] = v;       // HW % 4 == 0: quad q of the batch is floats [4 q, 4 q + 4) of the destination
  }
}

#endif  // !MLHOT_HOSTSIM

// any H * W and any alignment: one index per destination float
struct Pool1Any {
  const uint8_t* pool; const int* ids; float* dst; int HW; float div;
  MLHOT_HD void operator()(size_t i) const {
    const size_t img = i / (size_t)HW;
    dst[i] = (float)pool[(size_t)ids[img] * HW + (i - img * (size_t)HW)] / div;
  }
};

inline int run(const uint8_t* pool, const int* ids, float* dst, long n_img, int H, int W, float div, hipStream_t s) {
  const int HW = H * W;
  if (n_img == 0) return MLHOT_OK;
#ifndef MLHOT_HOSTSIM
  if ((HW & 3) == 0 && (reinterpret_cast<uintptr_t>(pool) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const long n_quads = n_img * (long)(HW / 4);
    const int grid = (int)((n_quads + (long)NT * QPT - 1) / ((long)NT * QPT));
    ProfScope ps("pool1.ingest.u8", s);
    hipLaunchKernelGGL(pool1_gather_kernel, dim3(grid), dim3(NT), 0, s, pool, ids, dst, n_quads, HW / 4, HW, div);
    return check_launch("pool1.ingest.u8");
  }
#endif
  return run_foreach(Pool1Any{pool, ids, dst, HW, div}, (size_t)n_img * HW, s, "pool1.ingest.u8.any");
}

}  // namespace pool1

}  // namespace pool
}  // namespace mlhot
