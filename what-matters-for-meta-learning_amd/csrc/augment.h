// Device-side data augmentation ("DA") fused into the uint8 batch ingest.
//
// The reference augments on the host, per image, with an imgaug Sequential inside get_batch (dataset/shapenet_1d.py:174-176,
// dataset/pascal_1d.py:116-118; the sequences: dataset/shapenet_1d.py:34-72 AugmenterShapeNet1D, utils/augment.py:83-122
// PascalAugmenter).  Here the bytes of a staged batch are augmented where they are expanded to fp32: ONE workgroup per image reads
// the image once into LDS, applies that image's drawn op list (include/mlhot.h mlhot_aug_record, sampled on the host by
// mlhot/augment.py) in its drawn order between two byte planes, and writes (float)byte / div as fp32 NCHW once - the divide of
// ingest.h, so an image whose ops are all off comes out bit-identical to mlhot_ingest_u8_nhwc.
//
// The semantics are a written spec (DESIGN.md "Device augmentation", include/mlhot.h), restated from imgaug 0.4 / cv2: integer and
// fixed-point arithmetic wherever cv2 uses it; the few float steps (bicubic coefficients, numpy's linear_ramp) run with contraction
// off so that the host oracle (tests/augment_ref.py) reproduces them bit for bit.  Every per-pixel step is a functor over an index;
// the GPU runs it strided over the workgroup's 256 lanes with a barrier behind, the MLHOT_HOSTSIM build as a plain loop.
#pragma once
#include "common.h"
#include "../../include/mlhot.h"

namespace mlhot {
namespace aug {

constexpr int MAXD = 128;                 // H, W <= 128
constexpr int MAXPAD = 6;                 // round(0.05 * 128): CropAndPad's largest side
constexpr int MAXP = MAXD + 2 * MAXPAD;   // padded plane edge
constexpr int NT = 256;

// ---- counter-based hash (Dropout, CoarseDropout): murmur3's 32-bit finaliser, chained --------------------------------------------
MLHOT_HD uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
MLHOT_HD uint32_t image_key(const mlhot_aug_record& r) {
  uint32_t k = fmix32(r.seed + 0x9E3779B9u);
  k = fmix32(k ^ r.counter);
  k = fmix32(k ^ r.side);
  return fmix32(k ^ r.image);
}
MLHOT_HD uint32_t pixel_hash(uint32_t key, uint32_t item) { return fmix32(key ^ (item * 0x9E3779B1u)); }
constexpr uint32_t COARSE_CELL = 0x40000000u;     // CoarseDropout's cells hash as items 2^30 + cell (pixels are < 2^14)

// ---- border rules: where index p of a line of n lands (-1: the constant) ----------------------------------------------------------
MLHOT_HD int imod(int p, int m) { const int q = p % m; return q < 0 ? q + m : q; }
MLHOT_HD int border_index(int p, int n, int mode) {
  if (p >= 0 && p < n) return p;
  switch (mode) {
    case MLHOT_BORDER_CONSTANT: return -1;
    case MLHOT_BORDER_EDGE: return p < 0 ? 0 : n - 1;
    case MLHOT_BORDER_SYMMETRIC: { if (n == 1) return 0; const int q = imod(p, 2 * n); return q < n ? q : 2 * n - 1 - q; }     // cv2 REFLECT
    case MLHOT_BORDER_REFLECT: { if (n == 1) return 0; const int q = imod(p, 2 * n - 2); return q < n ? q : 2 * n - 2 - q; }   // REFLECT_101
    default: return imod(p, n);                                                                                                  // WRAP
  }
}

// ---- plane state of one image ---------------------------------------------------------------------------------------------------
struct Planes {
  uint8_t* cur; uint8_t* nxt;   // H x W ping-pong
  uint8_t* pad;                  // (H + pt + pb) x (W + pl + pr) CropAndPad plane
  int* stat;                     // per-line statistic of the pad modes (MAXP)
  int* flag;                     // linear_ramp: does any edge of a side equal the end value (2)
  int* coef;                     // bicubic: per output column then row, {first tap, 4 weights} (5 * 2 * MAXD)
};

MLHOT_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// round-half-to-even of s / n for s >= 0 (numpy's `around` of a mean; cv2's cvRound of a box mean)
MLHOT_HD int div_round_even(int s, int n) {
  const int q = s / n, r = s - q * n;
  return q + ((2 * r > n || (2 * r == n && (q & 1))) ? 1 : 0);
}

// One line of the pad plane: the pixels of the ORIGINAL region along `axis` (axis 0: column `idx`, rows pt .. pt+H-1; axis 1: row
// `idx` of the whole padded height, columns pl .. pl+W-1) - what numpy's np.pad reads for each axis (it pads axis 0 on the original
// columns, then axis 1 over every row, corners included).
struct Line {
  const uint8_t* p; int step, n;
  MLHOT_HD int at(int k) const { return p[k * step]; }
};
struct PadGeom {
  int H, W, pt, pr, pb, pl, Wp, Hp;
  MLHOT_HD Line line(const uint8_t* P, int axis, int idx) const {
    return axis == 0 ? Line{P + pt * Wp + pl + idx, Wp, H} : Line{P + idx * Wp + pl, 1, W};
  }
};

// median of a line (numpy: mean of the two middle values for an even count, then rounded half-to-even): k-th smallest by a
// bisection over the byte range
MLHOT_HD int kth(const Line& L, int k) {
  int lo = 0, hi = 255;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    int c = 0;
    for (int i = 0; i < L.n; ++i) c += L.at(i) <= mid;
    if (c > k) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// np.pad's statistic modes: one value per line, the same on both sides
struct PadStats {
  const uint8_t* P; PadGeom g; int axis, mode; int* stat;
  MLHOT_HD void operator()(int idx) const {
    const Line L = g.line(P, axis, idx);
    int v = 0;
    if (mode == MLHOT_PAD_MAXIMUM || mode == MLHOT_PAD_MINIMUM) {
      v = L.at(0);
      for (int i = 1; i < L.n; ++i) v = mode == MLHOT_PAD_MAXIMUM ? (L.at(i) > v ? L.at(i) : v) : (L.at(i) < v ? L.at(i) : v);
    } else if (mode == MLHOT_PAD_MEAN) {
      int s = 0;
      for (int i = 0; i < L.n; ++i) s += L.at(i);
      v = div_round_even(s, L.n);
    } else {                                                          // MEDIAN
      const int a = kth(L, (L.n - 1) / 2), b = (L.n & 1) ? a : kth(L, L.n / 2);
      v = div_round_even(a + b, 2);
    }
    stat[idx] = v;
  }
};

// linear_ramp: numpy's linspace switches formula for a whole side when ANY line's step is zero (an edge equal to the end value)
struct RampFlags {
  const uint8_t* P; PadGeom g; int axis, cval; int* flag;
  MLHOT_HD void operator()(int side) const {
    const int lines = axis == 0 ? g.W : g.Hp;
    int any = 0;
    for (int idx = 0; idx < lines; ++idx) {
      const Line L = g.line(P, axis, idx);
      any |= L.at(side == 0 ? 0 : L.n - 1) == cval;
    }
    flag[side] = any;
  }
};

// numpy linspace(end, edge, width, endpoint=False, dtype=uint8)[i]: float64 arange * step + start, floored
MLHOT_HD int ramp_value(int i, int width, int cval, int edge, int any_zero) {
#pragma clang fp contract(off)
  const double delta = (double)edge - (double)cval;
  double y;
  if (any_zero) { y = (double)i / (double)width; y = y * delta; }
  else { const double step = delta / (double)width; y = (double)i * step; }
  y = y + (double)cval;
  return (int)floor(y);
}

// fills the pad area of one axis: axis 0 = rows pt above and pb below, over the original columns; axis 1 = columns pl left and pr
// right, over the whole padded height
struct PadFill {
  uint8_t* P; PadGeom g; int axis, mode, cval; const int* stat; const int* flag;
  MLHOT_HD void operator()(int i) const {
    int idx, j, lo, hi;                                  // line, position in the pad area, pad widths of the two sides
    if (axis == 0) { lo = g.pt; hi = g.pb; idx = i % g.W; j = i / g.W; }
    else { lo = g.pl; hi = g.pr; const int w = lo + hi; idx = i / w; j = i - idx * w; }
    const Line L = g.line(P, axis, idx);
    const int side = j < lo ? 0 : 1;
    const int d = side == 0 ? lo - j : j - lo + 1;       // distance from the line's end, 1 .. width
    const int width = side == 0 ? lo : hi;
    int v;
    switch (mode) {
      case MLHOT_PAD_CONSTANT: v = cval; break;
      case MLHOT_PAD_EDGE: v = L.at(side == 0 ? 0 : L.n - 1); break;
      case MLHOT_PAD_LINEAR_RAMP: v = ramp_value(width - d, width, cval, L.at(side == 0 ? 0 : L.n - 1), flag[side]); break;
      case MLHOT_PAD_MAXIMUM: case MLHOT_PAD_MEAN: case MLHOT_PAD_MEDIAN: case MLHOT_PAD_MINIMUM: v = stat[idx]; break;
      default: {
        const int bm = mode == MLHOT_PAD_REFLECT ? MLHOT_BORDER_REFLECT : mode == MLHOT_PAD_SYMMETRIC ? MLHOT_BORDER_SYMMETRIC : MLHOT_BORDER_WRAP;
        v = L.at(border_index(side == 0 ? -d : L.n - 1 + d, L.n, bm));
      }
    }
    uint8_t* dst = axis == 0 ? P + (side == 0 ? j : g.pt + g.H + (j - lo)) * g.Wp + g.pl + idx
                             : P + idx * g.Wp + (side == 0 ? j : g.pl + g.W + (j - lo));
    *dst = (uint8_t)v;
  }
};

struct CopyIn {             // the image into the pad plane's interior
  const uint8_t* src; uint8_t* P; PadGeom g;
  MLHOT_HD void operator()(int i) const { const int y = i / g.W, x = i - y * g.W; P[(g.pt + y) * g.Wp + g.pl + x] = src[i]; }
};

// cv2.resize INTER_CUBIC of uint8 (imgaug's keep_size resize): A = -0.75, half-pixel centres, coefficients in float rounded to
// 1/2048 (cvRound), replicated border, sum of 16 integer products rounded at 2^22 and saturated.  Entry i < W: output column i;
// W <= i < W + H: output row i - W.
struct CubicCoef {
  int* coef; int W, H, Wp, Hp;
  MLHOT_HD void operator()(int i) const {
#pragma clang fp contract(off)
    const bool col = i < W;
    const int d = col ? i : i - W, dn = col ? W : H, sn = col ? Wp : Hp;
    const double scale = (double)sn / (double)dn;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f = f - (float)s;
    const float A = -0.75f, x1 = f + 1.f, r = 1.f - f;
    const float w0 = ((A * x1 - 5.f * A) * x1 + 8.f * A) * x1 - 4.f * A;
    const float w1 = (((A + 2.f) * f - (A + 3.f)) * f) * f + 1.f;
    const float w2 = (((A + 2.f) * r - (A + 3.f)) * r) * r + 1.f;
    const float w3 = 1.f - w0 - w1 - w2;
    int* c = coef + 5 * i;
    c[0] = s - 1;
    c[1] = (int)rintf(w0 * 2048.f); c[2] = (int)rintf(w1 * 2048.f); c[3] = (int)rintf(w2 * 2048.f); c[4] = (int)rintf(w3 * 2048.f);
  }
};
struct CopyInCoef {
  CopyIn copy; CubicCoef coef; int HW;
  MLHOT_HD void operator()(int i) const { if (i < HW) copy(i); else coef(i - HW); }
};

struct CubicResize {
  const uint8_t* P; uint8_t* dst; const int* coef; int W, H, Wp, Hp;
  MLHOT_HD void operator()(int i) const {
    const int y = i / W, x = i - y * W;
    const int* cx = coef + 5 * x;
    const int* cy = coef + 5 * (W + y);
    int acc = 0;
    for (int k = 0; k < 4; ++k) {
      const uint8_t* row = P + clampi(cy[0] + k, 0, Hp - 1) * Wp;
      int h = 0;
      for (int j = 0; j < 4; ++j) h += cx[1 + j] * row[clampi(cx[0] + j, 0, Wp - 1)];
      acc += cy[1 + k] * h;
    }
    dst[i] = (uint8_t)clampi((acc + (1 << 21)) >> 22, 0, 255);
  }
};

struct Gamma {               // per-image LUT built on the host
  uint8_t* p; const uint8_t* lut;
  MLHOT_HD void operator()(int i) const { p[i] = lut[p[i]]; }
};

struct BoxBlur {             // cv2.blur: k x k mean, anchor k / 2, BORDER_REFLECT_101, rounded half to even
  const uint8_t* src; uint8_t* dst; int W, H, k;
  MLHOT_HD void operator()(int i) const {
    const int y = i / W, x = i - y * W, a = k / 2;
    int s = 0;
    for (int dy = 0; dy < k; ++dy) {
      const uint8_t* row = src + border_index(y - a + dy, H, MLHOT_BORDER_REFLECT) * W;
      for (int dx = 0; dx < k; ++dx) s += row[border_index(x - a + dx, W, MLHOT_BORDER_REFLECT)];
    }
    dst[i] = (uint8_t)div_round_even(s, k * k);
  }
};

// cv2.warpAffine of uint8 with the inverse map in 1/65536 px (src_x = (ax * x + bx) / 2^16; no shear / rotation in these
// sequences): order 0 = nearest (rounded), order 1 = bilinear on the 1/32-px grid with weights in 1/32768, rounded at 2^15
struct AffineWarp {
  const uint8_t* src; uint8_t* dst; int W, H, ax, bx, ay, by, order, mode, cval;
  MLHOT_HD int tap(int yy, int xx) const {
    const int sy = border_index(yy, H, mode), sx = border_index(xx, W, mode);
    return (sy < 0 || sx < 0) ? cval : src[sy * W + sx];
  }
  MLHOT_HD void operator()(int i) const {
    const int y = i / W, x = i - y * W;
    const int X = ax * x + bx, Y = ay * y + by;
    if (order == 0) { dst[i] = (uint8_t)tap((Y + 32768) >> 16, (X + 32768) >> 16); return; }
    const int Xq = (X + 1024) >> 11, Yq = (Y + 1024) >> 11;
    const int x0 = Xq >> 5, y0 = Yq >> 5, fx = Xq & 31, fy = Yq & 31;
    const int v = (32 - fy) * ((32 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) * 32
                + fy * ((32 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)) * 32;
    dst[i] = (uint8_t)clampi((v + (1 << 14)) >> 15, 0, 255);
  }
};

struct Dropout {
  uint8_t* p; uint32_t key, thresh;
  MLHOT_HD void operator()(int i) const { if (pixel_hash(key, (uint32_t)i) < thresh) p[i] = 0; }
};

struct CoarseDropout {       // a ch x cw keep-mask of Bernoulli(1 - p) cells, upscaled by nearest neighbour (src = dst * n_src / n_dst)
  uint8_t* p; uint32_t key, thresh; int W, H, ch, cw;
  int cell0 = 0;             // first cell of this plane (augment_img.h: per_channel masks); 0 for one plane
  MLHOT_HD void operator()(int i) const {
    const int y = i / W, x = i - y * W;
    const int cell = cell0 + (y * ch / H) * cw + x * cw / W;
    if (pixel_hash(key, COARSE_CELL + (uint32_t)cell) < thresh) p[i] = 0;
  }
};

// ---- the per-image op list: Exec runs a functor over [0, n) and then waits for the whole workgroup --------------------------------
template <class Exec>
MLHOT_DEV void augment_image(const Exec& ex, const mlhot_aug_record& r, const uint8_t* luts, int n_luts, int H, int W, Planes& pl) {
  const int HW = H * W;
  const int n_steps = clampi(r.n_steps, 0, 7);
  for (int s = 0; s < n_steps; ++s) {
    const int op = r.op[s];
    if (op < 0 || op > 5 || !((r.on >> op) & 1)) continue;
    if (op == MLHOT_AUG_CROP_PAD) {
      PadGeom g{H, W, clampi(r.pad[0], 0, MAXPAD), clampi(r.pad[1], 0, MAXPAD), clampi(r.pad[2], 0, MAXPAD), clampi(r.pad[3], 0, MAXPAD), 0, 0};
      if ((g.pt | g.pr | g.pb | g.pl) == 0) continue;             // nothing padded: no resize either
      g.Wp = W + g.pl + g.pr; g.Hp = H + g.pt + g.pb;
      const int mode = clampi(r.pad_mode, 0, 9), cval = r.pad_cval & 255;
      const bool stats = mode >= MLHOT_PAD_MAXIMUM && mode <= MLHOT_PAD_MINIMUM;
      ex(HW + W + H, CopyInCoef{CopyIn{pl.cur, pl.pad, g}, CubicCoef{pl.coef, W, H, g.Wp, g.Hp}, HW});   // independent of each other
      for (int axis = 0; axis < 2; ++axis) {
        if (stats) ex(axis == 0 ? W : g.Hp, PadStats{pl.pad, g, axis, mode, pl.stat});
        if (mode == MLHOT_PAD_LINEAR_RAMP) ex(2, RampFlags{pl.pad, g, axis, cval, pl.flag});
        ex(axis == 0 ? (g.pt + g.pb) * W : (g.pl + g.pr) * g.Hp, PadFill{pl.pad, g, axis, mode, cval, pl.stat, pl.flag});
      }
      ex(HW, CubicResize{pl.pad, pl.nxt, pl.coef, W, H, g.Wp, g.Hp});
    } else if (op == MLHOT_AUG_GAMMA) {
      if (n_luts <= 0) continue;
      ex(HW, Gamma{pl.cur, luts + 256 * clampi(r.lut, 0, n_luts - 1)});
      continue;
    } else if (op == MLHOT_AUG_BLUR) {
      const int k = clampi(r.blur_k, 1, 3);
      if (k == 1) continue;
      ex(HW, BoxBlur{pl.cur, pl.nxt, W, H, k});
    } else if (op == MLHOT_AUG_AFFINE) {
      ex(HW, AffineWarp{pl.cur, pl.nxt, W, H, r.aff_ax, r.aff_bx, r.aff_ay, r.aff_by, r.aff_order & 1, clampi(r.aff_mode, 0, 4), r.aff_cval & 255});
    } else if (op == MLHOT_AUG_DROPOUT) {
      ex(HW, Dropout{pl.cur, image_key(r), r.drop_thresh});
      continue;
    } else {
      ex(HW, CoarseDropout{pl.cur, image_key(r), r.coarse_thresh, W, H, clampi(r.coarse_h, 1, MAXD), clampi(r.coarse_w, 1, MAXD)});
      continue;
    }
    uint8_t* t = pl.cur; pl.cur = pl.nxt; pl.nxt = t;            // spatial ops wrote the other plane
  }
}

// ---- where the load stage finds image `img`'s H * W bytes: packed one behind the other (mlhot_augment_ingest_u8), or image ids[img] of
// the resident grey pool (mlhot_pool1_augment_ingest_u8; the byte offset in 64 bits - a pool can exceed 2 GiB) ---------
struct PackedSrc {
  const uint8_t* src;
  MLHOT_HD const uint8_t* image(long img, int HW) const { return src + img * HW; }
};
struct GreyPoolSrc {
  const uint8_t* pool; const int* ids;
  MLHOT_HD const uint8_t* image(long img, int HW) const { return pool + (long)ids[img] * HW; }
};

#ifndef MLHOT_HOSTSIM
struct BlockExec {
  template <class F>
  __device__ __forceinline__ void operator()(int n, const F f) const {
    for (int i = threadIdx.x; i < n; i += NT) f(i);
    __syncthreads();
  }
};

template <class Src>
__global__ __launch_bounds__(NT) void augment_ingest_kernel(const Src src, float* __restrict__ dst, int H, int W,
                                                            float div, const mlhot_aug_record* __restrict__ rec,
                                                            const uint8_t* __restrict__ luts, int n_luts, int vec) {
  __shared__ uint8_t s_a[MAXD * MAXD], s_b[MAXD * MAXD], s_pad[MAXP * MAXP];
  __shared__ int s_stat[MAXP], s_flag[2], s_coef[5 * 2 * MAXD];
  const long img = blockIdx.x;
  const int HW = H * W;
  const uint8_t* __restrict__ s = src.image(img, HW);
  if (vec) {                                                          // HW % 4 == 0, 4-byte aligned: one dword per lane step
    for (int q = threadIdx.x; q < HW / 4; q += NT) reinterpret_cast<uint32_t*>(s_a)[q] = reinterpret_cast<const uint32_t*>(s)[q];
  } else {
    for (int i = threadIdx.x; i < HW; i += NT) s_a[i] = s[i];
  }
  __syncthreads();
  Planes pl{s_a, s_b, s_pad, s_stat, s_flag, s_coef};
  augment_image(BlockExec{}, rec[img], luts, n_luts, H, W, pl);     // the record is read from global memory where it is used
  float* o = dst + img * HW;
  if (vec) {                                                          // the divide of ingest.h: (float)byte / div, float4 stores
    for (int q = threadIdx.x; q < HW / 4; q += NT) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(pl.cur)[q];
      float4 v;
      v.x = (float)(uint8_t)(w) / div;
      v.y = (float)(uint8_t)(w >> 8) / div;
      v.z = (float)(uint8_t)(w >> 16) / div;
      v.w = (float)(uint8_t)(w >> 24) / div;
      reinterpret_cast<float4*>(o)[q] = v;
    }
  } else {
    for (int i = threadIdx.x; i < HW; i += NT) o[i] = (float)pl.cur[i] / div;
  }
}
#else
struct LoopExec {
  template <class F>
  void operator()(int n, const F& f) const { for (int i = 0; i < n; ++i) f(i); }
};
#endif

// base: the pointer the images are read from (its alignment decides the dword loads)
template <class Src>
inline int run_src(const Src& src, const uint8_t* base, float* dst, long n_img, int H, int W, float div, const mlhot_aug_record* rec,
                   const uint8_t* luts, int n_luts, hipStream_t s, const char* what) {
  if (n_img == 0) return MLHOT_OK;
#ifndef MLHOT_HOSTSIM
  const int HW = H * W;
  const int vec = (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  ProfScope ps(what, s);
  hipLaunchKernelGGL(augment_ingest_kernel<Src>, dim3((unsigned)n_img), dim3(NT), 0, s, src, dst, H, W, div, rec, luts, n_luts, vec);
  return check_launch(what);
#else
  (void)s; (void)base; (void)what;
  static thread_local uint8_t a[MAXD * MAXD], b[MAXD * MAXD], pad[MAXP * MAXP];
  static thread_local int stat[MAXP], flag[2], coef[5 * 2 * MAXD];
  const int HW = H * W;
  for (long img = 0; img < n_img; ++img) {
    memcpy(a, src.image(img, HW), (size_t)HW);
    Planes pl{a, b, pad, stat, flag, coef};
    augment_image(LoopExec{}, rec[img], luts, n_luts, H, W, pl);
    for (int i = 0; i < HW; ++i) dst[img * HW + i] = (float)pl.cur[i] / div;
  }
  return MLHOT_OK;
#endif
}

inline int run(const uint8_t* src, float* dst, long n_img, int H, int W, float div, const mlhot_aug_record* rec, const uint8_t* luts,
               int n_luts, hipStream_t s) {
  return run_src(PackedSrc{src}, src, dst, n_img, H, W, div, rec, luts, n_luts, s, "augment.ingest.u8");
}

inline int run_pool1(const uint8_t* pool, const int* ids, float* dst, long n_img, int H, int W, float div, const mlhot_aug_record* rec,
                     const uint8_t* luts, int n_luts, hipStream_t s) {
  return run_src(GreyPoolSrc{pool, ids}, pool, dst, n_img, H, W, div, rec, luts, n_luts, s, "pool1.augment.ingest.u8");
}

}  // namespace aug
}  // namespace mlhot
