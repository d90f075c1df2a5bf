// Device-side data augmentation of the IMAGE tasks (shapenet_3d: utils/augment.py:22-63 Augmenter; distractor:
// dataset/shapenet_distractor.py:54-81 AugmenterDistractor), fused into the uint8 batch ingest like augment.h, whose functors it runs
// once per channel plane: ONE workgroup per image de-interleaves the channel-last bytes into planar LDS ([C][H][W]; two ping-pong
// plane sets and a pad plane set), applies the image's drawn op list (include/mlhot.h mlhot_aug_record_img) in its drawn order with a
// barrier behind each op, and writes (float)byte / div / div2 as fp32 NCHW once - the planar LDS index IS the NCHW index.
//
// New against augment.h: three channels through every op, AddToBrightness with its six colour spaces (integer / fixed point; Lab and
// Luv through host-built tables, mlhot_colour_tabs), per_channel dropouts, the loaders' byte handling (pre_op, div2).  The spec is
// DESIGN.md 6a-2 and include/mlhot.h; tests/augment_img_ref.py restates it in numpy and this file matches that bit for bit.
//
// The de-interleave stage reads through a source functor: NhwcSrc, the packed channel-last bytes (mlhot_augment_ingest_u8_img),
// PoolSrc, image ids[i] of the resident RGBA pool composed over the background bank (mlhot_pool_augment_ingest_u8_img), or
// GreyPoolImgSrc, image ids[i] of the resident single-channel pool (mlhot_pool1_augment_ingest_u8_img).
#pragma once
#include "augment.h"
#include "pool_ingest.h"

namespace mlhot {
namespace augimg {

using namespace aug;

constexpr int MAXD3 = 64;                              // H, W <= 64 at C = 3 (<= MAXD = 128 at C = 1)
constexpr int SET_BYTES = MAXD * MAXD;                 // one plane set: 128 x 128 x 1 >= 3 x 64 x 64
constexpr int PAD_BYTES = MAXP * MAXP;                 // 140 x 140 x 1 = 19600 >= 3 x 76 x 76 = 17328
constexpr int MAXC = 3;

struct PlaneSets {
  uint8_t* cur; uint8_t* nxt; uint8_t* pad;            // plane c of a set at + c * H * W (pad: + c * Hp * Wp)
  int* stat;                                           // MAXC * MAXP
  int* flag;                                           // [0, 2): the sides' flags over all channels; [2 + 2 c, 4 + 2 c): channel c's
  int* coef;                                           // shared by the channels (one geometry)
};

// runs make(c) - a functor of augment.h bound to plane c - over [0, n) per plane: index i -> plane i / n, item i % n
template <class Make>
struct PerPlane {
  Make make; int n;
  MLHOT_HD void operator()(int i) const { const int c = i / n; make(c)(i - c * n); }
};
template <class Make>
MLHOT_HD PerPlane<Make> per_plane(int n, Make make) { return PerPlane<Make>{make, n}; }

struct CopyInPlanesCoef {     // every plane into its pad plane's interior, and the (shared) bicubic coefficients
  const uint8_t* src; uint8_t* P; PadGeom g; CubicCoef coef; int HW, CHW;
  MLHOT_HD void operator()(int i) const {
    if (i >= CHW) { coef(i - CHW); return; }
    const int c = i / HW;
    CopyIn{src + c * HW, P + c * g.Hp * g.Wp, g}(i - c * HW);
  }
};

struct OrFlags {              // numpy's linspace asks `any(step == 0)` over the whole edge array: all channels of a side
  int* flag; int C;
  MLHOT_HD void operator()(int side) const {
    int any = 0;
    for (int c = 0; c < C; ++c) any |= flag[2 + 2 * c + side];
    flag[side] = any;
  }
};

// ---- AddToBrightness -----------------------------------------------------------------------------------------------------------
MLHOT_HD int sat8(int v) { return clampi(v, 0, 255); }
MLHOT_HD int64_t fdiv64(int64_t a, int64_t b) {        // floor(a / b), b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
MLHOT_HD int64_t rdiv64(int64_t a, int64_t b) { return fdiv64(2 * a + b, 2 * b); }
MLHOT_HD int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
MLHOT_HD int min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

struct Rgb { int r, g, b; };

// Y Cr Cb / Y U V: 14-bit fixed point; k = {c1 (first chroma, of d1), c2 (second, of d2), back: r, g1, g2, b}
MLHOT_HD Rgb bright_ycc(Rgb p, int add, bool yuv) {
  const int Y = (4899 * p.r + 9617 * p.g + 1868 * p.b + 8192) >> 14;
  const int half = (128 << 14) + 8192;
  if (!yuv) {
    const int Cr = sat8(((p.r - Y) * 11682 + half) >> 14), Cb = sat8(((p.b - Y) * 9241 + half) >> 14);
    const int y = sat8(Y + add), cr = Cr - 128, cb = Cb - 128;
    return Rgb{sat8(y + ((cr * 22987 + 8192) >> 14)), sat8(y + ((cr * -11698 + cb * -5636 + 8192) >> 14)), sat8(y + ((cb * 29049 + 8192) >> 14))};
  }
  const int U = sat8(((p.b - Y) * 8061 + half) >> 14), V = sat8(((p.r - Y) * 14369 + half) >> 14);
  const int y = sat8(Y + add), u = U - 128, v = V - 128;
  return Rgb{sat8(y + ((v * 18678 + 8192) >> 14)), sat8(y + ((u * -6472 + v * -9519 + 8192) >> 14)), sat8(y + ((u * 33292 + 8192) >> 14))};
}

MLHOT_HD int hue180(Rgb p, int mx, int d) {            // degrees / 2, 0 .. 179
  if (d == 0) return 0;
  int n = mx == p.r ? 30 * (p.g - p.b) : mx == p.g ? 30 * (p.b - p.r) + 60 * d : 30 * (p.r - p.g) + 120 * d;
  if (n < 0) n += 180 * d;
  const int h = (2 * n + d) / (2 * d);
  return h >= 180 ? h - 180 : h;
}

MLHOT_HD Rgb bright_hsv(Rgb p, int add) {
  const int mx = max3(p.r, p.g, p.b), d = mx - min3(p.r, p.g, p.b);
  const int S = mx ? (510 * d + mx) / (2 * mx) : 0, H = hue180(p, mx, d);
  const int V = sat8(mx + add);
  const int i = H / 30, f = H - 30 * i;
  const int P = (2 * V * (255 - S) + 255) / 510, Qv = (2 * V * (7650 - S * f) + 7650) / 15300, T = (2 * V * (7650 - S * (30 - f)) + 7650) / 15300;
  switch (i) {
    case 0: return Rgb{V, T, P};
    case 1: return Rgb{Qv, V, P};
    case 2: return Rgb{P, V, T};
    case 3: return Rgb{P, Qv, V};
    case 4: return Rgb{T, P, V};
    default: return Rgb{V, P, Qv};
  }
}

MLHOT_HD int hls_channel(int P1, int P2, int h) {
  h = h < 0 ? h + 180 : h >= 180 ? h - 180 : h;
  const int N = h < 30 ? 30 * P1 + (P2 - P1) * h : h < 90 ? 30 * P2 : h < 120 ? 30 * P1 + (P2 - P1) * (120 - h) : 30 * P1;
  return sat8((2 * N + 7650) / 15300);
}
MLHOT_HD Rgb bright_hls(Rgb p, int add) {
  const int mx = max3(p.r, p.g, p.b), mn = min3(p.r, p.g, p.b), d = mx - mn, m = mx + mn <= 255 ? mx + mn : 510 - mx - mn;
  const int S = d == 0 ? 0 : sat8((510 * d + m) / (2 * m)), H = hue180(p, mx, d);
  const int L = sat8(((mx + mn + 1) >> 1) + add);
  const int P2 = L <= 127 ? L * (255 + S) : 255 * L + 255 * S - L * S, P1 = 510 * L - P2;
  return Rgb{hls_channel(P1, P2, H + 60), hls_channel(P1, P2, H), hls_channel(P1, P2, H - 60)};
}

constexpr int CS_Q = MLHOT_CS_Q;
constexpr int64_t CS_D = 1479000;                                    // f = N / D: exact for every 8-bit L, a, b
constexpr int64_t CS_K = CS_D * CS_D * CS_D / CS_Q;                  // D^3 / Q (an integer: Q divides D^3)
static_assert(CS_K * CS_Q == CS_D * CS_D * CS_D, "Q must divide D^3");

MLHOT_HD int lin_of_f(int64_t N) {                                   // the inverse of f[] on N / D: linear light on 0 .. 2 Q
  int64_t t;
  if (29 * N > 6 * CS_D) t = (int64_t)(((uint64_t)(N * N * N) + (uint64_t)(CS_K / 2)) / (uint64_t)CS_K);
  else { t = rdiv64((int64_t)CS_Q * 108 * (29 * N - 4 * CS_D), 24389 * CS_D); if (t < 0) t = 0; }
  return (int)(t > 2 * CS_Q ? 2 * CS_Q : t);
}

MLHOT_HD Rgb bright_lab_luv(Rgb p, int add, bool luv, const mlhot_colour_tabs& ct) {
  const int lr = ct.lin[p.r], lg = ct.lin[p.g], lb = ct.lin[p.b];
  const int x = (ct.m[0] * lr + ct.m[1] * lg + ct.m[2] * lb + 2048) >> 12;
  const int y = (ct.m[3] * lr + ct.m[4] * lg + ct.m[5] * lb + 2048) >> 12;
  const int z = (ct.m[6] * lr + ct.m[7] * lg + ct.m[8] * lb + 2048) >> 12;
  const int Fy = ct.f[clampi(y, 0, CS_Q)];
  const int64_t Ln = 116 * (int64_t)Fy - (16 << 15);
  const int L8 = sat8((int)((2 * 255 * Ln + (100 << 15)) / (200 << 15)));
  const int l = sat8(L8 + add);
  const int64_t Ny = 5000 * (int64_t)l + 204000;
  int X, Y = lin_of_f(Ny), Z;
  if (!luv) {
    const int Fx = ct.f[clampi(x, 0, CS_Q)], Fz = ct.f[clampi(z, 0, CS_Q)];
    const int a8 = sat8(128 + ((500 * (Fx - Fy) + 16384) >> 15)), b8 = sat8(128 + ((200 * (Fy - Fz) + 16384) >> 15));
    X = lin_of_f(Ny + 2958 * (int64_t)(a8 - 128));
    Z = lin_of_f(Ny - 7395 * (int64_t)(b8 - 128));
  } else {
    const int64_t d = (int64_t)ct.xn * x + 15 * 4096 * (int64_t)y + 3 * (int64_t)ct.zn * z;
    const int64_t up = d == 0 ? ct.un : (2 * (4 * (int64_t)ct.xn * x << 16) + d) / (2 * d);
    const int64_t vp = d == 0 ? ct.vn : (2 * (9 * 4096 * (int64_t)y << 16) + d) / (2 * d);
    const int u8 = sat8(97 + (int)rdiv64(255 * 13 * Ln * (up - ct.un), 354 * ((int64_t)1 << 31)));
    const int v8 = sat8(136 + (int)rdiv64(255 * 13 * Ln * (vp - ct.vn), 262 * ((int64_t)1 << 31)));
    if (l == 0) { X = 0; Z = 0; }
    else {
      int64_t u2 = ct.un + rdiv64(354 * 65536 * (int64_t)(u8 - 97), 1300 * (int64_t)l);
      int64_t v2 = ct.vn + rdiv64(262 * 65536 * (int64_t)(v8 - 136), 1300 * (int64_t)l);
      if (v2 < 1) v2 = 1;
      if (u2 < 0) u2 = 0;
      int64_t zz = 12 * 65536 - 3 * u2 - 20 * v2;
      if (zz < 0) zz = 0;
      const int64_t xs = rdiv64(Y * u2 * ct.vn, v2 * ct.un), zs = rdiv64(Y * zz * ct.vn, v2 * ct.wz);
      X = (int)(xs > 2 * CS_Q ? 2 * CS_Q : xs);
      Z = (int)(zs > 2 * CS_Q ? 2 * CS_Q : zs);
    }
  }
  const int r = (ct.minv[0] * X + ct.minv[1] * Y + ct.minv[2] * Z + 2048) >> 12;
  const int g = (ct.minv[3] * X + ct.minv[4] * Y + ct.minv[5] * Z + 2048) >> 12;
  const int b = (ct.minv[6] * X + ct.minv[7] * Y + ct.minv[8] * Z + 2048) >> 12;
  return Rgb{ct.s8[clampi(r, 0, CS_Q)], ct.s8[clampi(g, 0, CS_Q)], ct.s8[clampi(b, 0, CS_Q)]};
}

struct Brightness {          // in place on the three planes of a pixel (C = 3), or sat_u8(v + add) on one (C = 1)
  uint8_t* p; int HW, C, add, space; const mlhot_colour_tabs* ct;
  MLHOT_HD void operator()(int i) const {
    if (C == 1) { p[i] = (uint8_t)sat8(p[i] + add); return; }
    const Rgb in{p[i], p[HW + i], p[2 * HW + i]};
    Rgb o;
    switch (space) {
      case MLHOT_CS_YCRCB: o = bright_ycc(in, add, false); break;
      case MLHOT_CS_YUV: o = bright_ycc(in, add, true); break;
      case MLHOT_CS_HSV: o = bright_hsv(in, add); break;
      case MLHOT_CS_HLS: o = bright_hls(in, add); break;
      default: o = bright_lab_luv(in, add, space == MLHOT_CS_LUV, *ct);
    }
    p[i] = (uint8_t)o.r; p[HW + i] = (uint8_t)o.g; p[2 * HW + i] = (uint8_t)o.b;
  }
};

// ---- the per-image op list ---------------------------------------------------------------------------------------------------------
template <class Exec>
MLHOT_DEV void augment_image_planes(const Exec& ex, const mlhot_aug_record_img& ri, const uint8_t* luts, int n_luts,
                                    const mlhot_colour_tabs* ct, int H, int W, int C, PlaneSets& pl) {
  const mlhot_aug_record& r = ri.base;
  const int HW = H * W, CHW = C * HW;
  const int n_steps = clampi(r.n_steps, 0, 7);
  for (int s = 0; s < n_steps; ++s) {
    const int op = r.op[s];
    if (op < 0 || op > MLHOT_AUG_BRIGHTNESS || !((r.on >> op) & 1)) continue;
    uint8_t* const cur = pl.cur;
    uint8_t* const nxt = pl.nxt;
    if (op == MLHOT_AUG_CROP_PAD) {
      PadGeom g{H, W, clampi(r.pad[0], 0, MAXPAD), clampi(r.pad[1], 0, MAXPAD), clampi(r.pad[2], 0, MAXPAD), clampi(r.pad[3], 0, MAXPAD), 0, 0};
      if ((g.pt | g.pr | g.pb | g.pl) == 0) continue;
      g.Wp = W + g.pl + g.pr; g.Hp = H + g.pt + g.pb;
      const int mode = clampi(r.pad_mode, 0, 9), cval = r.pad_cval & 255, PP = g.Hp * g.Wp;
      const bool stats = mode >= MLHOT_PAD_MAXIMUM && mode <= MLHOT_PAD_MINIMUM;
      uint8_t* const pad = pl.pad;
      int* const stat = pl.stat;
      int* const flag = pl.flag;
      int* const coef = pl.coef;
      ex(CHW + W + H, CopyInPlanesCoef{cur, pad, g, CubicCoef{coef, W, H, g.Wp, g.Hp}, HW, CHW});
      for (int axis = 0; axis < 2; ++axis) {
        const int lines = axis == 0 ? W : g.Hp, area = axis == 0 ? (g.pt + g.pb) * W : (g.pl + g.pr) * g.Hp;
        if (stats) ex(C * lines, per_plane(lines, [=](int c) { return PadStats{pad + c * PP, g, axis, mode, stat + c * MAXP}; }));
        if (mode == MLHOT_PAD_LINEAR_RAMP) {
          ex(2 * C, per_plane(2, [=](int c) { return RampFlags{pad + c * PP, g, axis, cval, flag + 2 + 2 * c}; }));
          ex(2, OrFlags{flag, C});
        }
        ex(C * area, per_plane(area, [=](int c) { return PadFill{pad + c * PP, g, axis, mode, cval, stat + c * MAXP, flag}; }));
      }
      ex(CHW, per_plane(HW, [=](int c) { return CubicResize{pad + c * PP, nxt + c * HW, coef, W, H, g.Wp, g.Hp}; }));
    } else if (op == MLHOT_AUG_GAMMA) {
      if (n_luts <= 0) continue;
      ex(CHW, Gamma{cur, luts + 256 * clampi(r.lut, 0, n_luts - 1)});       // one table for every channel
      continue;
    } else if (op == MLHOT_AUG_BLUR) {
      const int k = clampi(r.blur_k, 1, 3);
      if (k == 1) continue;
      ex(CHW, per_plane(HW, [=](int c) { return BoxBlur{cur + c * HW, nxt + c * HW, W, H, k}; }));
    } else if (op == MLHOT_AUG_AFFINE) {
      const int order = r.aff_order & 1, mode = clampi(r.aff_mode, 0, 4), cval = r.aff_cval & 255;
      const int ax = r.aff_ax, bx = r.aff_bx, ay = r.aff_ay, by = r.aff_by;
      ex(CHW, per_plane(HW, [=](int c) { return AffineWarp{cur + c * HW, nxt + c * HW, W, H, ax, bx, ay, by, order, mode, cval}; }));
    } else if (op == MLHOT_AUG_DROPOUT) {
      const uint32_t key = image_key(r), thresh = r.drop_thresh;
      if (ri.drop_per_channel) ex(CHW, Dropout{cur, key, thresh});          // item = c * H * W + pixel: the planar index itself
      else ex(CHW, per_plane(HW, [=](int c) { return Dropout{cur + c * HW, key, thresh}; }));
      continue;
    } else if (op == MLHOT_AUG_COARSE_DROPOUT) {
      const uint32_t key = image_key(r), thresh = r.coarse_thresh;
      const int ch = clampi(r.coarse_h, 1, MAXD), cw = clampi(r.coarse_w, 1, MAXD), step = ri.coarse_per_channel ? ch * cw : 0;
      ex(CHW, per_plane(HW, [=](int c) { return CoarseDropout{cur + c * HW, key, thresh, W, H, ch, cw, c * step}; }));
      continue;
    } else {
      const int space = clampi(ri.bright_space, 0, 5);
      if (C == 3 && (space == MLHOT_CS_LAB || space == MLHOT_CS_LUV) && ct == nullptr) continue;
      ex(HW, Brightness{cur, HW, C, clampi(ri.bright_add, -255, 255), space, ct});
      continue;
    }
    pl.cur = nxt; pl.nxt = cur;                                             // spatial ops wrote the other plane set
  }
}

MLHOT_HD uint8_t pre_byte(uint8_t b, int pre_op) { return pre_op ? (uint8_t)(256 - b) : b; }

// ---- where the kernel's de-interleave stage reads an image's bytes from: a functor that fills the planar set [C][H][W] ------------------
struct NhwcSrc {             // packed channel-last images of C channels (mlhot_augment_ingest_u8_img)
  const uint8_t* src; int C, pre_op;
#ifndef MLHOT_HOSTSIM
  __device__ __forceinline__ void fill_block(uint8_t* planes, long img, int HW, int vec) const {
    const int CHW = C * HW;
    const uint8_t* s = src + img * CHW;
    if (vec) {                                                          // CHW % 4 == 0, src 4-byte aligned: one dword per lane step
      for (int q = threadIdx.x; q < CHW / 4; q += NT) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(s)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * q + j, p = e / C, c = e - p * C;
          planes[c * HW + p] = pre_byte((uint8_t)(w >> (8 * j)), pre_op);
        }
      }
    } else {
      for (int e = threadIdx.x; e < CHW; e += NT) { const int p = e / C, c = e - p * C; planes[c * HW + p] = pre_byte(s[e], pre_op); }
    }
  }
#endif
  void fill_loop(uint8_t* planes, long img, int HW) const {
    const int CHW = C * HW;
    const uint8_t* sp = src + img * CHW;
    for (int e = 0; e < CHW; ++e) { const int p = e / C, c = e - p * C; planes[c * HW + p] = pre_byte(sp[e], pre_op); }
  }
};

struct PoolSrc {             // image ids[img] of the resident RGBA pool, composed over the bank (pool_ingest.h): C = 3
  const uint8_t* pool; const int* ids; const uint8_t* bank; const int* bg;
#ifndef MLHOT_HOSTSIM
  __device__ __forceinline__ void fill_block(uint8_t* planes, long img, int HW, int vec) const {
    const int b = bg[img];
    const uint8_t* px = pool + (long)ids[img] * HW * 4;
    const uint8_t* bk = b >= 0 ? bank + (long)b * HW * 3 : px;
    for (int p = threadIdx.x; p < HW; p += NT) {
      if (vec) {                                                        // pool 4-byte aligned: a pixel is one dword
        const uint32_t w = reinterpret_cast<const uint32_t*>(px)[p];
        const bool sel = b >= 0 && (w >> 24) == 255u;
#pragma unroll
        for (int c = 0; c < 3; ++c) planes[c * HW + p] = sel ? bk[3 * p + c] : (uint8_t)(w >> (8 * c));
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) planes[c * HW + p] = pool::composed_byte(px + 4 * p, bk + 3 * p, b, c);
      }
    }
  }
#endif
  void fill_loop(uint8_t* planes, long img, int HW) const {
    const int b = bg[img];
    const uint8_t* px = pool + (long)ids[img] * HW * 4;
    const uint8_t* bk = b >= 0 ? bank + (long)b * HW * 3 : px;
    for (int p = 0; p < HW; ++p)
      for (int c = 0; c < 3; ++c) planes[c * HW + p] = pool::composed_byte(px + 4 * p, bk + 3 * p, b, c);
  }
};

struct GreyPoolImgSrc {      // image ids[img] of the resident grey pool: C = 1, pre_byte as NhwcSrc applies it
  const uint8_t* pool; const int* ids; int pre_op;
#ifndef MLHOT_HOSTSIM
  __device__ __forceinline__ void fill_block(uint8_t* planes, long img, int HW, int vec) const {
    const uint8_t* s = pool + (long)ids[img] * HW;
    if (vec) {                                                          // HW % 4 == 0, pool 4-byte aligned: one dword per lane step
      for (int q = threadIdx.x; q < HW / 4; q += NT) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(s)[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) planes[4 * q + j] = pre_byte((uint8_t)(w >> (8 * j)), pre_op);
      }
    } else {
      for (int p = threadIdx.x; p < HW; p += NT) planes[p] = pre_byte(s[p], pre_op);
    }
  }
#endif
  void fill_loop(uint8_t* planes, long img, int HW) const {
    const uint8_t* sp = pool + (long)ids[img] * HW;
    for (int p = 0; p < HW; ++p) planes[p] = pre_byte(sp[p], pre_op);
  }
};

#ifndef MLHOT_HOSTSIM
template <class Src>
__global__ __launch_bounds__(NT) void augment_img_ingest_kernel(const Src src, float* __restrict__ dst, int H, int W, int C,
                                                                float div, float div2,
                                                                const mlhot_aug_record_img* __restrict__ rec,
                                                                const uint8_t* __restrict__ luts, int n_luts,
                                                                const mlhot_colour_tabs* __restrict__ ct, int vec_in, int vec_out) {
  // 16384 + 16384 + 19600 + 1680 + 32 + 5120 = 59200 bytes of the 64 KB static limit
  __shared__ __attribute__((aligned(16))) uint8_t s_a[SET_BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t s_b[SET_BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t s_pad[PAD_BYTES];
  __shared__ int s_stat[MAXC * MAXP], s_flag[2 + 2 * MAXC], s_coef[5 * 2 * MAXD];
  const long img = blockIdx.x;
  const int HW = H * W, CHW = C * HW;
  src.fill_block(s_a, img, HW, vec_in);
  __syncthreads();
  PlaneSets pl{s_a, s_b, s_pad, s_stat, s_flag, s_coef};
  augment_image_planes(BlockExec{}, rec[img], luts, n_luts, ct, H, W, C, pl);
  float* o = dst + img * CHW;
  if (vec_out) {                                                      // CHW % 4 == 0, dst 16-byte aligned: float4 stores
    for (int q = threadIdx.x; q < CHW / 4; q += NT) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(pl.cur)[q];
      float4 v;
      v.x = (float)(uint8_t)(w) / div / div2;
      v.y = (float)(uint8_t)(w >> 8) / div / div2;
      v.z = (float)(uint8_t)(w >> 16) / div / div2;
      v.w = (float)(uint8_t)(w >> 24) / div / div2;
      reinterpret_cast<float4*>(o)[q] = v;
    }
  } else {
    for (int i = threadIdx.x; i < CHW; i += NT) o[i] = (float)pl.cur[i] / div / div2;
  }
}
#endif

inline bool in_scope(int H, int W, int C) {
  return H >= 1 && W >= 1 && ((C == 1 && H <= MAXD && W <= MAXD) || (C == 3 && H <= MAXD3 && W <= MAXD3));
}

// vec_in: may the source read dwords?  vec_out: C * H * W % 4 == 0 and dst 16-byte aligned (float4 stores)
template <class Src>
inline int run_src(const Src& src, int vec_in, int vec_out, float* dst, long n_img, int H, int W, int C, float div, float div2,
                   const mlhot_aug_record_img* rec, const uint8_t* luts, int n_luts, const mlhot_colour_tabs* ct, hipStream_t s,
                   const char* what) {
  if (n_img == 0) return MLHOT_OK;
  const int HW = H * W, CHW = C * HW;
#ifndef MLHOT_HOSTSIM
  ProfScope ps(what, s);
  hipLaunchKernelGGL(augment_img_ingest_kernel<Src>, dim3((unsigned)n_img), dim3(NT), 0, s, src, dst, H, W, C, div, div2, rec, luts,
                     n_luts, ct, vec_in, vec_out);
  return check_launch(what);
#else
  (void)s; (void)vec_in; (void)vec_out; (void)what;
  static thread_local uint8_t a[SET_BYTES], b[SET_BYTES], pad[PAD_BYTES];
  static thread_local int stat[MAXC * MAXP], flag[2 + 2 * MAXC], coef[5 * 2 * MAXD];
  for (long img = 0; img < n_img; ++img) {
    src.fill_loop(a, img, HW);
    PlaneSets pl{a, b, pad, stat, flag, coef};
    augment_image_planes(LoopExec{}, rec[img], luts, n_luts, ct, H, W, C, pl);
    for (int i = 0; i < CHW; ++i) dst[img * CHW + i] = (float)pl.cur[i] / div / div2;
  }
  return MLHOT_OK;
#endif
}

inline int run(const uint8_t* src, float* dst, long n_img, int H, int W, int C, int pre_op, float div, float div2,
               const mlhot_aug_record_img* rec, const uint8_t* luts, int n_luts, const mlhot_colour_tabs* ct, hipStream_t s) {
  const int vec = ((C * H * W) & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  return run_src(NhwcSrc{src, C, pre_op}, vec, vec, dst, n_img, H, W, C, div, div2, rec, luts, n_luts, ct, s, "augment.ingest.u8.img");
}

inline int run_pool(const uint8_t* pool, const int* ids, const uint8_t* bank, const int* bg, float* dst, long n_img, int H, int W,
                    float div, const mlhot_aug_record_img* rec, const uint8_t* luts, int n_luts, const mlhot_colour_tabs* ct,
                    hipStream_t s) {
  const int vec_in = (reinterpret_cast<uintptr_t>(pool) & 3) == 0;
  const int vec_out = ((3 * H * W) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  return run_src(PoolSrc{pool, ids, bank, bg}, vec_in, vec_out, dst, n_img, H, W, 3, div, 1.0f, rec, luts, n_luts, ct, s, "pool.augment.ingest.u8.img");
}

inline int run_pool1(const uint8_t* pool, const int* ids, float* dst, long n_img, int H, int W, int pre_op, float div, float div2,
                     const mlhot_aug_record_img* rec, const uint8_t* luts, int n_luts, const mlhot_colour_tabs* ct, hipStream_t s) {
  const int vec_in = ((H * W) & 3) == 0 && (reinterpret_cast<uintptr_t>(pool) & 3) == 0;
  const int vec_out = ((H * W) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  return run_src(GreyPoolImgSrc{pool, ids, pre_op}, vec_in, vec_out, dst, n_img, H, W, 1, div, div2, rec, luts, n_luts, ct, s,
                 "pool1.augment.ingest.u8.img");
}

}  // namespace augimg
}  // namespace mlhot
