"""Test oracle of the device data augmentation: the spec of DESIGN.md "Device augmentation" restated in numpy, one image and one
parameter record (int32[32], include/mlhot.h mlhot_aug_record) at a time.  Independent of csrc/augment.h: np.pad for the pad modes,
its own fixed-point bicubic, affine remap, box blur and hash."""
import numpy as np

CROP_PAD, GAMMA, BLUR, AFFINE, DROPOUT, COARSE_DROPOUT = range(6)
PAD_MODES = ["constant", "edge", "linear_ramp", "maximum", "mean", "median", "minimum", "reflect", "symmetric", "wrap"]
AFFINE_MODES = ["constant", "edge", "symmetric", "reflect", "wrap"]

M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def image_key(seed, counter, side, image):
    k = fmix32((seed + 0x9E3779B9) & M32)
    for v in (counter, side, image):
        k = fmix32(k ^ np.uint64(v))
    return k


def hashes(key, items):
    items = np.asarray(items, dtype=np.uint64)
    return fmix32(np.uint64(key) ^ ((items * 0x9E3779B1) & M32))


# ---- ops ---------------------------------------------------------------------------------------------------------------------
def pad(img, top, right, bottom, left, mode, cval):
    """imgaug CropAndPad's padding: np.pad of the uint8 image (constant_values / end_values = cval)."""
    name = PAD_MODES[mode]
    kw = {"constant_values": cval} if name == "constant" else {"end_values": cval} if name == "linear_ramp" else {}
    return np.pad(img, ((top, bottom), (left, right)), mode=name, **kw)


def cubic_coeffs(dn, sn):
    """cv2.resize INTER_CUBIC for uint8 along one axis: first tap and four weights in 1/2048 per output index."""
    d = np.arange(dn, dtype=np.float64)
    f = ((d + 0.5) * (float(sn) / float(dn)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    A = np.float32(-0.75)
    one = np.float32(1)
    x1 = f + one
    r = one - f
    w0 = ((A * x1 - np.float32(5) * A) * x1 + np.float32(8) * A) * x1 - np.float32(4) * A
    w1 = (((A + np.float32(2)) * f - (A + np.float32(3))) * f) * f + one
    w2 = (((A + np.float32(2)) * r - (A + np.float32(3))) * r) * r + one
    w3 = one - w0 - w1 - w2
    w = np.stack([w0, w1, w2, w3], axis=1).astype(np.float32)
    return s - 1, np.rint(w * np.float32(2048)).astype(np.int64)


def resize_cubic(img, H, W):
    Hp, Wp = img.shape
    y0, wy = cubic_coeffs(H, Hp)
    x0, wx = cubic_coeffs(W, Wp)
    src = img.astype(np.int64)
    rows = np.clip(y0[:, None] + np.arange(4)[None, :], 0, Hp - 1)            # [H, 4]
    cols = np.clip(x0[:, None] + np.arange(4)[None, :], 0, Wp - 1)            # [W, 4]
    h = (src[:, cols] * wx[None, :, :]).sum(axis=2)                           # [Hp, W]: horizontal sums, exact
    v = (h[rows, :] * wy[:, :, None]).sum(axis=1)                             # [H, W]
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def border(p, n, mode):
    """index of p on a line of n under the cv2 border `mode` (AFFINE_MODES); -1 = the constant"""
    p = np.asarray(p, dtype=np.int64)
    inside = (p >= 0) & (p < n)
    name = AFFINE_MODES[mode]
    if name == "constant":
        out = np.full_like(p, -1)
    elif name == "edge":
        out = np.clip(p, 0, n - 1)
    elif name == "symmetric":
        q = np.mod(p, 2 * n)
        out = np.where(q < n, q, 2 * n - 1 - q) if n > 1 else np.zeros_like(p)
    elif name == "reflect":
        if n == 1:
            out = np.zeros_like(p)
        else:
            q = np.mod(p, 2 * n - 2)
            out = np.where(q < n, q, 2 * n - 2 - q)
    else:
        out = np.mod(p, n)
    return np.where(inside, p, out)


def affine(img, ax, bx, ay, by, order, mode, cval):
    H, W = img.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    X, Y = ax * x + bx, ay * y + by
    src = img.astype(np.int64)

    def tap(yy, xx):
        sy, sx = border(yy, H, mode), border(xx, W, mode)
        ok = (sy >= 0) & (sx >= 0)
        return np.where(ok, src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], cval)

    if order == 0:
        return tap((Y + 32768) >> 16, (X + 32768) >> 16).astype(np.uint8)
    Xq, Yq = (X + 1024) >> 11, (Y + 1024) >> 11
    x0, y0, fx, fy = Xq >> 5, Yq >> 5, Xq & 31, Yq & 31
    v = ((32 - fy) * (32 - fx) * 32 * tap(y0, x0) + (32 - fy) * fx * 32 * tap(y0, x0 + 1)
         + fy * (32 - fx) * 32 * tap(y0 + 1, x0) + fy * fx * 32 * tap(y0 + 1, x0 + 1))
    return np.clip((v + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def round_half_even_div(s, n):
    q, r = np.divmod(s, n)
    return q + ((2 * r > n) | ((2 * r == n) & (q % 2 == 1)))


def box_blur(img, k):
    if k == 1:
        return img.copy()
    H, W = img.shape
    a = k // 2
    ys = border(np.arange(H)[:, None] - a + np.arange(k)[None, :], H, AFFINE_MODES.index("reflect"))   # REFLECT_101
    xs = border(np.arange(W)[:, None] - a + np.arange(k)[None, :], W, AFFINE_MODES.index("reflect"))
    src = img.astype(np.int64)
    s = np.zeros((H, W), dtype=np.int64)
    for i in range(k):
        for j in range(k):
            s += src[ys[:, i]][:, xs[:, j]]
    return round_half_even_div(s, k * k).astype(np.uint8)


def gamma(img, lut):
    return lut[img]


def dropout(img, key, thresh):
    h = hashes(key, np.arange(img.size)).reshape(img.shape)
    return np.where(h < thresh, 0, img).astype(np.uint8)


def coarse_dropout(img, key, thresh, ch, cw):
    H, W = img.shape
    cells = hashes(key, (1 << 30) + np.arange(ch * cw)).reshape(ch, cw) < thresh        # dropped cells
    rows, cols = np.arange(H) * ch // H, np.arange(W) * cw // W
    return np.where(cells[rows][:, cols], 0, img).astype(np.uint8)


# ---- one image, one record --------------------------------------------------------------------------------------------------------
def augment(img, rec, luts=None):
    """img uint8 [H, W]; rec int32[32] -> uint8 [H, W]"""
    rec = np.asarray(rec, dtype=np.int32)
    u = rec.view(np.uint32)
    H, W = img.shape
    out = img.copy()
    key = int(image_key(int(u[28]), int(u[29]), int(u[30]), int(u[31])))
    for s in range(int(rec[0])):
        op = int(rec[1 + s])
        if not (int(rec[8]) >> op) & 1:
            continue
        if op == CROP_PAD:
            t, r, b, l_ = (int(v) for v in rec[9:13])
            if t or r or b or l_:
                out = resize_cubic(pad(out, t, r, b, l_, int(rec[13]), int(rec[14])), H, W)
        elif op == GAMMA:
            out = gamma(out, luts[int(rec[15])])
        elif op == BLUR:
            out = box_blur(out, int(rec[16]))
        elif op == AFFINE:
            out = affine(out, int(rec[20]), int(rec[21]), int(rec[22]), int(rec[23]), int(rec[17]), int(rec[18]), int(rec[19]))
        elif op == DROPOUT:
            out = dropout(out, key, int(u[24]))
        else:
            out = coarse_dropout(out, key, int(u[25]), int(rec[26]), int(rec[27]))
    return out


def augment_batch(imgs, records, luts=None):
    """imgs uint8 [n, H, W] -> uint8 [n, H, W]"""
    return np.stack([augment(im, rec, luts) for im, rec in zip(imgs, records)])
