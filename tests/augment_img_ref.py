"""Test oracle of the image tasks' device augmentation: the spec of DESIGN.md 6a-2 / include/mlhot.h (mlhot_aug_record_img) restated
in numpy, one [H, W, C] image and one record (int32[40]) at a time.  Independent of csrc/augment_img.h and of mlhot/augment.py: np.pad
on the whole [H, W, C] array for the pad modes, the single-channel oracle (tests/augment_ref.py) per channel for the shared ops, and
its own colour spaces and tables."""
import numpy as np

from tests import augment_ref as R

CROP_PAD, GAMMA, BLUR, AFFINE, DROPOUT, COARSE_DROPOUT, BRIGHTNESS = range(7)
YCRCB, HSV, HLS, LAB, LUV, YUV = range(6)
SPACES = ["YCrCb", "HSV", "HLS", "Lab", "Luv", "YUV"]
RECORD_INTS = 40
I_ADD, I_SPACE, I_DROP_PC, I_COARSE_PC = 32, 33, 34, 35
Q = 4080
D = 1479000


# ---- loader byte handling ------------------------------------------------------------------------------------------------------
def pre_op(img, op):
    """What `(images * 255).astype(uint8)` leaves of a byte: 0 = the byte, 1 = (256 - b) mod 256."""
    img = np.asarray(img, dtype=np.uint8)
    return img if op == 0 else ((256 - img.astype(np.int64)) % 256).astype(np.uint8)


def to_float(img, div=255.0, div2=1.0):
    """uint8 [..., H, W, C] -> fp32 [..., C, H, W]: two fp32 divisions in that order."""
    x = img.astype(np.float32) / np.float32(div)
    x = (x / np.float32(div2)).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


# ---- colour spaces -----------------------------------------------------------------------------------------------------------------
def _q14(c):
    return int(np.rint(c * 16384.0))


def _sat(v):
    return np.clip(v, 0, 255)


def _ycc(rgb, add, coef):
    """coef: (chroma 1 of B - Y or R - Y, ...) see callers; 14-bit fixed point, rounded at 2^13."""
    r, g, b = rgb
    y = (_q14(0.299) * r + _q14(0.587) * g + _q14(0.114) * b + 8192) >> 14
    (s1, k1), (s2, k2), back = coef
    d = {"r": r - y, "b": b - y}
    c1 = _sat((d[s1] * _q14(k1) + (128 << 14) + 8192) >> 14) - 128
    c2 = _sat((d[s2] * _q14(k2) + (128 << 14) + 8192) >> 14) - 128
    y = _sat(y + add)
    out = []
    for k_1, k_2 in back:                       # per output channel: coefficients of c1, c2
        out.append(_sat(y + ((c1 * _q14(k_1) + c2 * _q14(k_2) + 8192) >> 14)))
    return out


def ycrcb(rgb, add):
    return _ycc(rgb, add, (("r", 0.713), ("b", 0.564), ((1.403, 0.0), (-0.714, -0.344), (0.0, 1.773))))


def yuv(rgb, add):
    return _ycc(rgb, add, (("b", 0.492), ("r", 0.877), ((0.0, 1.140), (-0.395, -0.581), (2.032, 0.0))))


def _hue(r, g, b, mx, d):
    ds = np.maximum(d, 1)
    n = np.where(mx == r, 30 * (g - b), np.where(mx == g, 30 * (b - r) + 60 * d, 30 * (r - g) + 120 * d))
    n = np.where(n < 0, n + 180 * d, n)
    h = (2 * n + d) // (2 * ds)
    return np.where(d == 0, 0, np.where(h >= 180, h - 180, h))


def hsv(rgb, add):
    r, g, b = rgb
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    d = mx - mn
    s = np.where(mx > 0, (510 * d + mx) // (2 * np.maximum(mx, 1)), 0)
    h = _hue(r, g, b, mx, d)
    v = _sat(mx + add)
    i, f = h // 30, h % 30
    p = (2 * v * (255 - s) + 255) // 510
    q = (2 * v * (7650 - s * f) + 7650) // 15300
    t = (2 * v * (7650 - s * (30 - f)) + 7650) // 15300
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    return [np.choose(i, [table[k][c] for k in range(6)]) for c in range(3)]


def hls(rgb, add):
    r, g, b = rgb
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    d, sm = mx - mn, mx + mn
    m = np.where(sm <= 255, sm, 510 - sm)
    s = np.where(d == 0, 0, _sat((510 * d + m) // (2 * np.maximum(m, 1))))
    h = _hue(r, g, b, mx, d)
    l_ = _sat(((sm + 1) >> 1) + add)
    p2 = np.where(l_ <= 127, l_ * (255 + s), 255 * l_ + 255 * s - l_ * s)
    p1 = 510 * l_ - p2

    def chan(hh):
        hh = np.mod(hh, 180)
        n = np.where(hh < 30, 30 * p1 + (p2 - p1) * hh, np.where(hh < 90, 30 * p2, np.where(hh < 120, 30 * p1 + (p2 - p1) * (120 - hh), 30 * p1)))
        return _sat((2 * n + 7650) // 15300)
    return [chan(h + 60), chan(h), chan(h - 60)]


_TABLES = None


def _fix_rows(m):
    """rows x 2^12 rounded; the largest entry of a row takes the remainder, so that the row sums to exactly 2^12"""
    q = np.rint(m * 4096.0).astype(np.int64)
    for row in q:
        row[np.argmax(row)] += 4096 - row.sum()
    return q


def tables():
    """The Lab / Luv tables of the spec, in float64 (own statement; mlhot.augment.colour_tables() must agree)."""
    global _TABLES
    if _TABLES is None:
        v = np.arange(256, dtype=np.float64) / 255.0
        lin = np.rint(Q * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)).astype(np.int64)
        u = np.arange(Q + 1, dtype=np.float64) / Q
        f = np.rint(32768.0 * np.where(u > 216.0 / 24389.0, np.cbrt(u), (24389.0 / 27.0 * u + 16.0) / 116.0)).astype(np.int64)
        s8 = np.rint(255.0 * np.where(u <= 0.0031308, 12.92 * u, 1.055 * u ** (1.0 / 2.4) - 0.055)).astype(np.int64)
        m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
        mn = m / m.sum(axis=1, keepdims=True)
        xn, zn = int(np.rint(4096 * 0.950456)), int(np.rint(4096 * 1.088754))
        w = xn + 15 * 4096 + 3 * zn
        un, vn = (2 * 4 * xn * 65536 + w) // (2 * w), (2 * 9 * 4096 * 65536 + w) // (2 * w)
        _TABLES = dict(lin=lin, f=f, s8=s8, m=_fix_rows(mn), minv=_fix_rows(np.linalg.inv(mn)), xn=xn, zn=zn, un=un, vn=vn,
                       wz=12 * 65536 - 3 * un - 20 * vn)
    return _TABLES


def _rdiv(a, b):
    return (2 * a + b) // (2 * b)


def _lin_of_f(n):
    """exact integer cubes: N / D -> linear light on 0 .. 2 Q (python integers: no overflow to think about)"""
    k = D ** 3 // Q
    out = np.empty(n.shape, dtype=np.int64)
    for idx, v in np.ndenumerate(n):
        v = int(v)
        t = (v ** 3 + k // 2) // k if 29 * v > 6 * D else max(0, (2 * Q * 108 * (29 * v - 4 * D) + 24389 * D) // (2 * 24389 * D))
        out[idx] = min(t, 2 * Q)
    return out


def _lab_luv(rgb, add, luv):
    t = tables()
    lr, lg, lb = (t["lin"][c] for c in rgb)
    x, y, z = (((t["m"][k, 0] * lr + t["m"][k, 1] * lg + t["m"][k, 2] * lb + 2048) >> 12) for k in range(3))
    fx, fy, fz = t["f"][np.clip(x, 0, Q)], t["f"][np.clip(y, 0, Q)], t["f"][np.clip(z, 0, Q)]
    ln = 116 * fy - (16 << 15)
    l8 = _sat((2 * 255 * ln + (100 << 15)) // (200 << 15))
    l_ = _sat(l8 + add)
    ny = 5000 * l_ + 204000
    Y = _lin_of_f(ny)
    if not luv:
        a8 = _sat(128 + ((500 * (fx - fy) + 16384) >> 15))
        b8 = _sat(128 + ((200 * (fy - fz) + 16384) >> 15))
        X, Z = _lin_of_f(ny + 2958 * (a8 - 128)), _lin_of_f(ny - 7395 * (b8 - 128))
    else:
        d = t["xn"] * x + 15 * 4096 * y + 3 * t["zn"] * z
        ds = np.maximum(d, 1)
        up = np.where(d == 0, t["un"], (2 * 4 * t["xn"] * x * 65536 + d) // (2 * ds))
        vp = np.where(d == 0, t["vn"], (2 * 9 * 4096 * y * 65536 + d) // (2 * ds))
        u8 = _sat(97 + _rdiv(255 * 13 * ln * (up - t["un"]), 354 * 2 ** 31))
        v8 = _sat(136 + _rdiv(255 * 13 * ln * (vp - t["vn"]), 262 * 2 ** 31))
        ls = np.maximum(l_, 1)
        u2 = np.maximum(0, t["un"] + _rdiv(354 * 65536 * (u8 - 97), 1300 * ls))
        v2 = np.maximum(1, t["vn"] + _rdiv(262 * 65536 * (v8 - 136), 1300 * ls))
        zz = np.maximum(0, 12 * 65536 - 3 * u2 - 20 * v2)
        X = np.where(l_ == 0, 0, np.minimum(2 * Q, _rdiv(Y * u2 * t["vn"], v2 * t["un"])))
        Z = np.where(l_ == 0, 0, np.minimum(2 * Q, _rdiv(Y * zz * t["vn"], v2 * t["wz"])))
    return [t["s8"][np.clip((t["minv"][k, 0] * X + t["minv"][k, 1] * Y + t["minv"][k, 2] * Z + 2048) >> 12, 0, Q)] for k in range(3)]


def brightness(img, add, space):
    """img uint8 [H, W, C] -> uint8 [H, W, C]: AddToBrightness through `space`'s 8-bit round trip (C = 1: sat(v + add))."""
    x = img.astype(np.int64)
    if img.shape[2] == 1:
        return _sat(x + add).astype(np.uint8)
    rgb = [x[..., 0], x[..., 1], x[..., 2]]
    fn = {YCRCB: ycrcb, YUV: yuv, HSV: hsv, HLS: hls, LAB: lambda p, a: _lab_luv(p, a, False), LUV: lambda p, a: _lab_luv(p, a, True)}[space]
    return np.stack(fn(rgb, int(add)), axis=-1).astype(np.uint8)


# ---- shared ops on [H, W, C] ----------------------------------------------------------------------------------------------------------
def pad(img, top, right, bottom, left, mode, cval):
    name = R.PAD_MODES[mode]
    kw = {"constant_values": cval} if name == "constant" else {"end_values": cval} if name == "linear_ramp" else {}
    return np.pad(img, ((top, bottom), (left, right), (0, 0)), mode=name, **kw)


def _each(img, fn):
    return np.stack([fn(img[..., c]) for c in range(img.shape[2])], axis=-1)


def dropout(img, key, thresh, per_channel):
    H, W, C = img.shape
    if per_channel:
        items = (np.arange(C)[None, None, :] * H * W + np.arange(H * W).reshape(H, W, 1))
    else:
        items = np.broadcast_to(np.arange(H * W).reshape(H, W, 1), (H, W, C))
    return np.where(R.hashes(key, items) < thresh, 0, img).astype(np.uint8)


def coarse_dropout(img, key, thresh, ch, cw, per_channel):
    H, W, C = img.shape
    rows, cols = np.arange(H) * ch // H, np.arange(W) * cw // W
    out = img.copy()
    for c in range(C):
        first = (1 << 30) + (c * ch * cw if per_channel else 0)
        cells = R.hashes(key, first + np.arange(ch * cw)).reshape(ch, cw) < thresh
        out[..., c] = np.where(cells[rows][:, cols], 0, img[..., c])
    return out


def augment(img, rec, luts=None):
    """img uint8 [H, W, C] (after pre_op); rec int32[40] -> uint8 [H, W, C]"""
    rec = np.asarray(rec, dtype=np.int32)
    u = rec.view(np.uint32)
    H, W, C = img.shape
    out = img.copy()
    key = int(R.image_key(int(u[28]), int(u[29]), int(u[30]), int(u[31])))
    for s in range(int(rec[0])):
        op = int(rec[1 + s])
        if not (int(rec[8]) >> op) & 1:
            continue
        if op == CROP_PAD:
            t, r, b, l_ = (int(v) for v in rec[9:13])
            if t or r or b or l_:
                out = _each(pad(out, t, r, b, l_, int(rec[13]), int(rec[14])), lambda p: R.resize_cubic(p, H, W))
        elif op == GAMMA:
            out = luts[int(rec[15])][out]
        elif op == BLUR:
            out = _each(out, lambda p: R.box_blur(p, int(rec[16])))
        elif op == AFFINE:
            out = _each(out, lambda p: R.affine(p, int(rec[20]), int(rec[21]), int(rec[22]), int(rec[23]), int(rec[17]), int(rec[18]), int(rec[19])))
        elif op == DROPOUT:
            out = dropout(out, key, int(u[24]), bool(rec[I_DROP_PC]))
        elif op == COARSE_DROPOUT:
            out = coarse_dropout(out, key, int(u[25]), int(rec[26]), int(rec[27]), bool(rec[I_COARSE_PC]))
        else:
            out = brightness(out, int(rec[I_ADD]), int(rec[I_SPACE]))
    return out


def augment_batch(imgs, records, luts=None, pre=0, div=255.0, div2=1.0):
    """imgs uint8 [n, H, W, C] -> fp32 [n, C, H, W]: pre_op, the records' ops, the two divisions"""
    return to_float(np.stack([augment(pre_op(im, pre), rec, luts) for im, rec in zip(imgs, records)]), div, div2)
