"""The resident image pool's spec restated in numpy and plain Python integers, independently of mlhot/augment.py and
csrc/pool_ingest.h: the per-pixel select, the reference's float formula it stands for, and the background hash."""
import numpy as np

M32 = 0xFFFFFFFF
BG_TAG = 0x62673364


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def bg_index(seed, epoch, image_id, n_bank):
    k = fmix32((seed + 0x9E3779B9) & M32)
    for word in (BG_TAG, epoch, image_id):
        k = fmix32(k ^ (word & M32))
    return (k * n_bank) >> 32


def bg_indices(seed, epoch, ids, n_bank, source="train"):
    ids = np.asarray(ids)
    if source != "train" or epoch == 0:
        return np.full(ids.shape, -1, dtype=np.int32)
    return np.array([bg_index(seed, epoch, int(i), n_bank) for i in ids.ravel()], dtype=np.int32).reshape(ids.shape)


def compose(pool, bank, ids, bg):
    """uint8 [n, H, W, 3]: bank[bg] where bg >= 0 and the pool's alpha byte is 255, the pool's RGB elsewhere."""
    out = []
    for i, b in zip(np.asarray(ids).ravel(), np.asarray(bg).ravel()):
        px = pool[i]
        out.append(px[..., :3] if b < 0 else np.where((px[..., 3] == 255)[..., None], bank[b], px[..., :3]))
    return np.stack(out).astype(np.uint8)


def to_float(img, div=255.0):
    """fp32 [n, 3, H, W] = byte / div: the loaders' `astype(float32) / 255.0` and the permute."""
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(div)).transpose(0, 3, 1, 2))


def reference_formula(images_f32, bank_f32, ids, bg):
    """dataset/shapenet_3d.py:235-239 on float arrays, per output image: rgb * mask + bg * (1 - mask), mask = alpha < 1.0."""
    out = []
    for i, b in zip(np.asarray(ids).ravel(), np.asarray(bg).ravel()):
        item = images_f32[i].copy()
        if b >= 0:
            mask = (item[..., 3] < 1.0)[..., None]
            item[..., :3] = item[..., :3] * mask + bank_f32[b] * (1 - mask)
        out.append(item[..., :3])
    return np.stack(out)
