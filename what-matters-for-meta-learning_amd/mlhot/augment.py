"""Device data augmentation ("DA") of the 1D loaders: the host half.

The reference runs an imgaug Sequential per image on the host inside get_batch (dataset/shapenet_1d.py:174-176,
dataset/pascal_1d.py:116-118).  Here the host only DRAWS: `Sampler` fills one parameter record per image (include/mlhot.h
mlhot_aug_record) and the per-image gamma LUTs, vectorised with numpy, and the fused ingest kernel (csrc/augment.h) applies them to
the staged bytes on the device.  The semantics are the spec in DESIGN.md "Device augmentation".

    spec = AugmentSpec.for_task("shapenet_1d")
    sampler = Sampler(spec, seed=config.seed, rank=rank)
    table = sampler.batch(n_ctx_images, n_qry_images, H, W)     # one generate() per side, as the reference calls it
    ingest.stage(xs_u8, xq_u8, ys, yq, augment=table)

The sampler owns a numpy Generator seeded from (seed, rank): it never touches numpy's global generator, whose order of draws
belongs to the reference's loaders.
"""
import numpy as np

CROP_PAD, GAMMA, BLUR, AFFINE, DROPOUT, COARSE_DROPOUT = range(6)
ONEOF = -1                  # a step whose op is drawn per image: DROPOUT or COARSE_DROPOUT
N_PAD_MODES = 10            # np.pad: constant edge linear_ramp maximum mean median minimum reflect symmetric wrap
N_AFFINE_MODES = 5          # constant edge symmetric reflect wrap
RECORD_INTS = 32            # mlhot_aug_record

# int32 field offsets of mlhot_aug_record
F_N_STEPS, F_OP, F_ON, F_PAD, F_PAD_MODE, F_PAD_CVAL, F_LUT, F_BLUR_K = 0, 1, 8, 9, 13, 14, 15, 16
F_AFF_ORDER, F_AFF_MODE, F_AFF_CVAL, F_AFF_AX, F_AFF_BX, F_AFF_AY, F_AFF_BY = 17, 18, 19, 20, 21, 22, 23
F_DROP_THRESH, F_COARSE_THRESH, F_COARSE_H, F_COARSE_W = 24, 25, 26, 27
F_SEED, F_COUNTER, F_SIDE, F_IMAGE = 28, 29, 30, 31


class AugmentSpec:
    """The step list of one loader's Sequential (each step in Sometimes(0.5), random_order=True)."""

    SEQUENCES = {
        "shapenet_1d": (CROP_PAD, AFFINE, ONEOF),                      # dataset/shapenet_1d.py:34-72 AugmenterShapeNet1D
        "pascal_1d": (CROP_PAD, GAMMA, BLUR, AFFINE, ONEOF),           # utils/augment.py:83-122 PascalAugmenter
    }

    def __init__(self, task, steps):
        self.task, self.steps = task, tuple(steps)

    @classmethod
    def for_task(cls, task):
        if task not in cls.SEQUENCES:
            raise NotImplementedError(
                f"device augmentation covers the single-channel sequences {sorted(cls.SEQUENCES)}; task {task!r} uses the base "
                "Augmenter (AddToBrightness, per_channel dropouts): use config.device_augment_images (ImageAugmentSpec, ImageSampler)")
        return cls(task, cls.SEQUENCES[task])


class AugTable:
    """The drawn parameters of one batch: records int32 [n_img, 32] (context images first, then targets) and luts uint8 [n, 256]."""

    def __init__(self, records, luts):
        self.records, self.luts = records, luts

    @property
    def n_img(self):
        return self.records.shape[0]


def gamma_luts(g):
    """GammaContrast's per-image table (utils/augment.py:98), in float64: round(255 * (v / 255) ** g)."""
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.clip(np.rint(255.0 * v[None, :] ** np.asarray(g, dtype=np.float64)[:, None]), 0, 255).astype(np.uint8)


def affine_fixed(sx, sy, tx, ty, H, W):
    """The inverse of imgaug's Affine (scale about the centre (W/2 - 0.5, H/2 - 0.5), then translate by tx * W, ty * H) in 1/65536 px:
    src_x = (ax * x + bx) / 2^16.  Returns int32 arrays ax, bx, ay, by."""
    cx, cy = W / 2.0 - 0.5, H / 2.0 - 0.5
    ax = np.rint(65536.0 / sx)
    bx = np.rint(65536.0 * (cx - (cx + tx * W) / sx))
    ay = np.rint(65536.0 / sy)
    by = np.rint(65536.0 * (cy - (cy + ty * H) / sy))
    return [a.astype(np.int64).astype(np.int32) for a in (ax, bx, ay, by)]


def _thresh(p):
    """Bernoulli(p) as `hash < thresh` over uint32 hashes."""
    return np.minimum(np.floor(np.asarray(p, dtype=np.float64) * 4294967296.0), 4294967295.0).astype(np.uint32)


class Sampler:
    def __init__(self, spec, seed=0, rank=0):
        if not isinstance(spec, AugmentSpec):
            spec = AugmentSpec.for_task(spec)
        self.spec = spec
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(rank)])))
        self.hash_seed = int(np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(rank), 1]).generate_state(1, np.uint32)[0])
        self.counter = 0            # batches drawn so far (a hash input of the dropouts)

    def side(self, n, H, W, side, lut_base=0):
        """One generate() call of the reference: n images of H x W.  -> (records int32 [n, 32], luts uint8 [k, 256])."""
        rng, steps = self.rng, self.spec.steps
        ns = len(steps)
        perm = rng.permutation(ns)                                    # random_order: one order per call
        on = rng.random((n, ns)) < 0.5                                # Sometimes(0.5) per image and step
        coarse = rng.random(n) < 0.5                                  # OneOf: the second member (CoarseDropout) for these
        pad = np.rint(rng.uniform(0.0, 0.05, (n, 4)) * np.array([H, W, H, W], dtype=np.float64)).astype(np.int32)
        pad_mode = rng.integers(0, N_PAD_MODES, n)
        pad_cval = rng.integers(0, 256, n)
        gamma = rng.uniform(0.5, 2.0, n)
        blur_k = rng.integers(1, 4, n)
        scale = rng.uniform(0.8, 1.2, (n, 2))
        trans = rng.uniform(-0.1, 0.1, (n, 2))
        order = rng.integers(0, 2, n)
        mode = rng.integers(0, N_AFFINE_MODES, n)
        aff_cval = rng.integers(0, 256, n)
        drop_p = rng.uniform(0.01, 0.1, n)
        coarse_p = rng.uniform(0.0, 0.05, n)
        size_p = rng.uniform(0.02, 0.25, n)

        rec = np.zeros((n, RECORD_INTS), dtype=np.int32)
        u = rec.view(np.uint32)
        codes = np.array(steps, dtype=np.int32)[perm]
        ops = np.broadcast_to(codes, (n, ns)).copy()
        ops[ops == ONEOF] = np.broadcast_to(np.where(coarse, COARSE_DROPOUT, DROPOUT)[:, None], (n, ns))[ops == ONEOF]
        rec[:, F_N_STEPS] = ns
        rec[:, F_OP:F_OP + ns] = ops
        rec[:, F_ON] = ((on[:, perm].astype(np.int32)) << ops).sum(axis=1)
        rec[:, F_PAD:F_PAD + 4] = pad
        rec[:, F_PAD_MODE], rec[:, F_PAD_CVAL] = pad_mode, pad_cval
        rec[:, F_BLUR_K] = blur_k
        rec[:, F_AFF_ORDER], rec[:, F_AFF_MODE], rec[:, F_AFF_CVAL] = order, mode, aff_cval
        rec[:, F_AFF_AX], rec[:, F_AFF_BX], rec[:, F_AFF_AY], rec[:, F_AFF_BY] = affine_fixed(scale[:, 0], scale[:, 1], trans[:, 0],
                                                                                              trans[:, 1], H, W)
        u[:, F_DROP_THRESH], u[:, F_COARSE_THRESH] = _thresh(drop_p), _thresh(coarse_p)
        rec[:, F_COARSE_H] = np.maximum(3, np.rint(size_p * H)).astype(np.int32)
        rec[:, F_COARSE_W] = np.maximum(3, np.rint(size_p * W)).astype(np.int32)
        u[:, F_SEED], u[:, F_COUNTER], u[:, F_SIDE] = self.hash_seed, self.counter & 0xFFFFFFFF, side
        rec[:, F_IMAGE] = np.arange(n, dtype=np.int32)
        rec[:, F_LUT] = -1
        luts = np.zeros((0, 256), dtype=np.uint8)
        if GAMMA in steps:
            g_on = (rec[:, F_ON] >> GAMMA) & 1 == 1
            rec[g_on, F_LUT] = lut_base + np.arange(int(g_on.sum()), dtype=np.int32)
            luts = gamma_luts(gamma[g_on])
        return rec, luts

    def batch(self, n_ctx, n_qry, H, W):
        """Both sides of one meta-batch (context = side 0, targets = side 1), each its own generate() call."""
        rc, lc = self.side(n_ctx, H, W, 0)
        rq, lq = self.side(n_qry, H, W, 1, lut_base=lc.shape[0])
        self.counter += 1
        return AugTable(np.concatenate([rc, rq]), np.concatenate([lc, lq]))


# ---- the image tasks (shapenet_3d, distractor): DESIGN.md 6a-2, csrc/augment_img.h ---------------------------------------------------
BRIGHTNESS = 6
YCRCB, HSV, HLS, LAB, LUV, YUV = range(6)      # imgaug's six colour spaces of AddToBrightness (MLHOT_CS_*)
IMG_RECORD_INTS = 40                           # mlhot_aug_record_img: the 32 ints of mlhot_aug_record, then
F_BRIGHT_ADD, F_BRIGHT_SPACE, F_DROP_PER_CHANNEL, F_COARSE_PER_CHANNEL = 32, 33, 34, 35
CS_Q = 4080                                    # MLHOT_CS_Q: the linear-light grid of the Lab / Luv tables


class ImageAugmentSpec(AugmentSpec):
    """The step list of an image task's Sequential, and what its loader does to the bytes around generate(): `pre_op` (what
    `(images * 255).astype(uint8)` leaves of a byte), and the divisions behind it (`div`, then `div2`)."""

    SEQUENCES = {
        "shapenet_3d": (CROP_PAD, GAMMA, BRIGHTNESS, BLUR, AFFINE, ONEOF),       # utils/augment.py:22-63 Augmenter
        "distractor": (AFFINE, ONEOF),                                           # dataset/shapenet_distractor.py:54-81
    }
    # shapenet_3d: float32(k) / 255 * 255 truncates back to k; one division (utils/augment.py:69,77).  distractor: uint8 * 255 wraps to
    # (256 - k) mod 256, and shapenet_distractor.py:256 divides generate()'s output by 255 a second time - both reproduced.
    BYTES = {"shapenet_3d": (0, 255.0, 1.0), "distractor": (1, 255.0, 255.0)}

    def __init__(self, task, steps):
        AugmentSpec.__init__(self, task, steps)
        self.pre_op, self.div, self.div2 = self.BYTES[task]

    @classmethod
    def for_task(cls, task):
        if task not in cls.SEQUENCES:
            raise NotImplementedError(f"device augmentation of images covers {sorted(cls.SEQUENCES)}; task {task!r} is "
                                      "config.device_augment's (AugmentSpec) or has no sequence")
        return cls(task, cls.SEQUENCES[task])


class ImageAugTable(AugTable):
    """AugTable with records int32 [n_img, 40] (mlhot_aug_record_img) and the loader's byte handling of its spec."""

    def __init__(self, records, luts, spec):
        AugTable.__init__(self, records, luts)
        self.pre_op, self.div, self.div2 = spec.pre_op, spec.div, spec.div2


class ImageSampler(Sampler):
    """Sampler for the image tasks: the same draws in the same order, then per image AddToBrightness's integer and colour space and
    the two dropouts' per_channel flags (Dropout 0.5, CoarseDropout 0.2)."""

    def __init__(self, spec, seed=0, rank=0):
        if not isinstance(spec, ImageAugmentSpec):
            spec = ImageAugmentSpec.for_task(spec)
        Sampler.__init__(self, spec, seed=seed, rank=rank)

    def side(self, n, H, W, side, lut_base=0):
        base, luts = Sampler.side(self, n, H, W, side, lut_base=lut_base)
        rng = self.rng
        rec = np.zeros((n, IMG_RECORD_INTS), dtype=np.int32)
        rec[:, :RECORD_INTS] = base
        rec[:, F_BRIGHT_ADD] = rng.integers(-30, 31, n)
        rec[:, F_BRIGHT_SPACE] = rng.integers(0, 6, n)
        rec[:, F_DROP_PER_CHANNEL] = rng.random(n) < 0.5
        rec[:, F_COARSE_PER_CHANNEL] = rng.random(n) < 0.2
        return rec, luts

    def batch(self, n_ctx, n_qry, H, W):
        t = Sampler.batch(self, n_ctx, n_qry, H, W)
        return ImageAugTable(t.records, t.luts, self.spec)


def _rows_to_4096(m):
    q = np.rint(m * 4096.0).astype(np.int64)
    for row in q:
        row[np.argmax(row)] += 4096 - row.sum()          # the row sums to exactly 2^12: grey stays grey
    return q


_COLOUR_TABLES = {}


def colour_tables(device=None):
    """The Lab / Luv tables of AddToBrightness (include/mlhot.h mlhot_colour_tabs), built once in float64: a uint8 array of
    sizeof(mlhot_colour_tabs) bytes, or with `device` a tensor of it there (uploaded once per device).  They do not depend on the batch."""
    if "host" not in _COLOUR_TABLES:
        v = np.arange(256, dtype=np.float64) / 255.0
        lin = np.rint(CS_Q * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4))
        u = np.minimum(np.arange(4096, dtype=np.float64), CS_Q) / CS_Q            # entries above Q repeat the last
        f = np.rint(32768.0 * np.where(u > 216.0 / 24389.0, np.cbrt(u), (24389.0 / 27.0 * u + 16.0) / 116.0))
        s8 = np.rint(255.0 * np.where(u <= 0.0031308, 12.92 * u, 1.055 * u ** (1.0 / 2.4) - 0.055))
        m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
        m = m / m.sum(axis=1, keepdims=True)                                      # white-normalised rows
        xn, zn = int(np.rint(4096 * 0.950456)), int(np.rint(4096 * 1.088754))
        w = xn + 15 * 4096 + 3 * zn
        un, vn = (2 * 4 * xn * 65536 + w) // (2 * w), (2 * 9 * 4096 * 65536 + w) // (2 * w)
        head = np.concatenate([_rows_to_4096(m).ravel(), _rows_to_4096(np.linalg.inv(m)).ravel(),
                               [xn, zn, un, vn, 12 * 65536 - 3 * un - 20 * vn, 0]]).astype(np.int32)
        _COLOUR_TABLES["host"] = np.concatenate([head.view(np.uint8), lin.astype(np.uint16).view(np.uint8),
                                                 f.astype(np.uint16).view(np.uint8), s8.astype(np.uint8)])
    if device is None:
        return _COLOUR_TABLES["host"]
    import torch
    key = str(torch.device(device))
    if key not in _COLOUR_TABLES:
        _COLOUR_TABLES[key] = torch.from_numpy(_COLOUR_TABLES["host"]).to(device)
    return _COLOUR_TABLES[key]


# ---- the resident pool's backgrounds (csrc/pool_ingest.h) --------------------------------------------------------------
BG_TAG = 0x62673364            # "bg3d": keeps this hash chain apart from the dropouts' (csrc/augment.h image_key)


def fmix32(h):
    """murmur3's 32-bit finaliser over uint64 arrays holding 32-bit values (csrc/augment.h fmix32)."""
    h = np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


class BackgroundSampler:
    """Which background of the bank stands behind a training image: bg = mulhi32(hash(seed, epoch, id), B) with the finaliser chain
    of the dropouts over (seed, BG_TAG, epoch, id), epoch = it // bg_gen_freq (0 when config.gen_bg is off).  -1 (no composition) at
    epoch 0 - the training images show the file's backgrounds until the first regeneration - and for every other source, whose
    backgrounds the reference's trainer never regenerates.  A pure function of (seed, epoch, id): no rank, no batch position, no
    generator - an image keeps its background for exactly one epoch, as the reference's in-place regeneration gives."""

    def __init__(self, n_bank, seed=0, bg_gen_freq=1, gen_bg=True):
        self.n_bank, self.seed = int(n_bank), int(seed) & 0xFFFFFFFF
        self.bg_gen_freq, self.gen_bg = max(1, int(bg_gen_freq)), bool(gen_bg)

    def epoch(self, it):
        return int(it) // self.bg_gen_freq if self.gen_bg else 0

    def batch(self, ids, epoch, source="train"):
        """int32 bg indices shaped like `ids` (any integer array of pool ids)."""
        ids = np.asarray(ids)
        if source != "train" or epoch <= 0 or self.n_bank <= 0:
            return np.full(ids.shape, -1, dtype=np.int32)
        k = fmix32(np.uint64((self.seed + 0x9E3779B9) & 0xFFFFFFFF))
        k = fmix32(k ^ np.uint64(BG_TAG))
        k = fmix32(k ^ np.uint64(int(epoch) & 0xFFFFFFFF))
        h = fmix32(k ^ (ids.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)))
        return ((h * np.uint64(self.n_bank)) >> np.uint64(32)).astype(np.int32)


GREY_POOL_TASKS = ("shapenet_1d", "pascal_1d", "distractor")        # single-channel loaders: ResidentPool's grey kind


def check_trainer_config_pool(config, data):
    """The resident pool's switch (config.resident_pool; absent = off): is it on?  Refuses - ValueError, with the reason - what the
    route cannot do: another task, a loader without the task's protocol (rgba_pool for shapenet_3d, grey_pool for the
    single-channel tasks), a loader that still augments itself."""
    if not getattr(config, "resident_pool", False):
        return False
    task = getattr(config, "task", None)
    if task in GREY_POOL_TASKS:
        if not (hasattr(data, "grey_pool") and hasattr(data, "get_batch_ids")):
            raise ValueError(f"config.resident_pool: the resident RGBA pool (rgba_pool) serves task 'shapenet_3d' only (its loader composes "
                             f"backgrounds by alpha); task {task!r} has no alpha channel and needs grey_pool('train') -> uint8 [N, H, W, 1] "
                             "(the bytes of get_batch_u8) and get_batch_ids(source, tasks_per_batch, shot) -> (ctx_ids, qry_ids, ys, yq) "
                             "(INTEGRATION.md) - or leave the switch off")
    elif task != "shapenet_3d":
        raise ValueError(f"config.resident_pool serves tasks 'shapenet_3d' (rgba_pool) and {', '.join(GREY_POOL_TASKS)} (grey_pool); task "
                         f"{task!r} has no resident route - leave the switch off")
    elif not (hasattr(data, "rgba_pool") and hasattr(data, "get_batch_ids")):
        raise ValueError("config.resident_pool: the loader lacks the protocol - rgba_pool('train') -> (uint8 [N, H, W, 4], bank) and "
                         "get_batch_ids(source, tasks_per_batch, shot) -> (ctx_ids, qry_ids, ys, yq) (INTEGRATION.md)")
    if getattr(data, "data_aug", False):
        raise ValueError("config.resident_pool: the loader still augments on the host (data.data_aug is True), and batches described by "
                         "ids never pass through it.  Build it with aug=[a for a in config.aug_list if a != 'data_aug'] and set "
                         + ("config.device_augment_images" if task in ("shapenet_3d", "distractor") else "config.device_augment") + " (INTEGRATION.md)")
    return True


def check_trainer_config_images(config, data):
    """The image tasks' switch (config.device_augment_images; absent = off): None when off, else the ImageSampler."""
    if not getattr(config, "device_augment_images", False) or "data_aug" not in (getattr(config, "aug_list", None) or []):
        return None
    spec = ImageAugmentSpec.for_task(getattr(config, "task", None))
    if getattr(data, "data_aug", False):
        raise ValueError("config.device_augment_images: the loader still augments on the host (data.data_aug is True) - the batch would "
                         "be augmented twice.  Build it with aug=[a for a in config.aug_list if a != 'data_aug'] (INTEGRATION.md)")
    from .dist import rank as dist_rank
    return ImageSampler(spec, seed=int(getattr(config, "seed", 0) or 0), rank=dist_rank())


def check_trainer_config(config, data):
    """The trainer's switch (config.device_augment): None when off, else the Sampler.  Refuses what it cannot do."""
    if not getattr(config, "device_augment", False) or "data_aug" not in (getattr(config, "aug_list", None) or []):
        return None
    spec = AugmentSpec.for_task(getattr(config, "task", None))
    if getattr(data, "data_aug", False):
        raise ValueError("config.device_augment: the loader still augments on the host (data.data_aug is True) - the batch would be "
                         "augmented twice.  Build it with aug=[a for a in config.aug_list if a != 'data_aug'] (INTEGRATION.md)")
    from .dist import rank as dist_rank
    return Sampler(spec, seed=int(getattr(config, "seed", 0) or 0), rank=dist_rank())
