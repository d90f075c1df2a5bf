"""Shape-faithful synthetic meta-batches (the datasets are git-LFS pointers in the reference).

Layouts follow dataset/shapenet_1d.py:189-196 / pascal_1d.py get_batch: float32 tensors
ctx_x [T,Nc,C,H,W], qry_x [T,Nq,C,H,W] in [0,1) (the reference divides uint8 by 255),
labels [T,N,L]: shapenet_1d L=3 = [cos a, sin a, a] with a ~ U[0,2pi); pascal_1d L=1 ~ U[0,1)."""
import math

import torch


def get_batch(task, tasks_per_batch, n_ctx, n_qry, seed=1234, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    xs = torch.rand(tasks_per_batch, n_ctx, 1, 128, 128, generator=g)
    xq = torch.rand(tasks_per_batch, n_qry, 1, 128, 128, generator=g)
    if task == "shapenet_1d":
        a_s = torch.rand(tasks_per_batch, n_ctx, 1, generator=g) * 2 * math.pi
        a_q = torch.rand(tasks_per_batch, n_qry, 1, generator=g) * 2 * math.pi
        ys = torch.cat([torch.cos(a_s), torch.sin(a_s), a_s], dim=-1)
        yq = torch.cat([torch.cos(a_q), torch.sin(a_q), a_q], dim=-1)
    elif task == "pascal_1d":
        ys = torch.rand(tasks_per_batch, n_ctx, 1, generator=g)
        yq = torch.rand(tasks_per_batch, n_qry, 1, generator=g)
    else:
        raise ValueError(task)
    return tuple(t.to(device) for t in (xs, xq, ys, yq))


def get_batch_u8(task, tasks_per_batch, n_ctx, n_qry, seed=1234):
    """The same batch shapes as the loaders hold them BEFORE their host-side conversion (dataset/shapenet_1d.py:174-188):
    uint8 channel-last images [T,N,128,128,1] as numpy arrays + the fp32 labels.  Feed to mlhot.ingest.BatchIngest."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(0, 256, (tasks_per_batch, n_ctx, 128, 128, 1), generator=g, dtype=torch.uint8)
    xq = torch.randint(0, 256, (tasks_per_batch, n_qry, 128, 128, 1), generator=g, dtype=torch.uint8)
    _, _, ys, yq = get_batch(task, tasks_per_batch, n_ctx, n_qry, seed=seed)
    return xs.numpy(), xq.numpy(), ys, yq


def host_convert(u8):
    """What the reference's loaders do on the host (shapenet_1d.py:189-190 + utils/utils.py:26-30): the pageable-fp32
    route that `get_batch_u8` + mlhot.ingest.BatchIngest replaces (kept for A/B timing in bench.py)."""
    import numpy as np
    x = torch.from_numpy(np.asarray(u8).astype(np.float32) / 255.0).type(torch.FloatTensor)
    return x.permute(0, 1, 4, 2, 3).contiguous()


def get_batch_3d(tasks_per_batch, n_ctx, n_qry, seed=1234, device="cpu", task_aug=True):
    """ShapeNet3D-shaped meta-batch (BASELINE config c5; dataset/shapenet_3d.py:108-122,218-227): images [T, N, 3, 64, 64] in
    [0, 1) (the alpha channel is dropped by the loader), labels = unit quaternions with q[1] >= 0.  `task_aug`: the loader's
    task augmentation (utils/utils.py:33-58) - per task one random azimuth / elevation offset added to every label of the task
    (context and target alike) through Euler angles; host-side label arithmetic, it does not change any device shape.  The
    image augmentation (imgaug) of the loader is out of scope."""
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    xs = torch.rand(tasks_per_batch, n_ctx, 3, 64, 64, generator=g)
    xq = torch.rand(tasks_per_batch, n_qry, 3, 64, 64, generator=g)

    def quats(n):
        q = torch.nn.functional.normalize(torch.randn(tasks_per_batch, n, 4, generator=g), dim=-1)
        return torch.where(q[..., 1:2] < 0, -q, q)
    ys, yq = quats(n_ctx), quats(n_qry)
    if task_aug:
        from scipy.spatial.transform import Rotation as R
        rng = np.random.RandomState(seed)
        out = []
        for i in range(tasks_per_batch):
            d_az, d_el = rng.randint(-10, 20), rng.randint(-5, 10)
            pair = []
            for q in (ys[i], yq[i]):
                e = R.from_quat(q.numpy().astype(np.float64)).as_euler("ZYX", degrees=True)
                e[:, 0] += d_el
                e[:, 2] -= d_az
                pair.append(torch.from_numpy(R.from_euler("ZYX", e, degrees=True).as_quat().astype(np.float32)))
            out.append(pair)
        ys, yq = torch.stack([p_[0] for p_ in out]), torch.stack([p_[1] for p_ in out])
    return tuple(t.to(device) for t in (xs, xq, ys, yq))


class SyntheticData:
    """Minimal stand-in for dataset.ShapeNet1D / Pascal1D with the reference's `get_batch` contract
    (dataset/shapenet_1d.py:113-196): train batches draw a random context size in [3, shot], validation /
    test batches use `shot` context images; the target count is always `shot`."""

    def __init__(self, task="shapenet_1d", seed=42):
        import numpy as np
        self.task, self.test_counter = task, 0
        self.rng = np.random.RandomState(seed)
        self.val_rng, self.test_rng = np.random.RandomState(seed), np.random.RandomState(seed)
        self._step = 0

    def gen_bg(self, config, data="all"):
        pass

    def get_batch(self, source, tasks_per_batch, shot):
        rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
        n_ctx = int(rng.randint(3, shot + 1)) if source == "train" else shot
        self._step += 1
        return get_batch(self.task, tasks_per_batch, n_ctx, shot, seed=int(rng.randint(0, 2 ** 31 - 1)))

    def get_batch_u8(self, source, tasks_per_batch, shot):
        """`get_batch` before the host-side conversion: (ctx uint8 [T,Nc,H,W,C], qry uint8, ctx labels, qry labels)."""
        rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
        n_ctx = int(rng.randint(3, shot + 1)) if source == "train" else shot
        self._step += 1
        return get_batch_u8(self.task, tasks_per_batch, n_ctx, shot, seed=int(rng.randint(0, 2 ** 31 - 1)))


def shape_images(n, H=128, W=128, seed=0):
    """uint8 [n, H, W] images with visible structure for the augmentation to move: a horizontal gradient background and three
    filled ellipses / rectangles of random size, place and grey level per image (no noise)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    img = np.broadcast_to(x[None] / max(W - 1, 1) * rng.uniform(20, 80, (n, 1, 1)), (n, H, W)).copy()
    for _ in range(3):
        cy, cx = rng.uniform(0.2, 0.8, (2, n, 1, 1)) * np.array([H, W]).reshape(2, 1, 1, 1)
        ry, rx = rng.uniform(0.08, 0.3, (2, n, 1, 1)) * np.array([H, W]).reshape(2, 1, 1, 1)
        level = rng.uniform(90, 255, (n, 1, 1))
        ell = ((y[None] - cy) / ry) ** 2 + ((x[None] - cx) / rx) ** 2 <= 1.0
        box = (np.abs(y[None] - cy) <= ry) & (np.abs(x[None] - cx) <= rx)
        img = np.where(np.where(rng.rand(n, 1, 1) < 0.5, ell, box), level, img)
    return np.rint(img).astype(np.uint8)


class SyntheticShapesF32:
    """A 1D-task loader (shapenet_1d / pascal_1d: one channel) over a fixed pool of structured images (`shape_images`), with the
    reference's `get_batch` contract (fp32 [T, N, 1, H, W] = bytes / 255, the labels of `get_batch`); its fp32 batches take the
    trainer's host-batch route (mlhot.ingest.ExactU8Feed).  It does not augment itself (`data_aug = False`): pair it with config.device_augment."""

    data_aug = False

    def __init__(self, task="shapenet_1d", seed=42, pool=256, H=128, W=128):
        import numpy as np
        self.task, self.test_counter = task, 0
        self.pool = shape_images(pool, H, W, seed=seed)
        self.rng = np.random.RandomState(seed)
        self.val_rng, self.test_rng = np.random.RandomState(seed + 1), np.random.RandomState(seed + 2)

    def gen_bg(self, config, data="all"):
        pass

    def _draw_u8(self, source, tasks_per_batch, shot):
        import numpy as np
        rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
        n_ctx = int(rng.randint(3, shot + 1)) if source == "train" else shot
        idx = rng.randint(0, self.pool.shape[0], (tasks_per_batch, n_ctx + shot))
        imgs = self.pool[idx][..., None]                                       # [T, Nc + Nq, H, W, 1]
        g = torch.Generator().manual_seed(int(rng.randint(0, 2 ** 31 - 1)))
        if self.task == "shapenet_1d":              # [cos a, sin a, a], a ~ U[0, 2 pi), as get_batch's labels
            a = torch.rand(tasks_per_batch, n_ctx + shot, 1, generator=g) * 2 * math.pi
            y = torch.cat([torch.cos(a), torch.sin(a), a], dim=-1)
        else:
            y = torch.rand(tasks_per_batch, n_ctx + shot, 1, generator=g)
        return (np.ascontiguousarray(imgs[:, :n_ctx]), np.ascontiguousarray(imgs[:, n_ctx:]), y[:, :n_ctx].contiguous(),
                y[:, n_ctx:].contiguous())

    def get_batch(self, source, tasks_per_batch, shot):
        xs, xq, ys, yq = self._draw_u8(source, tasks_per_batch, shot)
        return host_convert(xs), host_convert(xq), ys, yq


class SyntheticShapes(SyntheticShapesF32):
    """`SyntheticShapesF32` with `get_batch_u8`: the trainer reads it through mlhot.ingest.BatchIngest."""

    def get_batch_u8(self, source, tasks_per_batch, shot):
        return self._draw_u8(source, tasks_per_batch, shot)


class SyntheticViews:
    """A loader with the EVAL-mode contract of the reference's ShapeNet3D / Distractor loaders (dataset/shapenet_3d.py:171-204,
    shapenet_distractor.py:263-299): a fixed pool of objects x views, `val_rng` / `test_rng` of its own (the evaluator re-seeds them
    before every sweep point), and draws that do not depend on `shot` - per task one object and one permutation of its views; the
    context is the first `shot` views of the permutation, the targets are ALL views in that order.  So the batch at context size k
    is a prefix of the batch at any larger size: the property the evaluator's prefix sweep rests on.
    task "shapenet_3d": uint8 64 x 64 x 3 images, unit-quaternion labels; "distractor": 128 x 128 x 1, labels in [0, 1)^2.
    mode "train" is the loaders' train-mode shape of the same pool - the targets are the `shot` views BEHIND the context, so nothing
    but the context's first views is shared between context sizes (what the prefix sweep has to refuse)."""

    def __init__(self, task="shapenet_3d", seed=42, objects=8, views=30, mode="eval"):
        import numpy as np
        if task not in ("shapenet_3d", "distractor"):
            raise ValueError(task)
        if mode not in ("eval", "train"):
            raise ValueError(mode)
        self.task, self.mode, self.views, self.test_counter = task, mode, views, 0
        H, C = (64, 3) if task == "shapenet_3d" else (128, 1)
        imgs = shape_images(objects * views * C, H, H, seed=seed).reshape(objects, views, C, H, H)
        self.pool = np.ascontiguousarray(imgs.transpose(0, 1, 3, 4, 2))                       # [objects, views, H, W, C]
        g = torch.Generator().manual_seed(seed)
        if task == "shapenet_3d":
            q = torch.nn.functional.normalize(torch.randn(objects, views, 4, generator=g), dim=-1)
            self.labels = torch.where(q[..., 1:2] < 0, -q, q)
        else:
            self.labels = torch.rand(objects, views, 2, generator=g)
        self.rng = np.random.RandomState(seed)
        self.val_rng, self.test_rng = np.random.RandomState(seed + 1), np.random.RandomState(seed + 2)

    def gen_bg(self, config, data="all"):
        pass

    def get_batch_u8(self, source, tasks_per_batch, shot):
        """(ctx uint8 [T, shot, H, W, C], targets uint8 [T, Nq, H, W, C], ctx labels, target labels) as numpy / fp32 tensors."""
        import numpy as np
        rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
        need = shot if self.mode == "eval" else 2 * shot
        if not 1 <= need <= self.views:
            raise ValueError(f"shot {shot} does not fit {self.views} views per object")
        objs = rng.randint(0, self.pool.shape[0], tasks_per_batch)
        perms = np.stack([rng.permutation(self.views) for _ in range(tasks_per_batch)])
        tgt = perms if self.mode == "eval" else perms[:, shot:2 * shot]
        ctx = perms[:, :shot]
        o_np, o_t = objs[:, None], torch.from_numpy(objs)[:, None]
        return (np.ascontiguousarray(self.pool[o_np, ctx]), np.ascontiguousarray(self.pool[o_np, tgt]),
                self.labels[o_t, torch.from_numpy(np.ascontiguousarray(ctx))].contiguous(),
                self.labels[o_t, torch.from_numpy(np.ascontiguousarray(tgt))].contiguous())

    def get_batch(self, source, tasks_per_batch, shot):
        xs, xq, ys, yq = self.get_batch_u8(source, tasks_per_batch, shot)
        return host_convert(xs), host_convert(xq), ys, yq


def colour_images(n, H=64, W=64, seed=0):
    """uint8 [n, H, W, 3] colour test images for the image tasks' augmentation: three independent `shape_images` planes (saturated and
    mixed colours, flat regions and edges), every fourth image grey (R = G = B)."""
    import numpy as np
    img = np.ascontiguousarray(shape_images(3 * n, H, W, seed=seed).reshape(n, 3, H, W).transpose(0, 2, 3, 1))
    img[::4] = img[::4, :, :, :1]
    return img


class SyntheticViewsF32:
    """`SyntheticViews` in its train-mode shape WITHOUT `get_batch_u8`: fp32 [T, N, C, H, W] = bytes / 255 host batches, which take the
    trainer's host-batch route (mlhot.ingest.ExactU8Feed).  Neither augments (`data_aug = False`): pair them with
    config.device_augment_images."""

    data_aug = False

    def __init__(self, task="shapenet_3d", seed=42, objects=8, views=30):
        self._views = SyntheticViews(task, seed=seed, objects=objects, views=views, mode="train")
        self.task, self.test_counter = task, 0

    def gen_bg(self, config, data="all"):
        pass

    def get_batch(self, source, tasks_per_batch, shot):
        return self._views.get_batch(source, tasks_per_batch, shot)


class SyntheticViewsRGBA:
    """The ShapeNet3D loader's TRAIN-mode shape over a pool that still has its alpha channel (dataset/shapenet_3d.py:113, 231-254):
    objects x views RGBA images uint8 [N, 64, 64, 4] - alpha 255 inside the shapes except a sprinkling of 254 right next to it, small
    values elsewhere - and a small background bank uint8 [B, 64, 64, 3].  It speaks the resident pool's protocol (`rgba_pool`,
    `get_batch_ids`: mlhot.ingest.ResidentPool, config.resident_pool) and, for the sources that keep their routes, `get_batch_u8`
    (the file's RGB, no composition).  Draws as SyntheticViews(mode="train"): per task one object, context = the first `shot` views of
    a permutation, targets = the `shot` behind them.  It neither augments nor regenerates (`data_aug = False`, `gen_bg` a no-op)."""

    data_aug = False

    def __init__(self, seed=42, objects=8, views=30, bank=5, H=64, W=64):
        import numpy as np
        self.task, self.views, self.test_counter = "shapenet_3d", views, 0
        n = objects * views
        rgb = colour_images(n, H, W, seed=seed)
        grey = shape_images(n, H, W, seed=seed + 7)                               # shapes at 90 .. 255 over a gradient below 81
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        alpha = np.where(grey >= 90, np.where((x + 2 * y)[None] % 7 == 0, 254, 255), grey).astype(np.uint8)
        self.pool = np.ascontiguousarray(np.concatenate([rgb, alpha[..., None]], axis=-1))       # [N, H, W, 4]
        self.bank = colour_images(bank, H, W, seed=seed + 13)                     # [B, H, W, 3]
        g = torch.Generator().manual_seed(seed)
        q = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
        self.labels = torch.where(q[..., 1:2] < 0, -q, q)
        self.rng = np.random.RandomState(seed)
        self.val_rng, self.test_rng = np.random.RandomState(seed + 1), np.random.RandomState(seed + 2)

    def gen_bg(self, config, data="all"):
        pass

    def rgba_pool(self, source="train"):
        return self.pool, self.bank

    def get_batch_ids(self, source, tasks_per_batch, shot):
        """(ctx ids int32 [T, shot], target ids int32 [T, shot], ctx labels, target labels): ids index rgba_pool()'s images."""
        import numpy as np
        rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
        if not 1 <= 2 * shot <= self.views:
            raise ValueError(f"shot {shot} does not fit {self.views} views per object")
        objs = rng.randint(0, self.pool.shape[0] // self.views, tasks_per_batch)
        perms = np.stack([rng.permutation(self.views) for _ in range(tasks_per_batch)])
        ids = (objs[:, None] * self.views + perms[:, :2 * shot]).astype(np.int32)
        ci, qi = np.ascontiguousarray(ids[:, :shot]), np.ascontiguousarray(ids[:, shot:])
        return ci, qi, self.labels[torch.from_numpy(ci).long()].contiguous(), self.labels[torch.from_numpy(qi).long()].contiguous()

    def get_batch_u8(self, source, tasks_per_batch, shot):
        ci, qi, ys, yq = self.get_batch_ids(source, tasks_per_batch, shot)
        import numpy as np
        return np.ascontiguousarray(self.pool[ci][..., :3]), np.ascontiguousarray(self.pool[qi][..., :3]), ys, yq


class SyntheticViewsRGBAHost:
    """`SyntheticViewsRGBA`'s twin for today's route: the same draws, but the backgrounds are composed on the HOST - the select of
    dataset/shapenet_3d.py:235-239 with the mlhot.augment.BackgroundSampler handed in, at an epoch that every `gen_bg` call advances
    (the trainer calls it every bg_gen_freq iterations) - and the batches are fp32 [T, N, 3, H, W] = bytes / 255 host tensors
    (the trainer's host-batch route).  No `get_batch_u8`, no pool protocol."""

    data_aug = False

    def __init__(self, sampler, **kw):
        self._rgba, self.sampler, self.epoch = SyntheticViewsRGBA(**kw), sampler, 0
        self.task, self.test_counter = "shapenet_3d", 0
        self.val_rng, self.test_rng = self._rgba.val_rng, self._rgba.test_rng

    def gen_bg(self, config, data="all"):
        self.epoch += 1                  # the reference regenerates in place: every training image gets this epoch's background

    def compose(self, ids, source):
        import numpy as np
        px = self._rgba.pool[ids]
        bg = self.sampler.batch(ids, self.epoch, source)
        take = (bg >= 0)[..., None, None] & (px[..., 3] == 255)
        return np.where(take[..., None], self._rgba.bank[np.maximum(bg, 0)], px[..., :3])

    def get_batch(self, source, tasks_per_batch, shot):
        ci, qi, ys, yq = self._rgba.get_batch_ids(source, tasks_per_batch, shot)
        return host_convert(self.compose(ci, source)), host_convert(self.compose(qi, source)), ys, yq


class SyntheticGreyPool:
    """A single-channel loader (task "shapenet_1d", "pascal_1d" or "distractor") over a fixed pool of structured images uint8
    [N, H, W, 1] that speaks BOTH routes of the trainer: the resident grey pool's protocol (`grey_pool`, `get_batch_ids`:
    mlhot.ingest.ResidentPool, config.resident_pool) and the byte route (`get_batch_u8`).  The two are twins: from the same generator
    state `get_batch_u8` returns grey_pool()[ids] for the ids - and the labels - `get_batch_ids` returns.  Draws as the 1D loaders: a
    training batch has a random context size in [3, shot], every image of a task is drawn from the whole pool; the labels belong to the
    images (shapenet_1d: [cos a, sin a, a]; pascal_1d: one value in [0, 1); distractor: two).  For "distractor" the pool is handed over
    already inverted - 255 - images, the bytes dataset/shapenet_distractor.py:233 ships - and `get_batch_u8` ships the same bytes.
    It does not augment (`data_aug = False`): pair it with config.device_augment (1D) or config.device_augment_images (distractor)."""

    data_aug = False

    def __init__(self, task="shapenet_1d", seed=42, pool=96, H=128, W=128):
        import numpy as np
        if task not in ("shapenet_1d", "pascal_1d", "distractor"):
            raise ValueError(task)
        self.task, self.test_counter = task, 0
        images = shape_images(pool, H, W, seed=seed)[..., None]
        self.pool = np.ascontiguousarray(255 - images if task == "distractor" else images)      # [N, H, W, 1]: what crosses PCIe today
        g = torch.Generator().manual_seed(seed)
        if task == "shapenet_1d":
            a = torch.rand(pool, 1, generator=g) * 2 * math.pi
            self.labels = torch.cat([torch.cos(a), torch.sin(a), a], dim=-1)
        else:
            self.labels = torch.rand(pool, 1 if task == "pascal_1d" else 2, generator=g)
        self.rng = np.random.RandomState(seed)
        self.val_rng, self.test_rng = np.random.RandomState(seed + 1), np.random.RandomState(seed + 2)

    def gen_bg(self, config, data="all"):
        pass

    def grey_pool(self, source="train"):
        return self.pool

    def get_batch_ids(self, source, tasks_per_batch, shot):
        """(ctx ids int32 [T, Nc], target ids int32 [T, shot], ctx labels, target labels): ids index grey_pool()'s images."""
        import numpy as np
        rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
        n_ctx = int(rng.randint(3, shot + 1)) if source == "train" else shot
        ids = rng.randint(0, self.pool.shape[0], (tasks_per_batch, n_ctx + shot)).astype(np.int32)
        ci, qi = np.ascontiguousarray(ids[:, :n_ctx]), np.ascontiguousarray(ids[:, n_ctx:])
        return ci, qi, self.labels[torch.from_numpy(ci).long()].contiguous(), self.labels[torch.from_numpy(qi).long()].contiguous()

    def get_batch_u8(self, source, tasks_per_batch, shot):
        import numpy as np
        ci, qi, ys, yq = self.get_batch_ids(source, tasks_per_batch, shot)
        return np.ascontiguousarray(self.pool[ci]), np.ascontiguousarray(self.pool[qi]), ys, yq

    def get_batch(self, source, tasks_per_batch, shot):
        xs, xq, ys, yq = self.get_batch_u8(source, tasks_per_batch, shot)
        return host_convert(xs), host_convert(xq), ys, yq
