"""Batch ingest: host uint8 channel-last images -> device fp32 channel-first tensors.

The reference's loaders convert on the host (dataset/shapenet_1d.py:189-196: `astype(float32) / 255.0`, then
utils/utils.py:26-30 permute) and the trainer copies pageable fp32 tensors with `.to(device)`
(trainer/model_trainer.py:67-70): 31.5 MB per 16-task ShapeNet1D batch, more than twice the GPU step time on PCIe.
Here a batch crosses the bus as uint8 (7.9 MB) from pinned staging on a copy stream while the previous step computes,
and `mlhot_ingest_u8_nhwc` does the divide + permute on the device (bit-identical to the host arithmetic).

    ing = BatchIngest(device)
    ing.stage(xs_u8, xq_u8, ys, yq)          # host arrays of batch k+1: returns at once (async H2D)
    ... run step k ...
    ctx_x, qry_x, ctx_y, qry_y = ing.take()   # fp32 [T,N,C,H,W] on the device, ordered on the current stream

`take()` writes into the same device tensors for every batch of the same shape, so a captured hipGraph of the step keeps
reading valid addresses.  There is no CPU fallback: the device must be a ROCm GPU.

`stage(..., augment=table)` (mlhot.augment.Sampler.batch): the batch's augmentation records and gamma LUTs ride in the same pinned
slot and the same H2D copy, and take() expands it with mlhot_augment_ingest_u8 (csrc/augment.h) instead of mlhot_ingest_u8_nhwc.
An mlhot.augment.ImageAugTable (ImageSampler.batch: the image tasks, C = 3 or 1) travels the same way and is expanded with
mlhot_augment_ingest_u8_img (csrc/augment_img.h) with the table's pre_op / div / div2.

`BatchIngest(device, pool=ResidentPool(images_rgba, bank, device))` + `stage_ids(ctx_ids, qry_ids, ys, yq, bg=..., augment=...)`: the
loader's RGBA pool and background bank live on the device, a batch is its image ids (+ one bank index per image), and take() gathers,
composes and converts with mlhot_pool_ingest_u8 / mlhot_pool_augment_ingest_u8_img (csrc/pool_ingest.h).

`ResidentPool(images_grey, device=...)` with a single-channel pool uint8 [N, H, W, 1] (shapenet_1d, pascal_1d, distractor: the bytes the
loader's `get_batch_u8` would carry) serves the same `stage_ids` - no bank, no bg; `augment` an AugTable (the 1D sequences) or an
ImageAugTable (Distractor's) - through mlhot_pool1_ingest_u8 / mlhot_pool1_augment_ingest_u8 / mlhot_pool1_augment_ingest_u8_img
(DESIGN.md 6a-4): what take() delivers is, bit for bit, what stage() delivers for the byte batch pool[ids].
"""
import collections
import threading

import numpy as np
import torch

from . import lib
from .binding import AUG_IMG_RECORD_BYTES, AUG_RECORD_BYTES, MlhotError


def _host(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.contiguous()
    if t.dtype != dtype:
        raise MlhotError(f"BatchIngest: expected {dtype}, got {t.dtype}")
    return t


def _layout(key):
    """Byte layout of one packed staging buffer: [ctx images | qry images | pad to 16 | ctx labels | qry labels]."""
    n_img = [int(np.prod(key[0])), int(np.prod(key[1]))]
    n_lab = [int(np.prod(key[2])), int(np.prod(key[3]))]
    lab_off = (n_img[0] + n_img[1] + 15) // 16 * 16
    return n_img, n_lab, lab_off, lab_off + 4 * (n_lab[0] + n_lab[1])


def _aug_layout(key, total):
    """Behind the labels of an augmented slot: [records int32 [n, 32] (image tasks: [n, 40]) | gamma LUTs uint8 [<= n, 256]], n = images
    of both sides."""
    n = _n_images(key)
    rec_off = (total + 15) // 16 * 16
    lut_off = rec_off + _record_bytes(key) * n
    return n, rec_off, lut_off, lut_off + 256 * n


def _record_bytes(key):
    return AUG_IMG_RECORD_BYTES if key[4] == "augimg" else AUG_RECORD_BYTES


def _n_images(key):
    return int(np.prod(key[0][:-3])) + int(np.prod(key[1][:-3]))


class _Slot:
    """One staging slot: ONE pinned host buffer + its device twin holding a whole batch (images as bytes, labels as fp32, and for an
    augmented batch - key + ("aug",), or ("augimg",) for an ImageAugTable - its records and LUTs), so a batch is one H2D copy."""

    def __init__(self, key, device):
        n_img, n_lab, lab_off, total = _layout(key)
        lab_end = total
        self.augmented = len(key) > 4
        if self.augmented:
            n_aug, rec_off, lut_off, total = _aug_layout(key, total)
        self.host = torch.empty(max(total, 16), dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(max(total, 16), dtype=torch.uint8, device=device)
        hn = self.host.numpy()
        self.host_np = [hn[:n_img[0]].reshape(key[0]), hn[n_img[0]:n_img[0] + n_img[1]].reshape(key[1]),
                        hn[lab_off:lab_off + 4 * n_lab[0]].view(np.float32).reshape(key[2]),
                        hn[lab_off + 4 * n_lab[0]:lab_end].view(np.float32).reshape(key[3])]
        self.dev_img = self.dev[:n_img[0] + n_img[1]]
        self.dev_lab = self.dev[lab_off:lab_end].view(torch.float32)
        self.n_bytes = None                    # bytes to copy: None = the whole buffer
        if self.augmented:
            self.aug_rec_np = hn[rec_off:lut_off].view(np.int32).reshape(n_aug, _record_bytes(key) // 4)
            self.image_table = None            # an ImageAugTable's (pre_op, div, div2), set per batch
            self.aug_lut_np = hn[lut_off:total].reshape(n_aug, 256)
            self.dev_rec = self.dev[rec_off:lut_off].view(torch.int32)
            self.dev_lut = self.dev[lut_off:total].view(n_aug, 256)
            self.lut_off, self.n_luts = lut_off, 0
        self.copied = torch.cuda.Event()       # H2D of this slot finished (host buffer reusable, device buffer readable)
        self.consumed = torch.cuda.Event()     # the kernels that read this slot's device buffer finished
        self.busy = False


def check_pool_indices(ids, bg, n_pool, n_bank):
    """The range check of a batch described by ids, on the HOST arrays, before anything is shipped: the kernels trust them."""
    ids, bg = np.asarray(ids), np.asarray(bg)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n_pool):
        raise MlhotError(f"resident pool: image id out of range [0, {n_pool}): min {int(ids.min())}, max {int(ids.max())}")
    if bg.shape != ids.shape:
        raise MlhotError(f"resident pool: {bg.shape} bg indices for {ids.shape} ids")
    if bg.size and (int(bg.min()) < -1 or int(bg.max()) >= n_bank):
        raise MlhotError(f"resident pool: bg index out of range [-1, {n_bank}): min {int(bg.min())}, max {int(bg.max())}")


def pool_bytes(a, channels, what, L=None, div=255.0):
    """A loader's image pool as contiguous uint8 [n, H, W, channels]: uint8 as it is; fp32 (the reference holds k / 255 floats) through
    mlhot_host_f32_to_u8_exact, refused unless EVERY element is exactly k / div."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.contiguous()
    if t.dim() != 4 or t.shape[-1] != channels or t.device.type != "cpu":
        raise MlhotError(f"ResidentPool: {what} must be a host array [n, H, W, {channels}] (channel-last), got {tuple(t.shape)}")
    if t.dtype == torch.uint8:
        return t
    if t.dtype != torch.float32:
        raise MlhotError(f"ResidentPool: {what} must be uint8 or float32, got {t.dtype}")
    out = torch.empty(t.shape, dtype=torch.uint8)
    bad = (L or lib()).host_f32_to_u8_exact(t.data_ptr(), out.data_ptr(), t.numel(), div, threads=default_feed_threads())
    if bad:
        raise MlhotError(f"ResidentPool: {bad} of {t.numel()} elements of {what} are not exactly k / {div:g} for a byte k - the pool "
                         "cannot be held as bytes")
    return out


def check_grey_batch(n_img, bg, augment):
    """What a batch of a GREY pool may carry, checked before a slot is taken: no bg (there is no bank on this route), and as `augment`
    None, an AugTable (the 1D sequences: 128-byte records) or an ImageAugTable (Distractor's sequence with its pre_op / div / div2:
    160-byte records) of one record per image.  -> the slot kind."""
    from .augment import AugTable, ImageAugTable
    if bg is not None:
        raise MlhotError("BatchIngest.stage_ids: a grey pool has no background bank - bg must be None")
    if augment is None:
        return "pool1"
    if not isinstance(augment, AugTable):
        raise MlhotError(f"BatchIngest.stage_ids: on a grey pool augment is None, an AugTable (shapenet_1d / pascal_1d) or an ImageAugTable "
                         f"(distractor), got {type(augment).__name__}")
    image = isinstance(augment, ImageAugTable)
    ints = (AUG_IMG_RECORD_BYTES if image else AUG_RECORD_BYTES) // 4
    if augment.records.ndim != 2 or augment.records.shape[1] != ints:
        raise MlhotError(f"BatchIngest.stage_ids: {type(augment).__name__} records must be int32 [n, {ints}], got {augment.records.shape}")
    if augment.n_img != n_img:
        raise MlhotError(f"BatchIngest.stage_ids: the augmentation table holds {augment.n_img} records for {n_img} images")
    return "pool1augimg" if image else "pool1aug"


class ResidentPool:
    """A loader's image pool, uploaded ONCE: batches are then described by image ids (BatchIngest.stage_ids) and gathered and converted
    on the device (csrc/pool_ingest.h).  The kind is read from the last dimension: uint8 [N, H, W, 4] is an RGBA pool with its
    background bank (uint8 [B, H, W, 3], or None), uint8 [N, H, W, 1] a grey pool, which has no bank (`grey`; 6a-4)."""

    def __init__(self, images_u8, bank_u8=None, device="cuda:0", div=255.0):
        self.device = torch.device(device)
        shape = tuple(images_u8.shape)
        self.grey = len(shape) == 4 and shape[-1] == 1
        if self.grey and bank_u8 is not None and len(bank_u8) > 0:
            raise MlhotError("ResidentPool: a grey pool [N, H, W, 1] has no alpha to compose behind - it takes no background bank")
        if self.device.type != "cuda":
            raise MlhotError("ResidentPool: the pool lives on a ROCm device; there is no CPU fallback")
        pool = pool_bytes(images_u8, 1 if self.grey else 4, "the image pool", div=div)
        bank = None if self.grey or bank_u8 is None or len(bank_u8) == 0 else pool_bytes(bank_u8, 3, "the background bank", div=div)
        if bank is not None and tuple(bank.shape[1:3]) != tuple(pool.shape[1:3]):
            raise MlhotError(f"ResidentPool: backgrounds of {tuple(bank.shape[1:3])} behind images of {tuple(pool.shape[1:3])}")
        try:
            self.pool = pool.to(self.device)
            self.bank = None if bank is None else bank.to(self.device)
        except RuntimeError as e:              # torch.OutOfMemoryError is one
            need = pool.numel() + (0 if bank is None else bank.numel())
            raise MlhotError(f"ResidentPool: cannot hold {need / 2 ** 20:.0f} MiB of images on {self.device} ({e}); leave "
                             "config.resident_pool off - batches then cross PCIe as bytes") from e
        self.n_pool, self.H, self.W = pool.shape[0], pool.shape[1], pool.shape[2]
        self.n_bank = 0 if bank is None else bank.shape[0]


class _IdSlot:
    """A staging slot of a batch described by ids: [ids int32 (ctx, qry) | bg int32 | pad to 16 | ctx labels | qry labels] and, when the
    batch is augmented, [records int32 [n, 40] | gamma LUTs] behind them - no image bytes.  key = (ctx ids shape, qry ids shape, ctx
    labels shape, qry labels shape, kind): "pool" | "poolaug" for an RGBA pool; "pool1" | "pool1aug" | "pool1augimg" for a grey pool,
    which has no bg array and whose record area follows the table kind - [n, 32] (AugTable) or [n, 40] (ImageAugTable)."""

    def __init__(self, key, device):
        n = int(np.prod(key[0])) + int(np.prod(key[1]))
        n_lab = [int(np.prod(key[2])), int(np.prod(key[3]))]
        grey = key[4].startswith("pool1")
        lab_off = ((4 if grey else 8) * n + 15) // 16 * 16
        lab_end = total = lab_off + 4 * (n_lab[0] + n_lab[1])
        self.augmented = key[4] in ("poolaug", "pool1aug", "pool1augimg")
        rec_bytes = AUG_RECORD_BYTES if key[4] == "pool1aug" else AUG_IMG_RECORD_BYTES
        if self.augmented:
            rec_off = (total + 15) // 16 * 16
            lut_off = rec_off + rec_bytes * n
            total = lut_off + 256 * n
        self.host = torch.empty(max(total, 16), dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(max(total, 16), dtype=torch.uint8, device=device)
        hn = self.host.numpy()
        self.n_img = n
        self.ids_np, self.bg_np = hn[:4 * n].view(np.int32), None if grey else hn[4 * n:8 * n].view(np.int32)
        self.lab_np = [hn[lab_off:lab_off + 4 * n_lab[0]].view(np.float32).reshape(key[2]),
                       hn[lab_off + 4 * n_lab[0]:lab_end].view(np.float32).reshape(key[3])]
        self.dev_ids, self.dev_bg = self.dev[:4 * n].view(torch.int32), None if grey else self.dev[4 * n:8 * n].view(torch.int32)
        self.dev_lab = self.dev[lab_off:lab_end].view(torch.float32)
        self.n_bytes = lab_end                 # bytes to copy: ids (+ bg) + labels (+ records + the LUTs in use)
        self.image_table = None                # an ImageAugTable's (pre_op, div, div2), set per batch
        if self.augmented:
            self.aug_rec_np = hn[rec_off:lut_off].view(np.int32).reshape(n, rec_bytes // 4)
            self.aug_lut_np = hn[lut_off:total].reshape(n, 256)
            self.dev_rec = self.dev[rec_off:lut_off].view(torch.int32)
            self.dev_lut = self.dev[lut_off:total].view(n, 256)
            self.lut_off, self.n_luts = lut_off, 0
        self.copied = torch.cuda.Event()
        self.consumed = torch.cuda.Event()
        self.busy = False


class _Out:
    """The fixed fp32 tensors batches of one shape are delivered in: images of both sets in one flat buffer (one ingest
    launch when the image geometry is shared), labels in another (one device copy)."""

    def __init__(self, key, device):
        (T, Nc, H, W, Cc), (_, Nq, H2, W2, C2) = key[0], key[1]
        n_img, n_lab, _, _ = _layout(key)
        self.same_geometry = (H, W, Cc) == (H2, W2, C2)
        self.img = torch.empty(n_img[0] + n_img[1], device=device)
        self.lab = torch.empty(n_lab[0] + n_lab[1], device=device)
        self.n_img = n_img
        self.tensors = (self.img[:n_img[0]].view(T, Nc, Cc, H, W), self.img[n_img[0]:].view(T, Nq, C2, H2, W2),
                        self.lab[:n_lab[0]].view(key[2]), self.lab[n_lab[0]:].view(key[3]))


class BatchIngest:
    def __init__(self, device, slots=2, div=255.0, pool=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise MlhotError("BatchIngest: the ingest path needs a ROCm device; there is no CPU fallback")
        self.device, self.n_slots, self.div = device, slots, div
        if pool is not None and pool.device != device:
            raise MlhotError(f"BatchIngest: the resident pool lives on {pool.device}, the ingest on {device}")
        self.pool = pool                        # a ResidentPool: stage_ids() describes batches by image ids
        self.copy_stream = torch.cuda.Stream(device)
        self._slots = {}                        # shapes -> [slot, ...]
        self._out = {}                          # shapes -> _Out (fixed fp32 outputs)
        self._queue = collections.deque()
        # stage*() may run on a worker thread while the owner take()s an earlier batch (trainer._HostPrefetch, two batches drawn ahead):
        # slot choice and the queue are guarded; the fill and the copy of a reserved slot are not (they touch only that slot).
        self._lock = threading.Lock()

    def _free_slot(self, key, make=_Slot):
        with self._lock:
            ring = self._slots.setdefault(key, [])
            slot = next((sl for sl in ring if not sl.busy), None)
            if slot is None:
                if len(ring) >= self.n_slots:
                    raise MlhotError("BatchIngest: more batches staged than slots; call take() first")
                slot = make(key, self.device)
                ring.append(slot)
            slot.busy = True                    # reserved from here on (given back by take(), or by a fill that refuses the batch)
        slot.copied.synchronize()               # the previous H2D out of this pinned buffer is done (no-op when fresh)
        return slot

    def stage(self, xs_u8, xq_u8, ys, yq, augment=None):
        """Queue one host batch: images uint8 [T,N,H,W,C] (channel-last), labels fp32 [T,N,L].  Returns a ticket.  `augment`: an
        mlhot.augment.AugTable for the context images then the targets (C = 1), or None."""
        src = [_host(xs_u8, torch.uint8), _host(xq_u8, torch.uint8), _host(ys, torch.float32), _host(yq, torch.float32)]
        if src[0].dim() != 5 or src[1].dim() != 5:
            raise MlhotError("BatchIngest: images must be [T, N, H, W, C]")
        key = tuple(tuple(t.shape) for t in src)
        slot = self._free_slot(self._slot_key(key, augment))
        for h, t in zip(slot.host_np, src):
            np.copyto(h, t.numpy())             # one thread on purpose: torch's copy_ wakes the whole OpenMP pool, whose
                                                # spinning workers then starve the HIP runtime's helper threads
        if augment is not None:
            self._put_augment(slot, augment)
        return self._ship(key, slot)

    def stage_ids(self, ctx_ids, qry_ids, ys, yq, bg=None, augment=None):
        """Queue one batch of the resident pool: image ids [T, Nc] / [T, Nq] (any integer type), labels fp32 [T, N, L]; `bg`: one bank
        index (or -1) per id, context ids first then targets - (ctx [T, Nc], qry [T, Nq]) or one flat array - None = no composition;
        `augment`: an mlhot.augment.ImageAugTable of the shapenet_3d sequence, or None.  Ids and bg indices are range-checked here, on
        the host; ids, bg, labels and records ride in one pinned slot and one H2D copy - no image bytes.  Returns a ticket.
        On a grey pool (ResidentPool.grey): `bg` must be None; `augment` is None, an AugTable (the 1D sequences) or an ImageAugTable
        carrying Distractor's (pre_op, div, div2) - check_grey_batch."""
        pool = self.pool
        if pool is None:
            raise MlhotError("BatchIngest.stage_ids: no resident pool (BatchIngest(device, pool=ResidentPool(...)))")
        ci, qi = np.asarray(ctx_ids), np.asarray(qry_ids)
        if ci.ndim != 2 or qi.ndim != 2 or ci.shape[0] != qi.shape[0] or ci.dtype.kind not in "iu" or qi.dtype.kind not in "iu":
            raise MlhotError(f"BatchIngest.stage_ids: integer ids [T, Nc] and [T, Nq], got {ci.shape} {ci.dtype} / {qi.shape} {qi.dtype}")
        ids = np.concatenate([ci.reshape(-1), qi.reshape(-1)]).astype(np.int64)
        kind = check_grey_batch(ids.size, bg, augment) if pool.grey else None
        if bg is None:
            bgs = np.full(ids.shape, -1, dtype=np.int64)
        else:
            parts = bg if isinstance(bg, (tuple, list)) else (bg,)
            bgs = np.concatenate([np.asarray(b).reshape(-1) for b in parts]).astype(np.int64)
        check_pool_indices(ids, bgs, pool.n_pool, pool.n_bank)
        lab = [_host(ys, torch.float32), _host(yq, torch.float32)]
        if augment is not None and not pool.grey:
            from .augment import ImageAugTable
            if not isinstance(augment, ImageAugTable) or (augment.pre_op, augment.div2) != (0, 1.0):
                raise MlhotError("BatchIngest.stage_ids: augment must be an ImageAugTable of the shapenet_3d sequence (pre_op 0, one division)")
            if augment.n_img != ids.size:
                raise MlhotError(f"BatchIngest.stage_ids: the augmentation table holds {augment.n_img} records for {ids.size} images")
        T, H, W = ci.shape[0], pool.H, pool.W
        if kind is None:
            kind = "pool" if augment is None else "poolaug"
        slot = self._free_slot((tuple(ci.shape), tuple(qi.shape), tuple(lab[0].shape), tuple(lab[1].shape), kind), make=_IdSlot)
        np.copyto(slot.ids_np, ids, casting="unsafe")
        if slot.bg_np is not None:
            np.copyto(slot.bg_np, bgs, casting="unsafe")
        for h, t in zip(slot.lab_np, lab):
            np.copyto(h, t.numpy())
        if augment is not None:
            self._put_augment(slot, augment)
        # delivered in the tensors a byte batch of the same shape is delivered in
        Cc = 1 if pool.grey else 3
        return self._ship(((T, ci.shape[1], H, W, Cc), (T, qi.shape[1], H, W, Cc), tuple(lab[0].shape), tuple(lab[1].shape)), slot)

    @staticmethod
    def _slot_key(key, augment):
        if augment is None:
            return key
        from .augment import ImageAugTable
        image = isinstance(augment, ImageAugTable)
        if not image and (key[0][-1] != 1 or key[1][-1] != 1):
            raise MlhotError(f"BatchIngest: device augmentation needs single-channel images, got {key[0]} / {key[1]}")
        if augment.n_img != _n_images(key):
            raise MlhotError(f"BatchIngest: the augmentation table holds {augment.n_img} records for {_n_images(key)} images")
        return key + ("augimg" if image else "aug",)

    @staticmethod
    def _put_augment(slot, augment):
        np.copyto(slot.aug_rec_np, augment.records)
        k = augment.luts.shape[0]
        if k:
            np.copyto(slot.aug_lut_np[:k], augment.luts)
        slot.n_luts = k
        if slot.aug_rec_np.shape[1] * 4 == AUG_IMG_RECORD_BYTES:
            slot.image_table = (augment.pre_op, augment.div, augment.div2)
        slot.n_bytes = slot.lut_off + 256 * k   # the copy stops behind the LUTs in use

    def stage_filled(self, key, fill, augment=None):
        """Queue a batch whose bytes the CALLER writes into the pinned staging buffers: `fill(host_np)` gets the slot's four numpy views
        ([ctx images u8 | qry images u8 | ctx labels f32 | qry labels f32], shaped like `key`) and returns True to ship the batch or
        False to give the slot back (nothing is queued; returns None).  `augment` as in stage()."""
        slot = self._free_slot(self._slot_key(key, augment))
        try:
            ok = fill(slot.host_np)
            if ok and augment is not None:
                self._put_augment(slot, augment)
        except BaseException:
            slot.busy = False
            raise
        if not ok:
            slot.busy = False
            return None
        return self._ship(key, slot)

    def _ship(self, key, slot):
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(slot.consumed)      # do not overwrite bytes an ingest kernel still reads
            if slot.n_bytes is None:
                slot.dev.copy_(slot.host, non_blocking=True)
            else:
                slot.dev[:slot.n_bytes].copy_(slot.host[:slot.n_bytes], non_blocking=True)
            slot.copied.record(self.copy_stream)
        with self._lock:
            self._queue.append((key, slot))
        return slot

    def device_views(self, ticket=None):
        """(uint8 [n, H, W, C] staged images on the device, fp32 [n, C, H, W] destination) of a staged batch whose two
        image sets share their geometry - what take() hands to mlhot_ingest_u8_nhwc; for profiling that kernel alone."""
        key, slot = self._queue[0] if ticket is None else next(e for e in self._queue if e[1] is ticket)
        out = self._out.setdefault(key, _Out(key, self.device))
        if not out.same_geometry:
            raise MlhotError("device_views: context and target images differ in geometry")
        _, _, H, W, Cc = key[0]
        return slot.dev_img.view(-1, H, W, Cc), out.img.view(-1, Cc, H, W)

    def take(self, ticket=None):
        """A staged batch (the oldest, or the one `ticket` names) as (ctx_x, qry_x, ctx_y, qry_y): fp32, channel-first,
        valid on the current stream.  Batches of one shape share their output tensors: use a batch before taking the next."""
        with self._lock:
            if not self._queue:
                raise MlhotError("BatchIngest.take() without a staged batch")
            if ticket is None:
                key, slot = self._queue.popleft()
            else:
                hit = [e for e in self._queue if e[1] is ticket]
                if not hit:
                    raise MlhotError("BatchIngest.take(): unknown or already taken ticket")
                key, slot = hit[0]
                self._queue.remove(hit[0])
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(slot.copied)
        out = self._out.get(key)
        if out is None:
            out = self._out[key] = _Out(key, self.device)
        L = lib()
        with torch.cuda.device(self.device):
            if isinstance(slot, _IdSlot):
                self._pool_into(L, slot, out)
            elif slot.augmented:
                self._augment_into(L, key, slot, out)
            elif out.same_geometry:             # both image sets are one packed run of (H, W, C) images
                _, _, H, W, Cc = key[0]
                L.ingest_u8_nhwc(slot.dev_img.view(-1, H, W, Cc), out=out.img.view(-1, Cc, H, W), div=self.div)
            else:
                n0 = out.n_img[0]
                L.ingest_u8_nhwc(slot.dev_img[:n0].view(key[0]), out=out.tensors[0], div=self.div)
                L.ingest_u8_nhwc(slot.dev_img[n0:].view(key[1]), out=out.tensors[1], div=self.div)
            out.lab.copy_(slot.dev_lab)
        slot.consumed.record(cur)
        slot.busy = False
        return out.tensors

    def _pool_into(self, L, slot, out):
        pool = self.pool
        if pool.grey:
            dst = out.img.view(slot.n_img, 1, pool.H, pool.W)
            luts = slot.dev_lut[:slot.n_luts] if slot.augmented and slot.n_luts else None
            if not slot.augmented:
                L.pool1_ingest_u8(pool.pool, slot.dev_ids, out=dst, div=self.div)
            elif slot.image_table is None:      # an AugTable: the 1D sequences, the byte route's division
                L.pool1_augment_ingest_u8(pool.pool, slot.dev_ids, slot.dev_rec, luts, out=dst, div=self.div)
            else:
                from .augment import colour_tables
                pre_op, div, div2 = slot.image_table
                L.pool1_augment_ingest_u8_img(pool.pool, slot.dev_ids, slot.dev_rec, luts, colour_tables(self.device), out=dst,
                                              pre_op=pre_op, div=div, div2=div2)
            return
        dst = out.img.view(slot.n_img, 3, pool.H, pool.W)
        if not slot.augmented:
            L.pool_ingest_u8(pool.pool, slot.dev_ids, pool.bank, slot.dev_bg, out=dst, div=self.div)
            return
        from .augment import colour_tables
        L.pool_augment_ingest_u8_img(pool.pool, slot.dev_ids, slot.dev_rec, pool.bank, slot.dev_bg, slot.dev_lut[:slot.n_luts] if slot.n_luts else None,
                                     colour_tables(self.device), out=dst, div=slot.image_table[1])

    def _augment_into(self, L, key, slot, out):
        luts = slot.dev_lut[:slot.n_luts] if slot.n_luts else None
        if slot.image_table is not None:
            from .augment import colour_tables
            pre_op, div, div2 = slot.image_table
            kw = dict(colour_tabs=colour_tables(self.device), pre_op=pre_op, div=div, div2=div2)
            if out.same_geometry:
                _, _, H, W, Cc = key[0]
                L.augment_ingest_u8_img(slot.dev_img.view(-1, H, W, Cc), slot.dev_rec, luts, out=out.img.view(-1, Cc, H, W), **kw)
            else:
                n0, r0 = out.n_img[0], int(np.prod(key[0][:-3])) * (AUG_IMG_RECORD_BYTES // 4)
                L.augment_ingest_u8_img(slot.dev_img[:n0].view(key[0]), slot.dev_rec[:r0], luts, out=out.tensors[0], **kw)
                L.augment_ingest_u8_img(slot.dev_img[n0:].view(key[1]), slot.dev_rec[r0:], luts, out=out.tensors[1], **kw)
            return
        if out.same_geometry:
            _, _, H, W, Cc = key[0]
            L.augment_ingest_u8(slot.dev_img.view(-1, H, W, Cc), slot.dev_rec, luts, out=out.img.view(-1, Cc, H, W), div=self.div)
        else:
            n0, r0 = out.n_img[0], int(np.prod(key[0][:-3]))
            L.augment_ingest_u8(slot.dev_img[:n0].view(key[0]), slot.dev_rec[:r0 * 32], luts, out=out.tensors[0], div=self.div)
            L.augment_ingest_u8(slot.dev_img[n0:].view(key[1]), slot.dev_rec[r0 * 32:], luts, out=out.tensors[1], div=self.div)


class ExactU8Feed:
    """fp32 host batches of a reference-style loader (dataset/shapenet_1d.py:189-196 -> utils/utils.py:26-30: `img.astype(float32) /
    255.0`, channel-first) across PCIe as BYTES when - and only when - every image element is exactly k / 255 for a byte k
    (mlhot_host_f32_to_u8_exact checks all of them while it converts; K native host threads, one pass): a quarter of the traffic, and the ingest
    kernel's `(float)k / 255` on the device gives the loader's fp32 values back bit for bit.  A batch with ANY other value (an
    augmentation that blends pixels, a loader that normalises differently) is refused - stage() returns None and the caller ships the
    fp32 tensors as before; after `give_up` refusals in a row the check is not attempted any more.

        feed = ExactU8Feed(device)
        ticket = feed.stage((ctx_x, qry_x, ctx_y, qry_y))     # fp32 host tensors [T, N, C, H, W] / [T, N, L]; None = not byte images
        ctx_x, qry_x, ctx_y, qry_y = feed.take(ticket)        # fp32 device tensors (fixed addresses per batch shape)
    """

    def __init__(self, device, threads=None, div=255.0, give_up=3, slots=3):
        self.ing = BatchIngest(device, slots=slots, div=div)      # the trainer passes its own count: trainer.model_trainer._HostPrefetch (batches drawn ahead + one on the spot)
        self.div, self.give_up = float(div), int(give_up)
        self.threads = default_feed_threads() if threads is None else max(1, min(64, int(threads)))
        self.ok, self.refused_in_a_row = True, 0
        self.shipped, self.refused = 0, 0

    def stage(self, host_batch, augment=None):
        """`augment`: an mlhot.augment.AugTable for the batch's images (single-channel), or None; an augmented batch is always checked
        (its caller has no other route for it)."""
        if not self.ok and augment is None:
            return None
        xs, xq, ys, yq = host_batch
        for t in (xs, xq, ys, yq):
            if not (torch.is_tensor(t) and t.device.type == "cpu" and t.dtype == torch.float32 and t.is_contiguous()):
                return self._refuse()
        if xs.dim() != 5 or xq.dim() != 5:
            return self._refuse()
        # channel-first bytes are ingested as one-channel images: [T, N * C, H, W, 1] -> [T, N * C, 1, H, W] = the fp32 layout itself
        (T, Nc, C, H, W), (_, Nq, C2, H2, W2) = xs.shape, xq.shape
        key = ((T, Nc * C, H, W, 1), (T, Nq * C2, H2, W2, 1), tuple(ys.shape), tuple(yq.shape))
        L = lib()
        from .augment import ImageAugTable
        image = isinstance(augment, ImageAugTable)
        if image:       # the image tasks' ops mix the channels of a pixel: the bytes are staged channel-last, as the kernel reads them
            key = ((T, Nc, H, W, C), (T, Nq, H2, W2, C2), tuple(ys.shape), tuple(yq.shape))

        def fill(host_np):
            for src, dst in ((xs, host_np[0]), (xq, host_np[1])):
                if image:
                    planar = np.empty(tuple(src.shape), dtype=np.uint8)
                    if L.host_f32_to_u8_exact(src.data_ptr(), planar.ctypes.data, src.numel(), self.div, threads=self.threads):
                        return False
                    np.copyto(dst, planar.transpose(0, 1, 3, 4, 2))
                elif L.host_f32_to_u8_exact(src.data_ptr(), dst.ctypes.data, src.numel(), self.div, threads=self.threads):
                    return False
            np.copyto(host_np[2], ys.numpy())
            np.copyto(host_np[3], yq.numpy())
            return True

        slot = self.ing.stage_filled(key, fill, augment=augment)
        if slot is None:
            return self._refuse()
        self.refused_in_a_row = 0
        self.shipped += 1
        return (slot, tuple(xs.shape), tuple(xq.shape))

    def _refuse(self):
        self.refused += 1
        self.refused_in_a_row += 1
        if self.refused_in_a_row >= self.give_up:
            self.ok = False                    # this loader does not hand out byte images: stop paying for the check
        return None

    def take(self, ticket):
        slot, sc, sq = ticket
        cx, qx, cy, qy = self.ing.take(slot)
        return cx.view(sc), qx.view(sq), cy, qy


def default_feed_threads():
    """Host threads of the byte conversion: MLHOT_FEED_THREADS, else min(4, usable cores // (2 x ranks on this node)), at least 1.
    Measured on the GPU box (EPYC 9575F, scripts/dev/u8_feed_probe.py, c3's 7.9 M floats): 1.23 / 0.62 / 0.34 / 0.30 / 0.47 / 0.86 ms on
    1 / 2 / 4 / 8 / 16 / 32 threads (the call starts its threads itself: beyond 8 the starts cost more than the pieces save); stage()
    as the trainer calls it - two image tensors, labels, the H2D issue - 0.43 ms with 4 threads, 0.54 with 8."""
    import os
    try:
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cores = os.cpu_count() or 1
    ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE") or 1))
    env = os.environ.get("MLHOT_FEED_THREADS")
    if env is not None:
        return max(1, min(int(env), max(1, cores // ranks)))
    return max(1, min(4, cores // (2 * ranks)))
