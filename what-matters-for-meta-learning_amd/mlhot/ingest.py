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

A batch takes one of the eight routes of `ROUTES`, decided once, when it is staged, from where its images come from
and the table that rides with it:

    source \\ augment=     None                an AugTable (1D sequences)     an ImageAugTable (image tasks)
    BYTES  stage()         ingest_u8_nhwc      augment_ingest_u8 (C = 1)      augment_ingest_u8_img
    RGBA   stage_ids()     pool_ingest_u8      -                              pool_augment_ingest_u8_img
    GREY   stage_ids()     pool1_ingest_u8     pool1_augment_ingest_u8        pool1_augment_ingest_u8_img

BYTES: the images themselves are staged.  RGBA / GREY: `BatchIngest(device, pool=ResidentPool(...))` holds the loader's pool on the
device (uint8 [N, H, W, 4] with its background bank, or uint8 [N, H, W, 1]) and a batch is its image ids, for the RGBA pool with one
bank index per image (csrc/pool_ingest.h); what take() delivers is, bit for bit, what the BYTES route
delivers for the byte batch pool[ids].  Whatever the route, the batch - payload, labels, and the table's records and gamma LUTs
(mlhot.augment.Sampler.batch / ImageSampler.batch) - is ONE pinned slot (`slot_layout`) and one H2D copy, and take() expands it with
the route's one library entry (`BatchIngest._expand`).
"""
import collections
import math
import threading
import typing

import numpy as np
import torch

from . import lib
from .augment import AugTable, ImageAugTable, colour_tables
from .binding import AUG_IMG_RECORD_BYTES, AUG_RECORD_BYTES, MlhotError


def _host(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.contiguous()
    if t.dtype != dtype:
        raise MlhotError(f"BatchIngest: expected {dtype}, got {t.dtype}")
    return t


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
BYTES, RGBA, GREY = "packed bytes", "the RGBA pool", "a grey pool"       # where a batch's images come from


class Route(typing.NamedTuple):
    name: str           # the last element of the slot key
    source: str         # BYTES | RGBA | GREY
    table: type         # what rides with the batch: None, AugTable or ImageAugTable
    record_ints: int    # int32s per record of that table: 0, 32 (mlhot_aug_record) or 40 (mlhot_aug_record_img)
    ids: bool           # the payload: int32 image ids (stage_ids) instead of the images' bytes (stage)
    bg: bool            # ... followed by one int32 bank index per id
    channels: int       # channels delivered by an id route (a byte route delivers its images' own)
    entry: str          # the MlhotLib method that expands the slot


_INTS, _IMG_INTS = AUG_RECORD_BYTES // 4, AUG_IMG_RECORD_BYTES // 4
ROUTES = {(r.source, r.table): r for r in (
    Route("u8", BYTES, None, 0, False, False, 0, "ingest_u8_nhwc"),
    Route("aug", BYTES, AugTable, _INTS, False, False, 0, "augment_ingest_u8"),
    Route("augimg", BYTES, ImageAugTable, _IMG_INTS, False, False, 0, "augment_ingest_u8_img"),
    Route("pool", RGBA, None, 0, True, True, 3, "pool_ingest_u8"),
    Route("poolaug", RGBA, ImageAugTable, _IMG_INTS, True, True, 3, "pool_augment_ingest_u8_img"),
    Route("pool1", GREY, None, 0, True, False, 1, "pool1_ingest_u8"),
    Route("pool1aug", GREY, AugTable, _INTS, True, False, 1, "pool1_augment_ingest_u8"),
    Route("pool1augimg", GREY, ImageAugTable, _IMG_INTS, True, False, 1, "pool1_augment_ingest_u8_img"),
)}
_TABLES_OF = {BYTES: "None, an AugTable (single-channel images) or an ImageAugTable",
              RGBA: "None or an ImageAugTable of the shapenet_3d sequence (pre_op 0, one division)",
              GREY: "None, an AugTable (shapenet_1d / pascal_1d) or an ImageAugTable (distractor)"}


def check_table(source, augment, n_img, bg=None, channels=(1, 1)):
    """May `augment` ride on a batch of `n_img` images from `source`?  -> the batch's Route, or MlhotError - before a slot is taken.
    `bg`: what the caller passed as bank indices (only the RGBA pool has a bank); `channels`: of the context and target images of a
    BYTES batch."""
    who = "BatchIngest.stage" if source == BYTES else "BatchIngest.stage_ids"
    if bg is not None and source == GREY:
        raise MlhotError(f"{who}: a grey pool has no background bank - bg must be None")
    table = None if augment is None else next((t for t in (ImageAugTable, AugTable) if isinstance(augment, t)), type(augment))
    route = ROUTES.get((source, table))
    if route is None:
        raise MlhotError(f"{who}: on {source} augment is {_TABLES_OF[source]}, got {type(augment).__name__}")
    if table is None:
        return route
    if source == RGBA and (augment.pre_op, augment.div2) != (0, 1.0):      # its entry composes, augments and divides once
        raise MlhotError(f"{who}: on {source} augment is {_TABLES_OF[source]}, got (pre_op, div2) = {(augment.pre_op, augment.div2)}")
    if augment.records.ndim != 2 or augment.records.shape[1] != route.record_ints:
        raise MlhotError(f"{who}: {table.__name__} records must be int32 [n, {route.record_ints}], got {augment.records.shape}")
    if augment.n_img != n_img:
        raise MlhotError(f"{who}: the augmentation table holds {augment.n_img} records for {n_img} images")
    if source == BYTES and table is AugTable and tuple(channels) != (1, 1):
        raise MlhotError(f"{who}: an AugTable (config.device_augment: the 1D sequences) needs single-channel images, got {channels[0]} / "
                         f"{channels[1]} channels; the image tasks draw an ImageAugTable (config.device_augment_images)")
    return route


def check_grey_batch(n_img, bg, augment):
    """What a batch of a GREY pool may carry (check_table): no bg, and as `augment` None, an AugTable (128-byte records) or an
    ImageAugTable (Distractor's sequence with its pre_op / div / div2: 160-byte records) of one record per image.  -> its Route."""
    return check_table(GREY, augment, n_img, bg=bg)


# ---- one slot ----------------------------------------------------------------------------------------------------------------------------
class Layout(typing.NamedTuple):
    """Byte offsets of one staging buffer: [payload | pad to 16 | ctx labels | qry labels] and, behind a route with a table,
    [pad to 16 | records int32 [n_img, ints] | gamma LUTs uint8 [<= n_img, 256]]."""
    parts: tuple        # where the payload's parts end: (0, ctx images, qry images), or (0, ids int32[, bg int32])
    lab_off: int
    lab_mid: int        # ctx labels | qry labels
    lab_end: int
    rec_off: int
    lut_off: int
    total: int          # the buffer: at least 16 bytes
    n_img: int          # images of both sides = records = LUT rows


def _pad16(n):
    return (n + 15) // 16 * 16


def slot_layout(route, key):
    """The Layout of `route`'s slot for key = (ctx, qry, ctx labels, qry labels) shapes; ctx / qry are the image shapes [T, N, H, W, C]
    of a byte route and the id shapes [T, N] of an id route.  Integers only: no torch, no device."""
    lead = [s if route.ids else s[:-3] for s in key[:2]]
    n_img = math.prod(lead[0]) + math.prod(lead[1])
    if route.ids:
        parts = (0, 4 * n_img, 8 * n_img) if route.bg else (0, 4 * n_img)
    else:
        parts = (0, math.prod(key[0]), math.prod(key[0]) + math.prod(key[1]))
    lab_off = _pad16(parts[-1])
    lab_mid = lab_off + 4 * math.prod(key[2])
    lab_end = lab_mid + 4 * math.prod(key[3])
    rec_off = _pad16(lab_end)
    lut_off = rec_off + 4 * route.record_ints * n_img
    end = lut_off + 256 * n_img if route.record_ints else lab_end
    return Layout(parts, lab_off, lab_mid, lab_end, rec_off, lut_off, max(end, 16), n_img)


class _Slot:
    """One staging slot: ONE pinned host buffer + its device twin holding a whole batch of `route` (slot_layout), so a batch is one
    H2D copy.  The ingest's ring key is key + (route.name,)."""

    def __init__(self, route, key, device):
        lay = slot_layout(route, key)
        self.route, self.layout = route, lay
        self.host = torch.empty(lay.total, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(lay.total, dtype=torch.uint8, device=device)
        hn, p = self.host.numpy(), lay.parts
        # the four views a byte batch is written through (stage_filled's `fill`), or ids[, bg] and the labels
        if route.ids:
            self.host_np = [hn[a:b].view(np.int32) for a, b in zip(p, p[1:])]
            self.dev_ids = self.dev[p[0]:p[1]].view(torch.int32)
            self.dev_bg = self.dev[p[1]:p[2]].view(torch.int32) if route.bg else None
        else:
            self.host_np = [hn[p[0]:p[1]].reshape(key[0]), hn[p[1]:p[2]].reshape(key[1])]
            self.dev_img = self.dev[:p[2]]
        self.host_np += [hn[lay.lab_off:lay.lab_mid].view(np.float32).reshape(key[2]),
                         hn[lay.lab_mid:lay.lab_end].view(np.float32).reshape(key[3])]
        self.dev_lab = self.dev[lay.lab_off:lay.lab_end].view(torch.float32)
        self.n_bytes = lay.lab_end             # bytes to copy: up to the end of the last section in use (_put_augment)
        if route.record_ints:
            self.rec_np = hn[lay.rec_off:lay.lut_off].view(np.int32).reshape(lay.n_img, route.record_ints)
            lut_end = lay.lut_off + 256 * lay.n_img
            self.lut_np = hn[lay.lut_off:lut_end].reshape(lay.n_img, 256)
            self.dev_rec = self.dev[lay.rec_off:lay.lut_off].view(torch.int32).view(lay.n_img, route.record_ints)
            self.dev_lut = self.dev[lay.lut_off:lut_end].view(lay.n_img, 256)
        self.n_luts = 0                        # LUT rows of the staged batch ...
        self.image_table = None                # ... and its ImageAugTable's (pre_op, div, div2)
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


class _Out:
    """The fixed fp32 tensors batches of one shape are delivered in: images of both sets in one flat buffer (one ingest
    launch when the image geometry is shared), labels in another (one device copy)."""

    def __init__(self, key, device):
        (T, Nc, H, W, Cc), (_, Nq, H2, W2, C2) = key[0], key[1]
        n_img, n_lab = [math.prod(key[0]), math.prod(key[1])], [math.prod(key[2]), math.prod(key[3])]
        self.same_geometry = (H, W, Cc) == (H2, W2, C2)
        self.img = torch.empty(n_img[0] + n_img[1], device=device)
        self.lab = torch.empty(n_lab[0] + n_lab[1], device=device)
        self.key, self.n_img = key, n_img
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
        self._slots = {}                        # shapes + (route name,) -> [slot, ...]
        self._out = {}                          # shapes -> _Out (fixed fp32 outputs)
        self._queue = collections.deque()
        # stage*() may run on a worker thread while the owner take()s an earlier batch (trainer._HostPrefetch, two batches drawn ahead):
        # slot choice and the queue are guarded; the fill and the copy of a reserved slot are not (they touch only that slot).
        self._lock = threading.Lock()

    def _free_slot(self, route, key):
        with self._lock:
            ring = self._slots.setdefault(key + (route.name,), [])
            slot = next((sl for sl in ring if not sl.busy), None)
            if slot is None:
                if len(ring) >= self.n_slots:
                    raise MlhotError("BatchIngest: more batches staged than slots; call take() first")
                slot = _Slot(route, key, self.device)
                ring.append(slot)
            slot.busy = True                    # reserved from here on (given back by take(), or by a fill that refuses the batch)
        slot.copied.synchronize()               # the previous H2D out of this pinned buffer is done (no-op when fresh)
        return slot

    def stage(self, xs_u8, xq_u8, ys, yq, augment=None):
        """Queue one host batch: images uint8 [T,N,H,W,C] (channel-last), labels fp32 [T,N,L].  Returns a ticket.  `augment`: an
        mlhot.augment.AugTable (C = 1) or ImageAugTable for the context images then the targets, or None."""
        src = [_host(xs_u8, torch.uint8), _host(xq_u8, torch.uint8), _host(ys, torch.float32), _host(yq, torch.float32)]
        if src[0].dim() != 5 or src[1].dim() != 5:
            raise MlhotError("BatchIngest: images must be [T, N, H, W, C]")

        def fill(host_np):
            for h, t in zip(host_np, src):
                np.copyto(h, t.numpy())         # one thread on purpose: torch's copy_ wakes the whole OpenMP pool, whose
            return True                         # spinning workers then starve the HIP runtime's helper threads
        return self.stage_filled(tuple(tuple(t.shape) for t in src), fill, augment=augment)

    def stage_filled(self, key, fill, augment=None):
        """Queue a batch whose bytes the CALLER writes into the pinned staging buffers: `fill(host_np)` gets the slot's four numpy views
        ([ctx images u8 | qry images u8 | ctx labels f32 | qry labels f32], shaped like `key`) and returns True to ship the batch or
        False to give the slot back (nothing is queued; returns None).  `augment` as in stage()."""
        n_img = math.prod(key[0][:-3]) + math.prod(key[1][:-3])
        slot = self._free_slot(check_table(BYTES, augment, n_img, channels=(key[0][-1], key[1][-1])), key)
        return self._fill_and_ship(key, slot, fill, augment)

    def stage_ids(self, ctx_ids, qry_ids, ys, yq, bg=None, augment=None):
        """Queue one batch of the resident pool: image ids [T, Nc] / [T, Nq] (any integer type), labels fp32 [T, N, L]; `bg`: one bank
        index (or -1) per id, context ids first then targets - (ctx [T, Nc], qry [T, Nq]) or one flat array - None = no composition;
        `augment`: what check_table allows on the pool - on an RGBA pool an mlhot.augment.ImageAugTable of the shapenet_3d sequence;
        on a grey pool (ResidentPool.grey, where `bg` must be None) an AugTable (the 1D sequences) or an ImageAugTable carrying
        Distractor's (pre_op, div, div2) - or None.  Ids and bg indices are range-checked here, on the host; ids, bg, labels and
        records ride in one pinned slot and one H2D copy - no image bytes.  Returns a ticket."""
        pool = self.pool
        if pool is None:
            raise MlhotError("BatchIngest.stage_ids: no resident pool (BatchIngest(device, pool=ResidentPool(...)))")
        ci, qi = np.asarray(ctx_ids), np.asarray(qry_ids)
        if ci.ndim != 2 or qi.ndim != 2 or ci.shape[0] != qi.shape[0] or ci.dtype.kind not in "iu" or qi.dtype.kind not in "iu":
            raise MlhotError(f"BatchIngest.stage_ids: integer ids [T, Nc] and [T, Nq], got {ci.shape} {ci.dtype} / {qi.shape} {qi.dtype}")
        ids = np.concatenate([ci.reshape(-1), qi.reshape(-1)]).astype(np.int64)
        route = check_table(GREY if pool.grey else RGBA, augment, ids.size, bg=bg)
        if bg is None:
            bgs = np.full(ids.shape, -1, dtype=np.int64)
        else:
            parts = bg if isinstance(bg, (tuple, list)) else (bg,)
            bgs = np.concatenate([np.asarray(b).reshape(-1) for b in parts]).astype(np.int64)
        check_pool_indices(ids, bgs, pool.n_pool, pool.n_bank)
        lab = [_host(ys, torch.float32), _host(yq, torch.float32)]
        key = (tuple(ci.shape), tuple(qi.shape), tuple(lab[0].shape), tuple(lab[1].shape))

        def fill(host_np):
            for h, a in zip(host_np, ([ids, bgs] if route.bg else [ids]) + [t.numpy() for t in lab]):
                np.copyto(h, a, casting="unsafe")
            return True
        # delivered in the tensors a byte batch of the same shape is delivered in
        (T, Nc), Nq, geom = ci.shape, qi.shape[1], (pool.H, pool.W, route.channels)
        return self._fill_and_ship(((T, Nc) + geom, (T, Nq) + geom) + key[2:], self._free_slot(route, key), fill, augment)

    def _fill_and_ship(self, out_key, slot, fill, augment):
        """Write a reserved slot - `fill(slot.host_np)`, then the table behind the labels - and start its H2D copy; a fill that
        returns False or raises gives the slot back."""
        try:
            ok = fill(slot.host_np)
            if ok:
                self._put_augment(slot, augment)
        except BaseException:
            slot.busy = False
            raise
        if not ok:
            slot.busy = False
            return None
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(slot.consumed)      # do not overwrite bytes an ingest kernel still reads
            slot.dev[:slot.n_bytes].copy_(slot.host[:slot.n_bytes], non_blocking=True)
            slot.copied.record(self.copy_stream)
        with self._lock:
            self._queue.append((out_key, slot))
        return slot

    @staticmethod
    def _put_augment(slot, augment):
        if augment is None:
            return
        np.copyto(slot.rec_np, augment.records)
        k = augment.luts.shape[0]
        if k:
            np.copyto(slot.lut_np[:k], augment.luts)
        slot.n_luts = k
        if slot.route.table is ImageAugTable:
            slot.image_table = (augment.pre_op, augment.div, augment.div2)
        slot.n_bytes = slot.layout.lut_off + 256 * k        # the copy stops behind the LUTs in use

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
        with torch.cuda.device(self.device):
            self._expand(slot, out)
            out.lab.copy_(slot.dev_lab)
        slot.consumed.record(cur)
        slot.busy = False
        return out.tensors

    def _expand(self, slot, out):
        """The one call into the library: slot -> out.img through the route's entry, its arguments built from the route and the slot."""
        route = slot.route
        entry, kw = getattr(lib(), route.entry), {"div": self.div}
        if route.record_ints:
            kw.update(records=slot.dev_rec, luts=slot.dev_lut[:slot.n_luts] if slot.n_luts else None)
        if route.table is ImageAugTable:
            pre_op, div, div2 = slot.image_table
            kw.update(colour_tabs=colour_tables(self.device), div=div)
            if route.source != RGBA:            # the RGBA pool's entry has neither: check_table admits only (0, 1.0) there
                kw.update(pre_op=pre_op, div2=div2)
        key, n = out.key, slot.layout.n_img
        _, _, H, W, Cc = key[0]
        if route.ids:
            if route.bg:
                kw.update(bank=self.pool.bank, bg=slot.dev_bg)
            entry(self.pool.pool, slot.dev_ids, out=out.img.view(n, Cc, H, W), **kw)
        elif out.same_geometry:                 # both image sets are one packed run of (H, W, C) images
            entry(slot.dev_img.view(n, H, W, Cc), out=out.img.view(n, Cc, H, W), **kw)
        else:                                   # one launch per side, each with its rows of the records and the whole LUT table
            n0, r0 = out.n_img[0], math.prod(key[0][:-3])
            for img, dst, rows in ((slot.dev_img[:n0].view(key[0]), out.tensors[0], slice(0, r0)),
                                   (slot.dev_img[n0:].view(key[1]), out.tensors[1], slice(r0, n))):
                if route.record_ints:
                    kw["records"] = slot.dev_rec[rows]
                entry(img, out=dst, **kw)


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
