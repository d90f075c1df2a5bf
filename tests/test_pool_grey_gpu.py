"""The resident grey pool on the MI355X: the three mlhot_pool1_* entries against the existing references applied to
pool[ids] bit for bit - the vector fast path, the any-size path, offsets past 2^31 bytes - BatchIngest.stage_ids shipping ids instead of
image bytes, and the trainer with config.resident_pool against the same loader on the byte route."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests.test_pool_grey_cpu import (IDS, N_POOL, SHAPES, all_off, grey_pool, run_aug, run_aug_img, run_plain, same_bits, tables, to_float,
                                      want_aug, want_aug_img)

DEV = "cuda:0"


# ---- 1. the plain entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_plain_entry_bit_exact(gpulib, H, W):
    pool = grey_pool(H, W)
    assert same_bits(run_plain(gpulib, pool, IDS, DEV), to_float(pool[IDS]))
    arange = np.arange(N_POOL, dtype=np.int32)                                    # identity ids: the plain ingest of the whole pool
    plain = gpulib.ingest_u8_nhwc(torch.from_numpy(pool).to(DEV)).cpu().numpy()
    assert same_bits(run_plain(gpulib, pool, arange, DEV), plain)


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W", [(37, 16, 16), (137, 16, 16), (480, 128, 128)])
def test_plain_entry_partial_workgroups_and_one_headline_batch(gpulib, n, H, W):
    """A workgroup takes 1024 quads of 4 pixels.  37 x 64 = 2368 quads: three workgroups, the last partly filled; 137 x 64 = 8768:
    nine, the last partly filled; 480 images of 128 x 128: the headline batch (1920 full workgroups), ids drawn with repeats from a
    96-image pool."""
    pool = grey_pool(H, W, n=96)
    ids = np.random.default_rng(n).integers(0, 96, n).astype(np.int32)
    ids[0], ids[-1] = 95, 0
    assert same_bits(run_plain(gpulib, pool, ids, DEV), to_float(pool[ids]))


# ---- 2. unaligned pool and destination ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unaligned_pool_and_destination_take_the_any_size_path(gpulib):
    pool = grey_pool(16, 16)
    want = to_float(pool[IDS])
    ids = torch.from_numpy(IDS).to(DEV)
    buf = torch.zeros(pool.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = torch.from_numpy(pool).to(DEV).view(-1)
    p1 = buf[1:].view(pool.shape)                                                  # the pool one byte into its buffer
    assert p1.data_ptr() % 16 == 1
    assert same_bits(gpulib.pool1_ingest_u8(p1, ids).cpu().numpy(), want)
    obuf = torch.full((want.size + 2,), -1.0, device=DEV)
    o1 = obuf[1:1 + want.size].view(want.shape)                                    # the destination one float into its buffer
    assert o1.data_ptr() % 16 == 4
    gpulib.pool1_ingest_u8(torch.from_numpy(pool).to(DEV), ids, out=o1)
    assert same_bits(o1.cpu().numpy(), want) and obuf[0].item() == -1.0 and obuf[-1].item() == -1.0
    # the augmenting entries on the same views: byte loads and scalar stores
    t1, _, ti = tables(16, 16)
    assert same_bits(gpulib.pool1_augment_ingest_u8(p1, ids, torch.from_numpy(t1.records).to(DEV), torch.from_numpy(t1.luts).to(DEV)).cpu().numpy(),
                     want_aug(pool, IDS, t1))
    gpulib.pool1_augment_ingest_u8_img(p1, ids, torch.from_numpy(ti.records).to(DEV), None, A.colour_tables(DEV), out=o1, pre_op=ti.pre_op,
                                       div=ti.div, div2=ti.div2)
    assert same_bits(o1.cpu().numpy(), want_aug_img(pool, IDS, ti)) and obuf[0].item() == -1.0 and obuf[-1].item() == -1.0


# ---- 3. 64-bit addressing -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_offsets_past_two_gib(gpulib):
    """131 073 images of 128 x 128: image N - 1 starts at byte 2^31 exactly, where ids * HW in 32 bits wraps.  Only the three gathered
    images are written; the rest of the allocation is never read."""
    N, H, W = 131073, 128, 128
    try:
        big = torch.empty((N, H, W, 1), dtype=torch.uint8, device=DEV)
    except RuntimeError as e:                                                      # torch.OutOfMemoryError is one
        pytest.skip(f"cannot allocate a {N * H * W / 2 ** 30:.2f} GiB device pool: {e}")
    small = grey_pool(H, W, n=3, seed=64)
    ids = np.array([N - 1, 0, N // 2], dtype=np.int32)
    for k, i in enumerate(ids):
        big[int(i)] = torch.from_numpy(small[k]).to(DEV)
    assert (N - 1) * H * W == 2 ** 31
    dev_ids = torch.from_numpy(ids).to(DEV)
    assert same_bits(gpulib.pool1_ingest_u8(big, dev_ids).cpu().numpy(), to_float(small))
    local = np.arange(3, dtype=np.int32)
    t1, _, ti = tables(H, W, n_ctx=1, n_qry=2)
    got = gpulib.pool1_augment_ingest_u8(big, dev_ids, torch.from_numpy(t1.records).to(DEV), torch.from_numpy(t1.luts).to(DEV) if len(t1.luts) else None)
    assert same_bits(got.cpu().numpy(), want_aug(small, local, t1))
    got = gpulib.pool1_augment_ingest_u8_img(big, dev_ids, torch.from_numpy(ti.records).to(DEV), None, A.colour_tables(DEV), pre_op=ti.pre_op,
                                             div=ti.div, div2=ti.div2)
    assert same_bits(got.cpu().numpy(), want_aug_img(small, local, ti))
    del big
    torch.cuda.empty_cache()


# ---- 4. the augmenting entries ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(128, 128), (7, 5), (1, 1)])
def test_whole_sequences_bit_exact(gpulib, H, W):
    pool = grey_pool(H, W, n=12)
    ids = np.random.default_rng(H).integers(0, 12, 16).astype(np.int32)            # T = 2, Nc = 3, Nq = 5, ids with repeats
    ids[0], ids[-1] = 11, 0
    t1, tp, ti = tables(H, W, n_ctx=6, n_qry=10)
    plain = run_plain(gpulib, pool, ids, DEV)
    for t in (t1, tp):
        got = run_aug(gpulib, pool, ids, t, DEV)
        assert same_bits(got, want_aug(pool, ids, t))
        assert same_bits(run_aug(gpulib, pool, ids, all_off(t), DEV), plain)       # every step off: the plain entry
        assert H == 1 or not same_bits(got, plain)
    got = run_aug_img(gpulib, pool, ids, ti, DEV)
    assert same_bits(got, want_aug_img(pool, ids, ti))
    off = all_off(ti)
    off.pre_op, off.div2 = 0, 1.0
    assert same_bits(run_aug_img(gpulib, pool, ids, off, DEV), plain)


# ---- 5. stage_ids -------------------------------------------------------------------------------------------------------------------
def _want_batch(pool, ids, t):
    if t is None:
        return to_float(pool[ids])
    return want_aug_img(pool, ids, t) if isinstance(t, A.ImageAugTable) else want_aug(pool, ids, t)


@pytest.mark.gpu
@pytest.mark.parametrize("task,kind", [("shapenet_1d", None), ("shapenet_1d", "aug"), ("pascal_1d", "aug"), ("distractor", "augimg")])
def test_stage_ids_ships_no_image_bytes(gpulib, task, kind):
    from mlhot.binding import AUG_IMG_RECORD_BYTES, AUG_RECORD_BYTES, MlhotError
    from mlhot.ingest import BatchIngest, ResidentPool
    from mlhot.synth import SyntheticGreyPool
    H = W = 128
    data = SyntheticGreyPool(task, seed=4, pool=24, H=H, W=W)
    pool = data.grey_pool("train")
    ing = BatchIngest(DEV, pool=ResidentPool(pool, device=DEV))
    assert ing.pool.grey and ing.pool.n_bank == 0 and ing.pool.n_pool == 24
    sampler = {None: None, "aug": A.Sampler(task, seed=8) if kind == "aug" else None, "augimg": A.ImageSampler("distractor", seed=8)}[kind]
    rec_bytes = {None: 0, "aug": AUG_RECORD_BYTES, "augimg": AUG_IMG_RECORD_BYTES}[kind]
    for _ in range(2):
        ci, qi, ys, yq = data.get_batch_ids("train", 2, 5)
        t = None if sampler is None else sampler.batch(ci.size, qi.size, H, W)
        slot = ing.stage_ids(ci, qi, ys, yq, augment=t)
        n = ci.size + qi.size
        want_bytes = (4 * n + 15) // 16 * 16 + 4 * (ys.numel() + yq.numel())       # ids (padded to 16) + labels ...
        if t is not None:
            want_bytes = (want_bytes + 15) // 16 * 16 + rec_bytes * n + 256 * t.luts.shape[0]        # ... + records + the LUTs in use
        # per image at most 4 (id) + 12 (label) + 160 (record) + 256 (LUT) + padding: under a sixteenth of its 16384 image bytes
        assert slot.n_bytes == want_bytes and want_bytes < n * H * W // 16
        cx, qx, cy, qy = ing.take(slot)
        ids = np.concatenate([ci.reshape(-1), qi.reshape(-1)])
        got = torch.cat([cx.reshape(-1, 1, H, W), qx.reshape(-1, 1, H, W)]).cpu().numpy()
        assert cx.shape == (2, ci.shape[1], 1, H, W) and qx.shape == (2, 5, 1, H, W) and same_bits(got, _want_batch(pool, ids, t))
        assert torch.equal(cy.cpu(), ys) and torch.equal(qy.cpu(), yq)
    # the refusals, none of which ships anything
    ci, qi, ys, yq = data.get_batch_ids("validation", 2, 5)
    t1, ti = A.Sampler("shapenet_1d", seed=1).batch(10, 10, H, W), A.ImageSampler("distractor", seed=1).batch(10, 10, H, W)
    with pytest.raises(MlhotError, match="out of range"):
        ing.stage_ids(ci + 24, qi, ys, yq)
    with pytest.raises(MlhotError, match="bg must be None"):
        ing.stage_ids(ci, qi, ys, yq, bg=(np.full(ci.shape, -1), np.full(qi.shape, -1)))
    with pytest.raises(MlhotError, match="AugTable"):
        ing.stage_ids(ci, qi, ys, yq, augment=t1.records)
    with pytest.raises(MlhotError, match="records for 20 images"):
        ing.stage_ids(ci, qi, ys, yq, augment=A.Sampler("shapenet_1d", seed=1).batch(10, 9, H, W))
    with pytest.raises(MlhotError, match="no background bank"):
        ResidentPool(pool, np.zeros((2, H, W, 3), dtype=np.uint8), device=DEV)
    assert not ing._queue
    # both table kinds through one ingest: each kind has its own slots (128- and 160-byte records)
    for t in (t1, ti, None):
        cx, qx, _, _ = ing.take(ing.stage_ids(ci, qi, ys, yq, augment=t))
        got = torch.cat([cx.reshape(-1, 1, H, W), qx.reshape(-1, 1, H, W)]).cpu().numpy()
        assert same_bits(got, _want_batch(pool, np.concatenate([ci.reshape(-1), qi.reshape(-1)]), t))


@pytest.mark.gpu
def test_a_three_slot_ring_drawn_two_ahead_stays_in_order(gpulib):
    from mlhot.ingest import BatchIngest, ResidentPool
    from mlhot.synth import SyntheticGreyPool
    data = SyntheticGreyPool("shapenet_1d", seed=6, pool=24, H=16, W=16)
    pool = data.grey_pool("train")
    ing = BatchIngest(DEV, slots=3, pool=ResidentPool(pool, device=DEV))
    sampler = A.Sampler("shapenet_1d", seed=3)
    drawn, tickets = [], []

    def draw():
        ci, qi, ys, yq = data.get_batch_ids("validation", 2, 4)                    # one shape: all batches share one slot ring and one _Out
        t = sampler.batch(ci.size, qi.size, 16, 16)
        drawn.append((np.concatenate([ci.reshape(-1), qi.reshape(-1)]), t, ys))
        tickets.append(ing.stage_ids(ci, qi, ys, yq, augment=t))
    draw(), draw()
    for k in range(6):
        draw()                                                                     # two ahead + the one about to be taken
        cx, qx, cy, _ = ing.take(tickets[k])
        ids, t, ys = drawn[k]
        got = torch.cat([cx.reshape(-1, 1, 16, 16), qx.reshape(-1, 1, 16, 16)]).cpu().numpy()
        assert same_bits(got, want_aug(pool, ids, t)) and torch.equal(cy.cpu(), ys), k
    assert len({id(s) for s in tickets}) == 3


# ---- 6. trainer ---------------------------------------------------------------------------------------------------------------------
class _Counting:
    """The loader, counting the byte-route calls; it speaks exactly what the inner loader speaks."""

    def __init__(self, inner):
        self.inner, self.calls, self.data_aug = inner, {"get_batch": 0, "get_batch_u8": 0, "get_batch_ids": 0}, False

    def gen_bg(self, *a, **k):
        pass

    def grey_pool(self, source="train"):
        return self.inner.grey_pool(source)

    def _count(name):
        def call(self, *a, **k):
            self.calls[name] += 1
            return getattr(self.inner, name)(*a, **k)
        return call
    get_batch, get_batch_u8, get_batch_ids = _count("get_batch"), _count("get_batch_u8"), _count("get_batch_ids")


CASES = {
    "shapenet_1d": ("ANPShapeNet1D", dict(task="shapenet_1d", input_dim=3, output_dim=2, agg_mode="attention", img_agg="", n_hidden_units_r=[100, 100],
                                          dim_r=64, dim_z=64, dim_w=64)),
    "shapenet_1d_aug": ("ANPShapeNet1D", dict(task="shapenet_1d", input_dim=3, output_dim=2, agg_mode="attention", img_agg="", n_hidden_units_r=[100, 100],
                                              dim_r=64, dim_z=64, dim_w=64, aug_list=["data_aug"], device_augment=True)),
    "distractor_aug": ("CNPDistractor", dict(task="distractor", input_dim=2, output_dim=2, agg_mode="max", img_agg="max", dim_w=16, temperature=0.07,
                                             aug_list=["data_aug"], device_augment_images=True)),
}


def _train(tmp_path, tag, case, resident, graph):
    import importlib
    from mlhot import binding
    from mlhot.synth import SyntheticGreyPool
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    method, over = CASES[case]
    # eager: a random context size per iteration (3 .. 5); replayed: shot 3 = one batch shape, so iterations 3 and 4 are replays
    cfg = dict(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, max_ctx_num=3 if graph else 5, beta=0, iterations=4,
               val_freq=1000, val_iters=1, bg_gen_freq=1000, gen_bg=False, contrastive=False, log_every=1, save_path=str(tmp_path / tag), logger=None)
    cfg.update(over)
    if not graph:
        cfg.update(graph_steps=False, lagged_loss_log=False)                      # graph: the trainer's own default decides, on both legs alike
    if resident:
        cfg.update(resident_pool=True)
    cfg = types.SimpleNamespace(**cfg)
    data = _Counting(SyntheticGreyPool(cfg.task, seed=9, pool=40))
    torch.manual_seed(0)
    model = getattr(importlib.import_module(f"networks.{method}"), method)(cfg).to(cfg.device)
    try:
        tr = ModelTrainer(model=model, loss=LossFunc("mse", cfg.task), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3), config=cfg, data=data)
        losses, report = [], tr._report
        tr._report = lambda it, v: (losses.append(v), report(it, v))[1]
        torch.manual_seed(31)
        tr.train()
        torch.cuda.synchronize()
    finally:
        binding.set_grad_arena(None)
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, losses, tr, data


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_trainer_resident_grey_pool_equals_the_byte_route(gpulib, tmp_path, case, graph):
    w_res, l_res, tr, data = _train(tmp_path, "r", case, True, graph)
    assert tr._resident and tr.ingest is not None and tr.ingest.pool.grey and (tr._augment is not None) == case.endswith("aug")
    assert data.calls["get_batch"] == 0 and data.calls["get_batch_u8"] == 0 and data.calls["get_batch_ids"] >= 4
    w_byte, l_byte, tr_b, data_b = _train(tmp_path, "b", case, False, graph)
    assert not tr_b._resident and tr_b.ingest is not None and tr_b.ingest.pool is None and tr_b._graph_default == tr._graph_default
    assert data_b.calls["get_batch_u8"] == data.calls["get_batch_ids"] and data_b.calls["get_batch_ids"] == 0
    if graph and tr._graph_default:             # where the byte route replays, so does this one
        assert any(not isinstance(g, str) for g in tr._graphs.values()) and any(not isinstance(g, str) for g in tr_b._graphs.values())
    print("losses", l_res, l_byte)
    assert len(l_res) == 4 and all(np.isfinite(v) for v in l_res)
    assert l_res == l_byte
    assert all(torch.equal(w_res[k], w_byte[k]) for k in w_res)
