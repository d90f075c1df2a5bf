"""The resident image pool on the MI355X: both entries against the oracle (tests/pool_ref.py) bit for bit, BatchIngest.stage_ids
shipping ids instead of image bytes, and the trainer with config.resident_pool against the same run on the host-composing twin."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_img_ref as RI
from tests import pool_ref as PR
from tests.test_pool_cpu import ALPHAS, SHAPES, all_off_records, pool_case, run_aug, run_plain, same_bits, sequence_case

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_pool_ingest_bit_exact(gpulib, n, H, W, alpha):
    pool, bank, ids, bg = pool_case(n, H, W, alpha)
    assert same_bits(run_plain(gpulib, pool, bank, ids, bg, DEV), PR.to_float(PR.compose(pool, bank, ids, bg)))
    assert same_bits(run_plain(gpulib, pool, None, ids, None, DEV), PR.to_float(pool[ids][..., :3]))
    arange = np.arange(pool.shape[0], dtype=np.int32)
    plain = gpulib.ingest_u8_nhwc(torch.from_numpy(np.ascontiguousarray(pool[..., :3])).to(DEV)).cpu().numpy()
    assert same_bits(run_plain(gpulib, pool, bank, arange, np.full(arange.shape, -1, dtype=np.int32), DEV), plain)
    assert same_bits(run_aug(gpulib, pool, bank, ids, bg, all_off_records(n, H, W), device=DEV), PR.to_float(PR.compose(pool, bank, ids, bg)))


@pytest.mark.gpu
def test_unaligned_views_take_the_any_size_path(gpulib):
    """A pool and a bank one byte into their buffers: neither the 16-byte quads nor the dword pixels may be read."""
    pool, bank, ids, bg = pool_case(5, 64, 64, "mixed")
    want = PR.to_float(PR.compose(pool, bank, ids, bg))
    bp = torch.zeros(pool.size + 1, dtype=torch.uint8, device=DEV)
    bb = torch.zeros(bank.size + 1, dtype=torch.uint8, device=DEV)
    bp[1:] = torch.from_numpy(pool).to(DEV).view(-1)
    bb[1:] = torch.from_numpy(bank).to(DEV).view(-1)
    p1, b1 = bp[1:].view(pool.shape), bb[1:].view(bank.shape)
    i, g = torch.from_numpy(ids).to(DEV), torch.from_numpy(bg).to(DEV)
    assert same_bits(gpulib.pool_ingest_u8(p1, i, b1, g).cpu().numpy(), want)
    recs = torch.from_numpy(all_off_records(5, 64, 64)).to(DEV)
    assert same_bits(gpulib.pool_augment_ingest_u8_img(p1, i, recs, b1, g).cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(64, 64), (7, 5), (1, 1)])
def test_whole_sequences_bit_exact(gpulib, H, W):
    pool, bank, ids, bg, t = sequence_case(H, W)
    got = run_aug(gpulib, pool, bank, ids, bg, t.records, t.luts, device=DEV)
    assert same_bits(got, RI.augment_batch(PR.compose(pool, bank, ids, bg), t.records, t.luts, t.pre_op, t.div, t.div2))


@pytest.mark.gpu
def test_one_600_image_batch_bit_exact(gpulib):
    from mlhot.synth import SyntheticViewsRGBA
    pool, bank = SyntheticViewsRGBA(seed=5, objects=8, views=30).rgba_pool("train")
    ids = np.random.default_rng(1).integers(0, pool.shape[0], 600).astype(np.int32)
    bg = PR.bg_indices(2578, 4, ids, bank.shape[0])
    bg[::50] = -1
    assert same_bits(run_plain(gpulib, pool, bank, ids, bg, DEV), PR.to_float(PR.compose(pool, bank, ids, bg)))


@pytest.mark.gpu
@pytest.mark.parametrize("augmented", [False, True])
def test_stage_ids_ships_no_image_bytes(gpulib, augmented):
    from mlhot.binding import AUG_IMG_RECORD_BYTES, MlhotError
    from mlhot.ingest import BatchIngest, ResidentPool
    from mlhot.synth import SyntheticViewsRGBA
    data = SyntheticViewsRGBA(seed=4, objects=3, views=12)
    images, bank = data.rgba_pool("train")
    ing = BatchIngest(DEV, pool=ResidentPool(images, bank, DEV))
    sampler, bgs = A.ImageSampler("shapenet_3d", seed=8), A.BackgroundSampler(bank.shape[0], seed=8)
    for epoch in (0, 2):
        ci, qi, ys, yq = data.get_batch_ids("train", 2, 5)
        t = sampler.batch(ci.size, qi.size, 64, 64) if augmented else None
        bg = (bgs.batch(ci, epoch), bgs.batch(qi, epoch))
        slot = ing.stage_ids(ci, qi, ys, yq, bg=bg, augment=t)
        n, labels = ci.size + qi.size, 4 * (ys.numel() + yq.numel())
        want_bytes = (8 * n + 15) // 16 * 16 + labels                              # ids + bg (padded to 16) + labels ...
        if augmented:
            want_bytes = (want_bytes + 15) // 16 * 16 + AUG_IMG_RECORD_BYTES * n + 256 * t.luts.shape[0]        # ... + records + LUTs in use
        # per image at most 8 (id, bg) + 16 (label) + 160 (record) + 256 (LUT) bytes: under a sixteenth of its 12288 image bytes
        assert slot.n_bytes == want_bytes and want_bytes < n * 64 * 64 * 3 // 16
        cx, qx, cy, qy = ing.take(slot)
        ids, b = np.concatenate([ci.reshape(-1), qi.reshape(-1)]), np.concatenate([bg[0].reshape(-1), bg[1].reshape(-1)])
        composed = PR.compose(images, bank, ids, b)
        want = RI.augment_batch(composed, t.records, t.luts, t.pre_op, t.div, t.div2) if augmented else PR.to_float(composed)
        got = torch.cat([cx.reshape(-1, 3, 64, 64), qx.reshape(-1, 3, 64, 64)]).cpu().numpy()
        assert cx.shape == (2, 5, 3, 64, 64) and same_bits(got, want)
        assert torch.equal(cy.cpu(), ys) and torch.equal(qy.cpu(), yq)
        assert (epoch == 0) == (b == -1).all()
    ci, qi, ys, yq = data.get_batch_ids("train", 2, 5)
    for bad_ci, bad_bg in ((ci + images.shape[0], None), (ci, (np.full(ci.shape, bank.shape[0]), np.full(qi.shape, -1)))):
        with pytest.raises(MlhotError, match="out of range"):
            ing.stage_ids(bad_ci, qi, ys, yq, bg=bad_bg)
    assert not ing._queue                                                          # nothing was shipped


# ---- trainer ------------------------------------------------------------------------------------------------------------------------
class _Counting:
    """The loader, counting the regenerations the trainer asks for."""

    def __init__(self, inner):
        self.inner, self.gen_bg_calls, self.data_aug = inner, 0, False
        for name in ("rgba_pool", "get_batch_ids", "get_batch_u8", "get_batch"):
            if hasattr(inner, name):
                setattr(self, name, getattr(inner, name))

    def gen_bg(self, *a, **k):
        self.gen_bg_calls += 1
        self.inner.gen_bg(*a, **k)


def _train(tmp_path, tag, resident, augment):
    from mlhot import binding
    from mlhot.synth import SyntheticViewsRGBA, SyntheticViewsRGBAHost
    from networks.ANPMRShapeNet3D import ANPMRShapeNet3D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    cfg = dict(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4, agg_mode="attention",
               img_agg="reshape", task="shapenet_3d", temperature=0.07, max_ctx_num=5, beta=1e-7, iterations=6, val_freq=1000, val_iters=1,
               bg_gen_freq=2, gen_bg=True, contrastive=False, log_every=1, graph_steps=False, lagged_loss_log=False,
               save_path=str(tmp_path / tag), logger=None)
    if augment:
        cfg.update(aug_list=["data_aug"], device_augment_images=True)
    if resident:
        cfg.update(resident_pool=True)
        data = _Counting(SyntheticViewsRGBA(seed=9))
    else:
        data = _Counting(SyntheticViewsRGBAHost(A.BackgroundSampler(5, seed=2578, bg_gen_freq=2), seed=9))
    cfg = types.SimpleNamespace(**cfg)
    torch.manual_seed(0)
    model = ANPMRShapeNet3D(cfg).to(cfg.device)
    seen = []
    model.register_forward_pre_hook(lambda m, args: seen.append(args[2].detach().cpu().numpy().copy()))
    try:
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_3d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3),
                          config=cfg, data=data)
        losses, report = [], tr._report
        tr._report = lambda it, v: (losses.append(v), report(it, v))[1]
        torch.manual_seed(31)
        tr.train()
        torch.cuda.synchronize()
    finally:
        binding.set_grad_arena(None)
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, losses, tr, data, seen


@pytest.mark.gpu
@pytest.mark.parametrize("augment", [False, True])
def test_trainer_resident_pool_equals_the_host_composing_route(gpulib, tmp_path, augment):
    """Six iterations, bg_gen_freq = 2: epochs 0, 1, 1, 2, 2, 3.  Losses and final weights of the resident route are those of the twin
    that composes on the host and ships fp32 batches through the existing host-batch route."""
    w_res, l_res, tr, data, seen_res = _train(tmp_path, "r", True, augment)
    assert tr._resident and tr.ingest is not None and tr.ingest.pool.n_bank == 5 and data.gen_bg_calls == 0
    assert tr._feed.train_it >= 7 and (tr._augment is not None) == augment
    w_host, l_host, tr_h, data_h, seen_host = _train(tmp_path, "h", False, augment)
    assert not tr_h._resident and tr_h._host_prefetch is not None and data_h.gen_bg_calls == 3 and data_h.inner.epoch == 3
    assert len(l_res) == 6 and all(np.isfinite(v) for v in l_res)
    print("losses", l_res, l_host)
    assert all(same_bits(a, b) for a, b in zip(seen_res, seen_host)) and len(seen_res) == len(seen_host) >= 6
    assert l_res == l_host
    assert all(torch.equal(w_res[k], w_host[k]) for k in w_res)
