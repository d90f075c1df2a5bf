"""Device augmentation of the image tasks on the MI355X: the fused kernel (csrc/augment_img.h) against the oracle
(tests/augment_img_ref.py) bit for bit, the all-off case against mlhot_ingest_u8_nhwc, BatchIngest shipping an ImageAugTable, and the
trainer with config.device_augment_images on both batch routes."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_img_ref as RI
from tests.test_augment_img_cpu import isolated_case, run_lib, sequence_case

DEV = "cuda:0"


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C", [(64, 64, 3), (37, 53, 3), (3, 5, 3), (128, 128, 1)])
def test_each_op_alone_bit_exact(gpulib, H, W, C):
    imgs, recs, luts = isolated_case(H, W, C, H * 7 + W)
    got = run_lib(gpulib, imgs, recs, luts, device=DEV)
    want = RI.augment_batch(imgs, recs, luts)
    bad = [i for i in range(len(recs)) if not _same_bits(got[i], want[i])]
    assert not bad, [recs[i].tolist() for i in bad[:3]]


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["shapenet_3d", "distractor"])
@pytest.mark.parametrize("H,W,C", [(64, 64, 3), (37, 53, 3), (3, 5, 3), (128, 128, 1)])
def test_whole_sequences_bit_exact(gpulib, task, H, W, C):
    imgs, t = sequence_case(task, H, W, C, n_ctx=2 * 3, n_qry=2 * 5)              # T = 2, Nc = 3, Nq = 5
    got = run_lib(gpulib, imgs, t.records, t.luts, t.pre_op, t.div, t.div2, device=DEV)
    assert _same_bits(got, RI.augment_batch(imgs, t.records, t.luts, t.pre_op, t.div, t.div2))


@pytest.mark.gpu
def test_one_shapenet3d_batch_bit_exact(gpulib):
    imgs, t = sequence_case("shapenet_3d", 64, 64, 3, n_ctx=8, n_qry=12, seed=20)  # 20 images of 64 x 64 x 3
    got = run_lib(gpulib, imgs, t.records, t.luts, t.pre_op, t.div, t.div2, device=DEV)
    assert _same_bits(got, RI.augment_batch(imgs, t.records, t.luts, t.pre_op, t.div, t.div2))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C", [(64, 64, 3), (37, 41, 3), (128, 128, 1)])
def test_all_off_equals_plain_ingest(gpulib, H, W, C):
    n = 40
    buf = torch.from_numpy(np.random.default_rng(3).integers(0, 256, n * H * W * C + 1, dtype=np.uint8)).to(DEV)
    recs = A.ImageSampler("shapenet_3d", seed=2).batch(n // 2, n // 2, H, W).records.copy()
    recs[:, A.F_ON] = 0
    recs = torch.from_numpy(recs).to(DEV)
    for off in (0, 1):                                      # off 1: a view one byte in - the scalar loads
        src = buf[off:off + n * H * W * C].view(n, H, W, C)
        got = gpulib.augment_ingest_u8_img(src, recs, None, None)
        plain = gpulib.ingest_u8_nhwc(src)
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), off


@pytest.mark.gpu
@pytest.mark.parametrize("task", ["shapenet_3d", "distractor"])
def test_batch_ingest_ships_the_image_table_with_the_batch(gpulib, task):
    from mlhot.ingest import BatchIngest
    from mlhot.synth import SyntheticViews
    data = SyntheticViews(task, seed=4, mode="train")
    ing = BatchIngest(DEV)
    sampler = A.ImageSampler(task, seed=8)
    for _ in range(2):
        xs, xq, ys, yq = data.get_batch_u8("train", 2, 3)
        H, W, C = xs.shape[2:]
        t = sampler.batch(xs.shape[0] * xs.shape[1], xq.shape[0] * xq.shape[1], H, W)
        cx, qx, cy, qy = ing.take(ing.stage(xs, xq, ys, yq, augment=t))
        imgs = np.concatenate([xs.reshape(-1, H, W, C), xq.reshape(-1, H, W, C)])
        want = RI.augment_batch(imgs, t.records, t.luts, t.pre_op, t.div, t.div2)
        got = torch.cat([cx.reshape(-1, C, H, W), qx.reshape(-1, C, H, W)]).cpu().numpy()
        assert _same_bits(got, want)
        assert torch.equal(cy.cpu(), ys) and torch.equal(qy.cpu(), yq)
        cx = cx.clone()
        assert not torch.equal(ing.take(ing.stage(xs, xq, ys, yq))[0], cx)


@pytest.mark.gpu
@pytest.mark.parametrize("task,C", [("shapenet_3d", 3), ("distractor", 1)])
def test_batch_ingest_split_geometry_with_an_image_table(gpulib, task, C):
    from tests.test_augment_gpu import split_geometry_case
    sampler = A.ImageSampler(task, seed=6)
    split_geometry_case(sampler, C, lambda src, rec, luts, t: gpulib.augment_ingest_u8_img(src, rec, luts, A.colour_tables(DEV), pre_op=t.pre_op,
                                                                                           div=t.div, div2=t.div2),
                        as_table=lambda t: A.ImageAugTable(t.records, t.luts, sampler.spec))


# ---- trainer ---------------------------------------------------------------------------------------------------------------------
_UNSET = object()


class _Recording:
    """A loader that remembers the bytes of the training batches it handed out, in order."""

    def __init__(self, inner, u8):
        self.inner, self.train_bytes, self.data_aug = inner, [], False
        if u8:
            self.get_batch_u8 = self._get_u8

    def gen_bg(self, *a, **k):
        pass

    def _get_u8(self, source, tasks_per_batch, shot):
        out = self.inner.get_batch_u8(source, tasks_per_batch, shot)
        if source == "train":
            self.train_bytes.append((out[0].copy(), out[1].copy()))
        return out

    def get_batch(self, source, tasks_per_batch, shot):
        out = self.inner.get_batch(source, tasks_per_batch, shot)
        if source == "train":                               # fp32 [T, N, C, H, W] = k / 255 -> the bytes, channel-last
            self.train_bytes.append(tuple(np.rint(x.numpy() * 255.0).astype(np.uint8).transpose(0, 1, 3, 4, 2) for x in out[:2]))
        return out


def _train(tmp_path, tag, route, **over):
    from mlhot import binding
    from mlhot.synth import SyntheticViews, SyntheticViewsF32
    from networks.ANPMRShapeNet3D import ANPMRShapeNet3D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    cfg = dict(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4, agg_mode="attention",
               img_agg="reshape", task="shapenet_3d", temperature=0.07, max_ctx_num=4, beta=1e-7, iterations=3, val_freq=1000, val_iters=1,
               bg_gen_freq=1000, gen_bg=False, contrastive=False, log_every=1, graph_steps=False, lagged_loss_log=False,
               aug_list=["data_aug"], device_augment_images=True, save_path=str(tmp_path / tag), logger=None)
    cfg.update(over)
    cfg = types.SimpleNamespace(**{k: v for k, v in cfg.items() if v is not _UNSET})
    inner = SyntheticViews("shapenet_3d", seed=9, mode="train") if route == "ingest" else SyntheticViewsF32("shapenet_3d", seed=9)
    data = _Recording(inner, u8=route == "ingest")
    torch.manual_seed(0)
    model = ANPMRShapeNet3D(cfg).to(cfg.device)
    seen = []
    model.register_forward_pre_hook(lambda m, args: seen.append((args[0].detach().cpu().numpy().copy(), args[2].detach().cpu().numpy().copy())))
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


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["ingest", "host"])
def test_trainer_device_augment_images(gpulib, tmp_path, route):
    w_aug, losses, tr, data, seen = _train(tmp_path, "a", route)
    assert isinstance(tr._augment, A.ImageSampler) and ((tr.ingest is not None) == (route == "ingest"))
    assert len(losses) == 3 and all(np.isfinite(v) for v in losses) and len(seen) >= 3
    sampler = A.ImageSampler("shapenet_3d", seed=2578, rank=0)           # the trainer's stream: (config.seed, rank)
    for (cx, qx), (xs, xq) in zip(seen, data.train_bytes):               # batches are drawn, and their tables with them, in order
        T, Nc, H, W, C = xs.shape
        t = sampler.batch(T * Nc, T * xq.shape[1], H, W)
        want = RI.augment_batch(np.concatenate([xs.reshape(-1, H, W, C), xq.reshape(-1, H, W, C)]), t.records, t.luts, t.pre_op, t.div, t.div2)
        got = np.concatenate([cx.reshape(-1, C, H, W), qx.reshape(-1, C, H, W)])
        assert _same_bits(got, want)
    w_off, _, tr_off, _, seen_off = _train(tmp_path, "b", route, device_augment_images=False)
    w_unset, _, _, _, _ = _train(tmp_path, "c", route, device_augment_images=_UNSET, aug_list=_UNSET)
    assert tr_off._augment is None and _same(w_off, w_unset)            # off = today's path
    assert not _same(w_aug, w_off) and not np.array_equal(seen[0][0], seen_off[0][0])
