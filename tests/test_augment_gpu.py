"""Device data augmentation on the MI355X: the fused kernel (csrc/augment.h) against the oracle (tests/augment_ref.py) bit for bit,
the all-off case against mlhot_ingest_u8_nhwc, and the trainer with config.device_augment on both batch routes."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_ref as R
from tests.test_augment_cpu import _isolated_records

DEV = "cuda:0"


def _kernel(lib, imgs, records, luts=None):
    out = lib.augment_ingest_u8(torch.from_numpy(np.ascontiguousarray(imgs[..., None])).to(DEV), torch.from_numpy(records).to(DEV),
                                None if luts is None or len(luts) == 0 else torch.from_numpy(luts).to(DEV))
    return out.cpu().numpy()[:, 0]


def _want(imgs, records, luts=None):
    return R.augment_batch(imgs, records, luts).astype(np.float32) / np.float32(255.0)       # the ingest's divide


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(128, 128), (37, 53), (61, 128), (3, 5)])
def test_each_op_alone_bit_exact(gpulib, H, W):
    rng = np.random.default_rng(H * 7 + W)
    one = _isolated_records(H, W, rng)
    recs = np.concatenate([one] * (200 // len(one) + 1))[:200]                  # a batch of 200 images
    recs[:, A.F_IMAGE] = np.arange(len(recs))
    luts = A.gamma_luts([0.5, 1.7])
    imgs = rng.integers(0, 256, (len(recs), H, W), dtype=np.uint8)
    got = _kernel(gpulib, imgs, recs, luts)
    want = _want(imgs, recs, luts)
    bad = [i for i in range(len(recs)) if not np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32))]
    assert not bad, [recs[i][:27].tolist() for i in bad[:3]]


@pytest.mark.gpu
@pytest.mark.parametrize("task,T,Nc,Nq,H,W", [("shapenet_1d", 10, 15, 15, 128, 128), ("pascal_1d", 10, 15, 15, 128, 128),
                                               ("shapenet_1d", 20, 15, 15, 67, 45), ("pascal_1d", 40, 7, 8, 101, 33)])
def test_whole_sequences_bit_exact(gpulib, task, T, Nc, Nq, H, W):
    from mlhot.synth import shape_images
    t = A.Sampler(task, seed=T + H).batch(T * Nc, T * Nq, H, W)
    imgs = shape_images(T * (Nc + Nq), H, W, seed=W)
    got = _kernel(gpulib, imgs, t.records, t.luts)
    assert np.array_equal(got.view(np.uint32), _want(imgs, t.records, t.luts).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(128, 128), (37, 41)])
def test_all_off_equals_plain_ingest(gpulib, H, W):
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, (300, H, W), dtype=np.uint8)
    recs = A.Sampler("pascal_1d", seed=2).batch(150, 150, H, W).records.copy()
    recs[:, A.F_ON] = 0
    got = _kernel(gpulib, imgs, recs)
    plain = gpulib.ingest_u8_nhwc(torch.from_numpy(imgs[..., None]).to(DEV)).cpu().numpy()[:, 0]
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


@pytest.mark.gpu
def test_batch_ingest_ships_the_table_with_the_batch(gpulib):
    """stage(..., augment=table) + take(): the records and LUTs travel in the slot; the result is the kernel's on the same bytes."""
    from mlhot.ingest import BatchIngest
    from mlhot.synth import SyntheticShapes
    data = SyntheticShapes("pascal_1d", seed=4)
    ing = BatchIngest(DEV)
    for _ in range(3):
        xs, xq, ys, yq = data.get_batch_u8("train", 10, 15)
        n_ctx = xs.shape[0] * xs.shape[1]
        t = A.Sampler("pascal_1d", seed=int(n_ctx)).batch(n_ctx, xq.shape[0] * xq.shape[1], 128, 128)
        cx, qx, cy, qy = ing.take(ing.stage(xs, xq, ys, yq, augment=t))
        imgs = np.concatenate([xs.reshape(-1, 128, 128), xq.reshape(-1, 128, 128)])
        want = _want(imgs, t.records, t.luts)
        got = torch.cat([cx.reshape(-1, 128, 128), qx.reshape(-1, 128, 128)]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert torch.equal(cy.cpu(), ys) and torch.equal(qy.cpu(), yq)
        cx, qx = cx.clone(), qx.clone()                   # batches of one shape share their output tensors
        plain = ing.take(ing.stage(xs, xq, ys, yq))
        assert not torch.equal(plain[0], cx) and not torch.equal(plain[1], qx)


def split_geometry_case(sampler, C, direct, as_table=None):
    """Context images [2, 3, 8, 8, C] and targets [2, 2, 12, 8, C] through BatchIngest.stage() + take(): one launch per side.  The table
    is drawn as Sampler.batch draws it - one side() call per side, the targets' LUT rows behind the context's - and each side must equal,
    bit for bit, `direct(side's bytes, its rows of the records, the WHOLE LUT table)` - the library entry called directly."""
    from mlhot.ingest import BatchIngest
    rng = np.random.default_rng(5)
    ing = BatchIngest(DEV)
    for _ in range(2):                                    # the second batch reuses the first one's slot
        xs, xq = rng.integers(0, 256, (2, 3, 8, 8, C), dtype=np.uint8), rng.integers(0, 256, (2, 2, 12, 8, C), dtype=np.uint8)
        ys, yq = torch.from_numpy(rng.random((2, 3, 3), dtype=np.float32)), torch.from_numpy(rng.random((2, 2, 3), dtype=np.float32))
        t = luts = None
        rows = [None, None]
        if sampler is not None:
            rc, lc = sampler.side(6, 8, 8, 0)
            rq, lq = sampler.side(4, 12, 8, 1, lut_base=lc.shape[0])
            sampler.counter += 1
            t = A.AugTable(np.concatenate([rc, rq]), np.concatenate([lc, lq]))
            t = t if as_table is None else as_table(t)
            rows = [torch.from_numpy(t.records[:6]).to(DEV), torch.from_numpy(t.records[6:]).to(DEV)]
            luts = torch.from_numpy(t.luts).to(DEV) if len(t.luts) else None
        cx, qx, cy, qy = ing.take(ing.stage(xs, xq, ys, yq, augment=t))
        assert cx.shape == (2, 3, C, 8, 8) and qx.shape == (2, 2, C, 12, 8)
        for got, x, rec in ((cx, xs, rows[0]), (qx, xq, rows[1])):
            want = direct(torch.from_numpy(x).to(DEV), rec, luts, t)
            assert want.shape == got.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(cy.cpu(), ys) and torch.equal(qy.cpu(), yq)
    return t


@pytest.mark.gpu
def test_batch_ingest_split_geometry_plain(gpulib):
    split_geometry_case(None, 1, lambda src, rec, luts, t: gpulib.ingest_u8_nhwc(src))


@pytest.mark.gpu
def test_batch_ingest_split_geometry_with_a_table(gpulib):
    t = split_geometry_case(A.Sampler("pascal_1d", seed=6), 1, lambda src, rec, luts, t: gpulib.augment_ingest_u8(src, rec, luts))
    assert (t.records[:6, A.F_LUT] >= 0).any() and (t.records[6:, A.F_LUT] >= 0).any()        # both sides index the one LUT table


# ---- trainer ---------------------------------------------------------------------------------------------------------------------
def _train(tmp_path, tag, data, **over):
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    cfg = dict(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=4, input_dim=3, output_dim=2,
               agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d",
               iterations=6, val_freq=1000, val_iters=1, bg_gen_freq=1000, gen_bg=False, max_ctx_num=15, beta=0, contrastive=False,
               aug_list=["data_aug"], device_augment=True, host_prefetch_depth=2, save_path=str(tmp_path / tag), logger=None)
    cfg.update(over)
    cfg = types.SimpleNamespace(**{k: v for k, v in cfg.items() if v is not _UNSET})
    torch.manual_seed(0)
    model = ANPShapeNet1D(cfg).to(cfg.device)
    tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3),
                      config=cfg, data=data)
    losses, report = [], tr._report
    tr._report = lambda it, v: (losses.append(v), report(it, v))[1]
    tr.train()                                             # host_prefetch_depth 2: batches drawn ahead under the steps
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, losses, tr


_UNSET = object()


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["ingest", "host"])
def test_trainer_device_augment(gpulib, tmp_path, route):
    from mlhot.synth import SyntheticShapes, SyntheticShapesF32
    mk = (lambda: SyntheticShapes(seed=9)) if route == "ingest" else (lambda: SyntheticShapesF32(seed=9))
    w_aug, losses, tr = _train(tmp_path, "a", mk(), graph_steps=False, lagged_loss_log=False)
    assert tr._augment is not None and ((tr.ingest is not None) == (route == "ingest"))
    assert len(losses) == 6 and all(np.isfinite(v) for v in losses)
    w_aug2, _, _ = _train(tmp_path, "b", mk(), graph_steps=False, lagged_loss_log=False)
    assert _same(w_aug, w_aug2)                                                     # same seed: bit-identical weights
    w_graph, _, _ = _train(tmp_path, "c", mk(), graph_steps=True, lagged_loss_log=False)
    assert _same(w_aug, w_graph)                                                    # replayed steps = the eager loop
    w_off, _, tr_off = _train(tmp_path, "d", mk(), graph_steps=False, lagged_loss_log=False, device_augment=False)
    w_unset, _, _ = _train(tmp_path, "e", mk(), graph_steps=False, lagged_loss_log=False, device_augment=_UNSET, aug_list=_UNSET)
    assert tr_off._augment is None and _same(w_off, w_unset)                        # off = today's path
    assert not _same(w_aug, w_off)                                                  # the augmented batches differ


@pytest.mark.gpu
def test_trainer_refuses_non_byte_batches(gpulib, tmp_path):
    from mlhot.synth import SyntheticShapesF32

    class Noisy(SyntheticShapesF32):
        def get_batch(self, source, tasks_per_batch, shot):
            xs, xq, ys, yq = SyntheticShapesF32.get_batch(self, source, tasks_per_batch, shot)
            return xs * 0.999, xq, ys, yq                                           # no longer k / 255
    with pytest.raises(ValueError, match="not exact bytes"):
        _train(tmp_path, "n", Noisy(seed=1), graph_steps=False, host_copy_thread=False)
