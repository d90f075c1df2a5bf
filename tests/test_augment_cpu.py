"""Device data augmentation without a GPU: the oracle (tests/augment_ref.py) against numpy's own definitions, the host sampler
(mlhot/augment.py), the kernel's functors in the host build (the `hostsim` fixture) against the oracle bit for bit, and the
trainer's refusals."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_ref as R


def _img(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _record(op=None, **f):
    """A record with one step (or none) switched on, fields by mlhot.augment.F_* name suffix."""
    rec = np.zeros(A.RECORD_INTS, dtype=np.int32)
    u = rec.view(np.uint32)
    rec[A.F_N_STEPS] = 1 if op is not None else 0
    rec[A.F_OP] = op if op is not None else 0
    rec[A.F_ON] = (1 << op) if op is not None else 0
    rec[A.F_AFF_AX] = rec[A.F_AFF_AY] = 65536
    rec[A.F_BLUR_K] = 1
    rec[A.F_COARSE_H] = rec[A.F_COARSE_W] = 3
    for k, v in f.items():
        idx = getattr(A, "F_" + k.upper())
        if k in ("drop_thresh", "coarse_thresh", "seed", "counter", "side", "image"):
            u[idx] = v
        elif k == "pad":
            rec[idx:idx + 4] = v
        else:
            rec[idx] = v
    return rec


# ---- oracle sanity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(128, 128), (17, 31)])
def test_oracle_identities(H, W):
    img = _img(H, W)
    ident = np.arange(256, dtype=np.uint8)[None]
    assert np.array_equal(R.augment(img, _record(A.CROP_PAD, pad=[0, 0, 0, 0], pad_mode=3)), img)
    assert np.array_equal(R.resize_cubic(img, H, W), img)
    for mode in range(A.N_AFFINE_MODES):
        for order in (0, 1):
            rec = _record(A.AFFINE, aff_order=order, aff_mode=mode, aff_cval=77, aff_bx=0, aff_by=0)
            assert np.array_equal(R.augment(img, rec), img), (mode, order)
    assert np.array_equal(R.augment(img, _record(A.BLUR, blur_k=1)), img)
    assert np.array_equal(R.augment(img, _record(A.GAMMA, lut=0), A.gamma_luts([1.0])), img)
    assert np.array_equal(A.gamma_luts([1.0]), ident)
    assert np.array_equal(R.augment(img, _record(A.DROPOUT, drop_thresh=0)), img)
    assert np.array_equal(R.augment(img, _record(A.COARSE_DROPOUT, coarse_thresh=0)), img)


def test_oracle_pad_modes_are_np_pad():
    img = _img(9, 7)
    kw = {0: {"constant_values": 200}, 2: {"end_values": 200}}
    for mode, name in enumerate(R.PAD_MODES):
        got = R.pad(img, 1, 3, 2, 4, mode, 200)
        assert np.array_equal(got, np.pad(img, ((1, 2), (4, 3)), mode=name, **kw.get(mode, {}))), name
        assert got.shape == (12, 14) and np.array_equal(got[1:10, 4:11], img)


@pytest.mark.parametrize("shift", [(2, -3), (-1, 5)])
def test_oracle_whole_pixel_translation(shift):
    """order 0, scale 1, a whole-pixel shift: a shifted copy with that mode's border (np.pad's modes of the same name)."""
    img = _img(11, 13)
    dy, dx = shift
    np_mode = {0: "constant", 1: "edge", 2: "symmetric", 3: "reflect", 4: "wrap"}
    for mode in range(A.N_AFFINE_MODES):
        rec = _record(A.AFFINE, aff_order=0, aff_mode=mode, aff_cval=99, aff_bx=-dx * 65536, aff_by=-dy * 65536)
        got = R.augment(img, rec)
        p = 8
        big = np.pad(img, p, mode=np_mode[mode], **({"constant_values": 99} if mode == 0 else {}))
        want = big[p - dy:p - dy + 11, p - dx:p - dx + 13]
        assert np.array_equal(got, want), mode


# ---- sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["shapenet_1d", "pascal_1d"])
def test_sampler_rates_and_ranges(task):
    s = A.Sampler(task, seed=3)
    n = 20000
    rec, luts = s.side(n, 128, 128, side=0)
    steps = A.AugmentSpec.for_task(task).steps
    ops = rec[:, A.F_OP:A.F_OP + len(steps)]
    assert (rec[:, A.F_N_STEPS] == len(steps)).all()
    assert len({tuple(r) for r in ops[:, :][:, :]}) <= 2            # one permutation per call (up to the OneOf member)
    on = rec[:, A.F_ON]
    for code in set(steps) - {A.ONEOF}:
        assert abs(((on >> code) & 1).mean() - 0.5) < 0.02, code
    is_coarse = (ops == A.COARSE_DROPOUT).any(axis=1)
    assert abs(is_coarse.mean() - 0.5) < 0.02
    oneof_on = ((on >> A.DROPOUT) & 1) | ((on >> A.COARSE_DROPOUT) & 1)
    assert abs(oneof_on.mean() - 0.5) < 0.02
    pad = rec[:, A.F_PAD:A.F_PAD + 4]
    assert pad.min() == 0 and pad.max() == 6                            # round(U(0, 0.05) * 128)
    assert set(np.unique(rec[:, A.F_PAD_MODE])) == set(range(10))
    assert rec[:, A.F_PAD_CVAL].min() == 0 and rec[:, A.F_PAD_CVAL].max() == 255
    assert set(np.unique(rec[:, A.F_BLUR_K])) == {1, 2, 3}
    assert set(np.unique(rec[:, A.F_AFF_ORDER])) == {0, 1} and set(np.unique(rec[:, A.F_AFF_MODE])) == set(range(5))
    sx = 65536.0 / rec[:, A.F_AFF_AX]
    assert sx.min() >= 0.8 - 1e-4 and sx.max() <= 1.2 + 1e-4
    cx = 63.5
    tx = (cx - rec[:, A.F_AFF_BX] / 65536.0) * sx - cx                 # bx = 2^16 (cx - (cx + tx W) / sx)
    assert tx.min() >= -12.8 - 0.01 and tx.max() <= 12.8 + 0.01
    u = rec.view(np.uint32)
    p_drop = u[:, A.F_DROP_THRESH] / 2.0 ** 32
    p_coarse = u[:, A.F_COARSE_THRESH] / 2.0 ** 32
    assert p_drop.min() >= 0.01 - 1e-9 and p_drop.max() <= 0.1 and p_coarse.max() <= 0.05
    assert rec[:, A.F_COARSE_H].min() == 3 and rec[:, A.F_COARSE_H].max() == 32
    assert (rec[:, A.F_IMAGE] == np.arange(n)).all() and (u[:, A.F_SIDE] == 0).all()
    if A.GAMMA in steps:
        g_on = (on >> A.GAMMA) & 1 == 1
        assert luts.shape == (g_on.sum(), 256) and (rec[g_on, A.F_LUT] == np.arange(g_on.sum())).all()
    else:
        assert luts.shape == (0, 256)


def test_sampler_determinism_ranks_and_global_rng():
    state = np.random.get_state()
    a = A.Sampler("pascal_1d", seed=5, rank=0).batch(30, 40, 128, 128)
    b = A.Sampler("pascal_1d", seed=5, rank=0).batch(30, 40, 128, 128)
    c = A.Sampler("pascal_1d", seed=5, rank=1).batch(30, 40, 128, 128)
    after = np.random.get_state()
    assert np.array_equal(a.records, b.records) and np.array_equal(a.luts, b.luts)
    assert not np.array_equal(a.records, c.records)
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert a.n_img == 70 and (a.records.view(np.uint32)[:30, A.F_SIDE] == 0).all() and (a.records.view(np.uint32)[30:, A.F_SIDE] == 1).all()


def test_spec_refuses_other_tasks():
    for task in ("shapenet_3d", "distractor"):
        with pytest.raises(NotImplementedError):
            A.AugmentSpec.for_task(task)


# ---- the kernel's functors (host build) against the oracle ------------------------------------------------------------------------
def _run(hostsim, imgs, records, luts=None):
    out = hostsim.augment_ingest_u8(torch.from_numpy(np.ascontiguousarray(imgs[..., None])), torch.from_numpy(np.ascontiguousarray(records)),
                                    None if luts is None or len(luts) == 0 else torch.from_numpy(np.ascontiguousarray(luts)))
    return out.numpy()[:, 0]


def _expect(imgs, records, luts=None):
    return R.augment_batch(imgs, records, luts).astype(np.float32) / np.float32(255.0)


SIZES = [(128, 128), (37, 53), (61, 128), (3, 5)]


def _isolated_records(H, W, rng):
    """Every op alone, every pad / border mode, both orders."""
    recs = []
    for mode in range(A.N_PAD_MODES):
        for pad in ([1, 2, 3, 0], [6, 6, 6, 6], [0, 0, 2, 0], [int(x) for x in rng.integers(0, 7, 4)]):
            recs.append(_record(A.CROP_PAD, pad=pad, pad_mode=mode, pad_cval=int(rng.integers(0, 256))))
    recs.append(_record(A.CROP_PAD, pad=[0, 0, 0, 0], pad_mode=4))
    for mode in range(A.N_AFFINE_MODES):
        for order in (0, 1):
            sx, sy, tx, ty = rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
            ax, bx, ay, by = (int(v[0]) for v in A.affine_fixed(np.array([sx]), np.array([sy]), np.array([tx]), np.array([ty]), H, W))
            recs.append(_record(A.AFFINE, aff_order=order, aff_mode=mode, aff_cval=int(rng.integers(0, 256)), aff_ax=ax, aff_bx=bx,
                                aff_ay=ay, aff_by=by))
    for k in (1, 2, 3):
        recs.append(_record(A.BLUR, blur_k=k))
    recs.append(_record(A.GAMMA, lut=0))
    recs.append(_record(A.GAMMA, lut=1))
    for p in (0.01, 0.1, 0.5):
        recs.append(_record(A.DROPOUT, drop_thresh=int(p * 2 ** 32), seed=7, counter=3, side=1, image=len(recs)))
    for p, ch, cw in ((0.05, 3, 3), (0.5, 7, 32), (0.3, 32, 5)):
        recs.append(_record(A.COARSE_DROPOUT, coarse_thresh=int(p * 2 ** 32), coarse_h=ch, coarse_w=cw, seed=9, image=len(recs)))
    return np.stack(recs)


@pytest.mark.parametrize("H,W", SIZES)
def test_hostsim_each_op_alone_bit_exact(hostsim, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    recs = _isolated_records(H, W, rng)
    luts = A.gamma_luts([0.5, 1.7])
    imgs = rng.integers(0, 256, (len(recs), H, W), dtype=np.uint8)
    got = _run(hostsim, imgs, recs, luts)
    want = _expect(imgs, recs, luts)
    bad = [i for i in range(len(recs)) if not np.array_equal(got[i], want[i])]
    assert not bad, [recs[i][:27].tolist() for i in bad[:3]]
    changed = sum(not np.array_equal(R.augment(im, r, luts), im) for im, r in zip(imgs, recs))
    assert changed >= len(recs) // 2                      # the cases move pixels


@pytest.mark.parametrize("task", ["shapenet_1d", "pascal_1d"])
@pytest.mark.parametrize("H,W", SIZES)
def test_hostsim_whole_sequences_bit_exact(hostsim, task, H, W):
    from mlhot.synth import shape_images
    s = A.Sampler(task, seed=11)
    n_ctx, n_qry = 24, 30
    t = s.batch(n_ctx, n_qry, H, W)
    imgs = shape_images(n_ctx + n_qry, H, W, seed=H + W)
    got = _run(hostsim, imgs, t.records, t.luts)
    assert np.array_equal(got, _expect(imgs, t.records, t.luts))
    assert not np.array_equal(got, imgs.astype(np.float32) / np.float32(255.0))


def test_hostsim_all_off_is_the_plain_ingest(hostsim):
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, (6, 37, 41), dtype=np.uint8)
    recs = A.Sampler("pascal_1d", seed=1).batch(3, 3, 37, 41).records.copy()
    recs[:, A.F_ON] = 0
    got = _run(hostsim, imgs, recs)
    plain = hostsim.ingest_u8_nhwc(torch.from_numpy(imgs[..., None])).numpy()[:, 0]
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


def test_hostsim_refuses_multichannel(hostsim):
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError):
        hostsim.augment_ingest_u8(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 32, dtype=torch.int32))


# ---- trainer refusals -----------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    base = dict(device=torch.device("cpu"), seed=1, task="shapenet_1d", aug_list=["data_aug", "task_aug"], device_augment=True,
                iterations=1, save_path="/nonexistent")
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_trainer_refuses_a_loader_that_still_augments():
    from trainer.model_trainer import ModelTrainer
    with pytest.raises(ValueError, match="augmented twice"):
        ModelTrainer(None, None, None, _cfg(), types.SimpleNamespace(data_aug=True))


def test_trainer_refuses_tasks_without_a_device_sequence():
    from trainer.model_trainer import ModelTrainer
    with pytest.raises(NotImplementedError):
        ModelTrainer(None, None, None, _cfg(task="shapenet_3d"), types.SimpleNamespace(data_aug=False))


def test_device_augment_off_is_not_checked():
    assert A.check_trainer_config(_cfg(device_augment=False), types.SimpleNamespace(data_aug=True)) is None
    assert A.check_trainer_config(_cfg(aug_list=["task_aug"]), types.SimpleNamespace(data_aug=True)) is None
    assert isinstance(A.check_trainer_config(_cfg(), types.SimpleNamespace(data_aug=False)), A.Sampler)
