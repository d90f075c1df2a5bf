"""Device augmentation of the image tasks (shapenet_3d, distractor) without a GPU: the oracle (tests/augment_img_ref.py) against its
own properties, the loaders' byte handling, the host sampler (mlhot.augment.ImageSampler), the kernel's functors in the host build
against the oracle bit for bit, and the refusals."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_img_ref as RI
from tests import augment_ref as R


def record(op=None, **f):
    """A 40-int record with one step (or none) switched on; fields by mlhot.augment.F_* name suffix."""
    rec = np.zeros(A.IMG_RECORD_INTS, dtype=np.int32)
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


def rgb(H, W, seed=0, n=None):
    shape = (H, W, 3) if n is None else (n, H, W, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- oracle properties -----------------------------------------------------------------------------------------------------------
def test_oracle_all_off_is_the_identity():
    from mlhot.synth import colour_images
    for img in (rgb(17, 31), colour_images(1, 64, 64)[0]):
        assert np.array_equal(RI.augment(img, record()), img)
        rec = A.ImageSampler("shapenet_3d", seed=1).batch(1, 1, *img.shape[:2]).records[0].copy()
        rec[A.F_ON] = 0
        assert np.array_equal(RI.augment(img, rec), img)


def test_oracle_single_channel_equals_the_1d_oracle():
    t = A.ImageSampler("shapenet_3d", seed=4).batch(40, 0, 37, 53)
    imgs = np.random.default_rng(2).integers(0, 256, (40, 37, 53), dtype=np.uint8)
    recs = t.records.copy()
    recs[:, A.F_ON] &= ~(1 << A.BRIGHTNESS)                     # the shared ops: everything but AddToBrightness
    for im, rec in zip(imgs, recs):
        assert np.array_equal(RI.augment(im[..., None], rec, t.luts)[..., 0], R.augment(im, rec[:32], t.luts))
    assert any(not np.array_equal(R.augment(im, rec[:32], t.luts), im) for im, rec in zip(imgs, recs))
    one = record(A.BRIGHTNESS, bright_add=-20, bright_space=A.LAB)
    assert np.array_equal(RI.augment(imgs[0][..., None], one)[..., 0], np.clip(imgs[0].astype(int) - 20, 0, 255))


@pytest.mark.parametrize("op,f", [(A.DROPOUT, dict(drop_thresh=1 << 31)), (A.COARSE_DROPOUT, dict(coarse_thresh=1 << 31, coarse_h=7, coarse_w=9))])
def test_oracle_per_channel_masks(op, f):
    img = np.full((32, 40, 3), 200, dtype=np.uint8)
    flag = "drop_per_channel" if op == A.DROPOUT else "coarse_per_channel"
    same = RI.augment(img, record(op, seed=5, image=3, **f, **{flag: 0})) == 0
    own = RI.augment(img, record(op, seed=5, image=3, **f, **{flag: 1})) == 0
    assert np.array_equal(same[..., 0], same[..., 1]) and np.array_equal(same[..., 1], same[..., 2]) and 0.3 < same.mean() < 0.7
    assert not np.array_equal(own[..., 0], own[..., 1]) and not np.array_equal(own[..., 1], own[..., 2])
    assert np.array_equal(own[..., 0], same[..., 0])             # channel 0's items are the shared mask's
    one = img[..., :1]
    assert np.array_equal(RI.augment(one, record(op, seed=5, image=3, **f, **{flag: 1})), RI.augment(one, record(op, seed=5, image=3, **f)))


@pytest.mark.parametrize("space", range(6))
def test_oracle_brightness_grey_and_monotone(space):
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    img = rgb(48, 48, seed=7)
    means = []
    for a in range(-30, 31, 3):
        out = RI.brightness(grey, a, space)
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 1], out[..., 2]), a
        if space in (A.YCRCB, A.YUV, A.HSV, A.HLS):
            assert np.array_equal(out[..., 0], np.clip(grey[..., 0].astype(int) + a, 0, 255)), a
        means.append(RI.brightness(img, a, space).astype(np.float64).mean())
    assert all(b >= a for a, b in zip(means, means[1:])) and means[-1] > means[0]


# max |out - in| per space over the fixed sample below with add = 0: how lossy each 8-bit round trip of the spec is.
# YUV's V = 0.877 (R - Y) and YCrCb's Cr leave the byte range for saturated colours and are clipped, as cv2's 8-bit forms are.
ROUND_TRIP = {A.YCRCB: 1, A.HSV: 4, A.HLS: 5, A.LAB: 18, A.LUV: 16, A.YUV: 28}


@pytest.mark.parametrize("space", range(6))
def test_oracle_round_trip_deviation_is_the_recorded_one(space):
    px = np.random.default_rng(0).integers(0, 256, (64, 64, 3), dtype=np.uint8)          # 4096 pixels
    dev = int(np.abs(RI.brightness(px, 0, space).astype(int) - px.astype(int)).max())
    print(RI.SPACES[space], "round trip max deviation", dev)
    assert dev == ROUND_TRIP[space]


def test_oracle_pad_modes_are_np_pad_over_hwc():
    img = rgb(9, 7, seed=3)
    img[0, :, 1] = 200                                          # an edge equal to the end value in ONE channel: linear_ramp's zero step
    kw = {0: {"constant_values": 200}, 2: {"end_values": 200}}
    for mode, name in enumerate(R.PAD_MODES):
        got = RI.pad(img, 1, 3, 2, 4, mode, 200)
        assert np.array_equal(got, np.pad(img, ((1, 2), (4, 3), (0, 0)), mode=name, **kw.get(mode, {}))), name
        assert got.shape == (12, 14, 3) and np.array_equal(got[1:10, 4:11], img)


def test_colour_tables_agree_with_the_oracles():
    blob, t = A.colour_tables(), RI.tables()
    head = blob[:96].view(np.int32)
    assert np.array_equal(head[:9], t["m"].ravel()) and np.array_equal(head[9:18], t["minv"].ravel())
    assert head[18:23].tolist() == [t["xn"], t["zn"], t["un"], t["vn"], t["wz"]]
    assert t["m"].sum(axis=1).tolist() == [4096] * 3 and t["minv"].sum(axis=1).tolist() == [4096] * 3
    assert np.array_equal(blob[96:608].view(np.uint16), t["lin"])
    assert np.array_equal(blob[608:8800].view(np.uint16)[:RI.Q + 1], t["f"]) and np.array_equal(blob[8800:][:RI.Q + 1], t["s8"])
    assert blob.size == 12896


# ---- loader byte handling -----------------------------------------------------------------------------------------------------------
def test_byte_handling_of_the_two_loaders():
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(RI.pre_op(k, 0), (k.astype(np.float32) / 255 * 255).astype(np.uint8))      # shapenet_3d: fp32 k / 255
    assert np.array_equal(RI.pre_op(k, 1), k * 255)                                                   # distractor: uint8 wraps
    assert (k * 255).dtype == np.uint8
    got = RI.to_float(k.reshape(1, 16, 16, 1), 255.0, 255.0)
    want = ((k / 255.0).astype(np.float32) / 255.0).astype(np.float32).reshape(1, 1, 16, 16)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for task, want in (("shapenet_3d", (0, 255.0, 1.0)), ("distractor", (1, 255.0, 255.0))):
        s = A.ImageAugmentSpec.for_task(task)
        assert (s.pre_op, s.div, s.div2) == want


# ---- sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,H,C", [("shapenet_3d", 64, 3), ("distractor", 128, 1)])
def test_image_sampler_rates_and_ranges(task, H, C):
    """n = 4000: a rate p has sigma = sqrt(p (1 - p) / n) <= 0.008; every bound below is five sigma of its own p."""
    n = 4000
    rec, luts = A.ImageSampler(task, seed=3).side(n, H, H, side=1)
    steps = A.ImageAugmentSpec.for_task(task).steps
    assert rec.shape == (n, 40) and (rec[:, A.F_N_STEPS] == len(steps)).all()
    ops = rec[:, A.F_OP:A.F_OP + len(steps)]
    assert len({tuple(r) for r in ops}) <= 2                               # one permutation per call (up to the OneOf member)
    on = rec[:, A.F_ON]
    for code in set(steps) - {A.ONEOF}:
        assert abs(((on >> code) & 1).mean() - 0.5) < 0.04, code
    assert abs((ops == A.COARSE_DROPOUT).any(axis=1).mean() - 0.5) < 0.04
    assert abs((((on >> A.DROPOUT) & 1) | ((on >> A.COARSE_DROPOUT) & 1)).mean() - 0.5) < 0.04
    assert rec[:, A.F_BRIGHT_ADD].min() == -30 and rec[:, A.F_BRIGHT_ADD].max() == 30
    assert abs(rec[:, A.F_BRIGHT_ADD].mean()) < 5 * 17.6 / np.sqrt(n)       # uniform on 61 integers: sigma 17.6
    for space in range(6):
        assert abs((rec[:, A.F_BRIGHT_SPACE] == space).mean() - 1 / 6) < 0.03, space
    assert set(np.unique(rec[:, A.F_DROP_PER_CHANNEL])) == {0, 1} and abs(rec[:, A.F_DROP_PER_CHANNEL].mean() - 0.5) < 0.04
    assert set(np.unique(rec[:, A.F_COARSE_PER_CHANNEL])) == {0, 1} and abs(rec[:, A.F_COARSE_PER_CHANNEL].mean() - 0.2) < 0.032
    pad = rec[:, A.F_PAD:A.F_PAD + 4]
    assert pad.min() == 0 and pad.max() == round(0.05 * H)
    assert set(np.unique(rec[:, A.F_PAD_MODE])) == set(range(10)) and set(np.unique(rec[:, A.F_BLUR_K])) == {1, 2, 3}
    assert set(np.unique(rec[:, A.F_AFF_ORDER])) == {0, 1} and set(np.unique(rec[:, A.F_AFF_MODE])) == set(range(5))
    sx = 65536.0 / rec[:, A.F_AFF_AX]
    assert sx.min() >= 0.8 - 1e-4 and sx.max() <= 1.2 + 1e-4
    u = rec.view(np.uint32)
    assert (u[:, A.F_DROP_THRESH] / 2.0 ** 32).max() <= 0.1 and (u[:, A.F_COARSE_THRESH] / 2.0 ** 32).max() <= 0.05
    assert (rec[:, A.F_IMAGE] == np.arange(n)).all() and (u[:, A.F_SIDE] == 1).all() and (rec[:, 36:] == 0).all()
    if A.GAMMA in steps:
        g_on = (on >> A.GAMMA) & 1 == 1
        assert luts.shape == (g_on.sum(), 256) and (rec[g_on, A.F_LUT] == np.arange(g_on.sum())).all()
    else:
        assert luts.shape == (0, 256) and not ((on >> A.BRIGHTNESS) & 1).any()


def test_image_sampler_determinism_ranks_and_global_rng():
    state = np.random.get_state()
    a = A.ImageSampler("shapenet_3d", seed=5, rank=0).batch(30, 40, 64, 64)
    b = A.ImageSampler("shapenet_3d", seed=5, rank=0).batch(30, 40, 64, 64)
    c = A.ImageSampler("shapenet_3d", seed=5, rank=1).batch(30, 40, 64, 64)
    after = np.random.get_state()
    assert np.array_equal(a.records, b.records) and np.array_equal(a.luts, b.luts) and not np.array_equal(a.records, c.records)
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert isinstance(a, A.ImageAugTable) and a.n_img == 70 and (a.pre_op, a.div, a.div2) == (0, 255.0, 1.0)
    u = a.records.view(np.uint32)
    assert (u[:30, A.F_SIDE] == 0).all() and (u[30:, A.F_SIDE] == 1).all()


# ---- the kernel's functors (host build) against the oracle -------------------------------------------------------------------------
def run_lib(lib, imgs, records, luts=None, pre_op=0, div=255.0, div2=1.0, device="cpu"):
    ct = torch.from_numpy(A.colour_tables()).to(device)
    out = lib.augment_ingest_u8_img(torch.from_numpy(np.ascontiguousarray(imgs)).to(device), torch.from_numpy(np.ascontiguousarray(records)).to(device),
                                    None if luts is None or len(luts) == 0 else torch.from_numpy(np.ascontiguousarray(luts)).to(device), ct,
                                    pre_op=pre_op, div=div, div2=div2)
    return out.cpu().numpy()


def isolated_records(H, W, C, rng):
    """Every op alone: every pad mode, every affine mode and order, k in {1, 2, 3}, every colour space with add in {-30, -7, 0, 30},
    both per_channel settings."""
    recs, top = [], 3 if C == 3 else 6
    for mode in range(A.N_PAD_MODES):
        for pad in ([1, 2, 3, 0], [top] * 4, [0, 0, 2, 0], [int(x) for x in rng.integers(0, top + 1, 4)]):
            recs.append(record(A.CROP_PAD, pad=pad, pad_mode=mode, pad_cval=int(rng.integers(0, 256))))
    for mode in range(A.N_AFFINE_MODES):
        for order in (0, 1):
            sx, sy, tx, ty = rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
            ax, bx, ay, by = (int(v[0]) for v in A.affine_fixed(np.array([sx]), np.array([sy]), np.array([tx]), np.array([ty]), H, W))
            recs.append(record(A.AFFINE, aff_order=order, aff_mode=mode, aff_cval=int(rng.integers(0, 256)), aff_ax=ax, aff_bx=bx,
                               aff_ay=ay, aff_by=by))
    for k in (1, 2, 3):
        recs.append(record(A.BLUR, blur_k=k))
    recs += [record(A.GAMMA, lut=0), record(A.GAMMA, lut=1)]
    for space in range(6):
        for add in (-30, -7, 0, 30):
            recs.append(record(A.BRIGHTNESS, bright_add=add, bright_space=space))
    for pc in (0, 1):
        for p in (0.01, 0.1, 0.5):
            recs.append(record(A.DROPOUT, drop_thresh=int(p * 2 ** 32), drop_per_channel=pc, seed=7, counter=3, side=1, image=len(recs)))
        for p, ch, cw in ((0.05, 3, 3), (0.5, 7, 16), (0.3, 16, 5)):
            recs.append(record(A.COARSE_DROPOUT, coarse_thresh=int(p * 2 ** 32), coarse_h=ch, coarse_w=cw, coarse_per_channel=pc, seed=9,
                               image=len(recs)))
    return np.stack(recs)


def isolated_case(H, W, C, seed):
    from mlhot.synth import colour_images
    rng = np.random.default_rng(seed)
    recs = isolated_records(H, W, C, rng)
    imgs = rng.integers(0, 256, (len(recs), H, W, C), dtype=np.uint8)
    if C == 3:
        imgs[::3] = colour_images(len(imgs[::3]), H, W, seed=seed)          # structured and grey images among the noise
    return imgs, recs, A.gamma_luts([0.5, 1.7])


SIZES = [(64, 64, 3), (37, 53, 3), (3, 5, 3), (128, 128, 1), (61, 128, 1)]


@pytest.mark.parametrize("H,W,C", SIZES)
def test_hostsim_each_op_alone_bit_exact(hostsim, H, W, C):
    imgs, recs, luts = isolated_case(H, W, C, H * 1000 + W)
    got = run_lib(hostsim, imgs, recs, luts)
    want = RI.augment_batch(imgs, recs, luts)
    bad = [i for i in range(len(recs)) if not np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32))]
    assert not bad, [recs[i].tolist() for i in bad[:3]]
    changed = sum(not np.array_equal(RI.augment(im, r, luts), im) for im, r in zip(imgs, recs))
    assert changed >= len(recs) // 2                      # the cases move pixels


def sequence_case(task, H, W, C, n_ctx=6, n_qry=10, seed=11):
    from mlhot.synth import colour_images, shape_images
    t = A.ImageSampler(task, seed=seed).batch(n_ctx, n_qry, H, W)
    n = n_ctx + n_qry
    imgs = colour_images(n, H, W, seed=H + W) if C == 3 else shape_images(n, H, W, seed=H + W)[..., None]
    return imgs, t


@pytest.mark.parametrize("task", ["shapenet_3d", "distractor"])
@pytest.mark.parametrize("H,W,C", SIZES)
def test_hostsim_whole_sequences_bit_exact(hostsim, task, H, W, C):
    imgs, t = sequence_case(task, H, W, C, n_ctx=12, n_qry=20)
    got = run_lib(hostsim, imgs, t.records, t.luts, t.pre_op, t.div, t.div2)
    want = RI.augment_batch(imgs, t.records, t.luts, t.pre_op, t.div, t.div2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, RI.to_float(RI.pre_op(imgs, t.pre_op), t.div, t.div2))


@pytest.mark.parametrize("C", [3, 1])
def test_hostsim_all_off_is_the_plain_ingest(hostsim, C):
    imgs = np.random.default_rng(1).integers(0, 256, (6, 37, 41, C), dtype=np.uint8)
    recs = A.ImageSampler("shapenet_3d", seed=1).batch(3, 3, 37, 41).records.copy()
    recs[:, A.F_ON] = 0
    plain = hostsim.ingest_u8_nhwc(torch.from_numpy(imgs)).numpy()
    assert np.array_equal(run_lib(hostsim, imgs, recs).view(np.uint32), plain.view(np.uint32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_is_unsupported(hostsim):
    from mlhot.binding import MlhotError
    for shape in ((2, 8, 8, 2), (2, 65, 8, 3), (2, 8, 65, 3), (1, 129, 8, 1)):
        with pytest.raises(MlhotError, match="only"):
            hostsim.augment_ingest_u8_img(torch.zeros(shape, dtype=torch.uint8), torch.zeros(shape[0], 40, dtype=torch.int32))
    with pytest.raises(MlhotError):
        hostsim.augment_ingest_u8_img(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 32, dtype=torch.int32))     # the 1D record


def _cfg(**kw):
    base = dict(device=torch.device("cpu"), seed=1, task="shapenet_3d", aug_list=["data_aug", "task_aug"], iterations=1, save_path="/nonexistent")
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_the_three_old_refusals_hold(hostsim):
    from mlhot.binding import MlhotError
    from trainer.model_trainer import ModelTrainer
    for task in ("shapenet_3d", "distractor"):
        with pytest.raises(NotImplementedError):
            A.AugmentSpec.for_task(task)
    with pytest.raises(MlhotError):
        hostsim.augment_ingest_u8(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 32, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        ModelTrainer(None, None, None, _cfg(device_augment=True), types.SimpleNamespace(data_aug=False))


def test_the_new_switch_refuses_a_loader_that_still_augments():
    from trainer.model_trainer import ModelTrainer
    with pytest.raises(ValueError, match="augmented twice"):
        ModelTrainer(None, None, None, _cfg(device_augment_images=True), types.SimpleNamespace(data_aug=True))
    assert A.check_trainer_config_images(_cfg(), types.SimpleNamespace(data_aug=True)) is None                     # absent = off
    assert A.check_trainer_config_images(_cfg(device_augment_images=True, aug_list=["task_aug"]), types.SimpleNamespace(data_aug=True)) is None
    s = A.check_trainer_config_images(_cfg(device_augment_images=True, task="distractor"), types.SimpleNamespace(data_aug=False))
    assert isinstance(s, A.ImageSampler) and s.spec.task == "distractor"
    with pytest.raises(NotImplementedError):
        A.check_trainer_config_images(_cfg(device_augment_images=True, task="shapenet_1d"), types.SimpleNamespace(data_aug=False))
