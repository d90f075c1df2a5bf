"""The resident grey pool without a GPU: the three mlhot_pool1_* entries in the host build against the existing
references (tests/augment_ref.py, tests/augment_img_ref.py) applied to pool[ids] gathered with numpy - bit for bit - and the refusals of
ResidentPool, stage_ids' batch check and the trainer's switch; the synthetic loader's twin property."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_img_ref as RI
from tests import augment_ref as R

SHAPES = [(128, 128), (16, 16), (4, 4), (7, 5), (1, 1)]
N_POOL = 6
IDS = np.array([N_POOL - 1, 2, 2, 0, 4], dtype=np.int32)                      # n = 5: ids N - 1 and 0, one id twice, unsorted


def grey_pool(H, W, n=N_POOL, seed=0):
    """uint8 [n, H, W, 1]: structured images (something for the spatial steps to move) with noise on every second one."""
    from mlhot.synth import shape_images
    rng = np.random.default_rng(seed + 1000 * H + W)
    pool = shape_images(n, H, W, seed=seed + H)[..., None].copy()
    pool[::2] = rng.integers(0, 256, pool[::2].shape, dtype=np.uint8)
    return pool


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def to_float(img, div=255.0):
    """fp32 [n, 1, H, W] = byte / div of uint8 [n, H, W, 1]: the loaders' `astype(float32) / 255.0` and the permute."""
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(div)).transpose(0, 3, 1, 2))


def _t(a, device):
    return None if a is None or len(a) == 0 else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run_plain(lib, pool, ids, device="cpu", div=255.0):
    return lib.pool1_ingest_u8(_t(pool, device), _t(ids, device), div=div).cpu().numpy()


def run_aug(lib, pool, ids, t, device="cpu"):
    return lib.pool1_augment_ingest_u8(_t(pool, device), _t(ids, device), _t(t.records, device), _t(t.luts, device)).cpu().numpy()


def run_aug_img(lib, pool, ids, t, device="cpu"):
    return lib.pool1_augment_ingest_u8_img(_t(pool, device), _t(ids, device), _t(t.records, device), _t(t.luts, device),
                                           _t(A.colour_tables(), device), pre_op=t.pre_op, div=t.div, div2=t.div2).cpu().numpy()


def want_aug(pool, ids, t):
    """tests/augment_ref.py on the gathered images, then the ingest's divide."""
    return to_float(R.augment_batch(pool[ids][..., 0], t.records, t.luts)[..., None])


def want_aug_img(pool, ids, t):
    return RI.augment_batch(pool[ids], t.records, t.luts, t.pre_op, t.div, t.div2)


def tables(H, W, n_ctx=2, n_qry=3, seed=11):
    """One whole drawn sequence per image: shapenet_1d's and pascal_1d's (AugTable), Distractor's (ImageAugTable: pre_op 1, two divisions)."""
    return (A.Sampler("shapenet_1d", seed=seed).batch(n_ctx, n_qry, H, W), A.Sampler("pascal_1d", seed=seed + 1).batch(n_ctx, n_qry, H, W),
            A.ImageSampler("distractor", seed=seed + 2).batch(n_ctx, n_qry, H, W))


def all_off(t):
    out = types.SimpleNamespace(records=t.records.copy(), luts=t.luts[:0], pre_op=getattr(t, "pre_op", 0), div=getattr(t, "div", 255.0),
                                div2=getattr(t, "div2", 1.0))
    out.records[:, A.F_ON] = 0
    return out


# ---- the entries in the host build --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_hostsim_plain_entry_is_the_byte_ingest_of_the_gathered_images(hostsim, H, W):
    pool = grey_pool(H, W)
    got = run_plain(hostsim, pool, IDS)
    assert got.shape == (5, 1, H, W) and same_bits(got, to_float(pool[IDS]))
    assert same_bits(got, hostsim.ingest_u8_nhwc(torch.from_numpy(np.ascontiguousarray(pool[IDS]))).numpy())
    assert same_bits(run_plain(hostsim, pool, IDS, div=3.0), to_float(pool[IDS], 3.0))
    arange = np.arange(N_POOL, dtype=np.int32)
    assert same_bits(run_plain(hostsim, pool, arange), hostsim.ingest_u8_nhwc(torch.from_numpy(pool)).numpy())


@pytest.mark.parametrize("H,W", SHAPES)
def test_hostsim_1d_sequences_bit_exact(hostsim, H, W):
    pool = grey_pool(H, W)
    for t in tables(H, W)[:2]:
        got = run_aug(hostsim, pool, IDS, t)
        assert same_bits(got, want_aug(pool, IDS, t))
        packed = hostsim.augment_ingest_u8(torch.from_numpy(np.ascontiguousarray(pool[IDS])), torch.from_numpy(t.records), _t(t.luts, "cpu")).numpy()
        assert same_bits(got, packed)                                            # the byte entry on pool[ids]: the contract itself
        assert same_bits(run_aug(hostsim, pool, IDS, all_off(t)), run_plain(hostsim, pool, IDS))
    if H >= 16:
        assert not same_bits(run_aug(hostsim, pool, IDS, tables(H, W)[0]), run_plain(hostsim, pool, IDS))


@pytest.mark.parametrize("H,W", SHAPES)
def test_hostsim_distractor_sequences_bit_exact(hostsim, H, W):
    pool = grey_pool(H, W)
    t = tables(H, W)[2]
    assert (t.pre_op, t.div, t.div2) == (1, 255.0, 255.0)                          # Distractor's quirks travel unchanged
    got = run_aug_img(hostsim, pool, IDS, t)
    assert same_bits(got, want_aug_img(pool, IDS, t))
    packed = hostsim.augment_ingest_u8_img(torch.from_numpy(np.ascontiguousarray(pool[IDS])), torch.from_numpy(t.records), _t(t.luts, "cpu"),
                                           torch.from_numpy(A.colour_tables()), pre_op=t.pre_op, div=t.div, div2=t.div2).numpy()
    assert same_bits(got, packed)
    off = all_off(t)
    off.pre_op, off.div2 = 0, 1.0
    assert same_bits(run_aug_img(hostsim, pool, IDS, off), run_plain(hostsim, pool, IDS))


def test_hostsim_empty_batches_return_ok(hostsim):
    pool, none = torch.from_numpy(grey_pool(4, 4)), torch.zeros(0, dtype=torch.int32)
    assert hostsim.pool1_ingest_u8(pool, none).shape == (0, 1, 4, 4)
    assert hostsim.pool1_augment_ingest_u8(pool, none, torch.zeros(0, 32, dtype=torch.int32)).shape == (0, 1, 4, 4)
    assert hostsim.pool1_augment_ingest_u8_img(pool, none, torch.zeros(0, 40, dtype=torch.int32)).shape == (0, 1, 4, 4)


def test_hostsim_entries_refuse_what_they_cannot_do(hostsim):
    from mlhot.binding import MlhotError
    ids = torch.zeros(2, dtype=torch.int32)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)                    # noqa: E731
    r32, r40 = torch.zeros(2, 32, dtype=torch.int32), torch.zeros(2, 40, dtype=torch.int32)
    with pytest.raises(MlhotError, match="single-channel"):
        hostsim.pool1_ingest_u8(u8(3, 8, 8, 4), ids)                               # an RGBA pool
    for shape in ((3, 129, 8, 1), (3, 8, 129, 1)):                                 # outside the augmenting kernels' envelope
        with pytest.raises(MlhotError, match="only"):
            hostsim.pool1_augment_ingest_u8(u8(*shape), ids, r32)
        with pytest.raises(MlhotError, match="only"):
            hostsim.pool1_augment_ingest_u8_img(u8(*shape), ids, r40)
        assert hostsim.pool1_ingest_u8(u8(*shape), ids).shape == (2, 1, *shape[1:3])           # the plain entry takes any H, W
    with pytest.raises(MlhotError, match="records"):
        hostsim.pool1_augment_ingest_u8(u8(3, 8, 8, 1), ids, r40)
    with pytest.raises(MlhotError, match="records"):
        hostsim.pool1_augment_ingest_u8_img(u8(3, 8, 8, 1), ids, r32)
    for bad in ([0, 3], [-1, 0]):
        with pytest.raises(MlhotError, match="out of range"):
            hostsim.pool1_ingest_u8(u8(3, 8, 8, 1), torch.tensor(bad, dtype=torch.int32))


# ---- ResidentPool / stage_ids -------------------------------------------------------------------------------------------------------
def test_grey_pool_and_batch_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ingest import ResidentPool, check_grey_batch, check_pool_indices
    pool = grey_pool(8, 8)
    with pytest.raises(MlhotError, match="no background bank"):
        ResidentPool(pool, np.zeros((2, 8, 8, 3), dtype=np.uint8), device="cpu")   # a bank with a grey pool (refused before the device is)
    t1, _, ti = tables(8, 8)
    assert check_grey_batch(5, None, None).name == "pool1" and check_grey_batch(5, None, t1).name == "pool1aug" and check_grey_batch(5, None, ti).name == "pool1augimg"
    with pytest.raises(MlhotError, match="bg must be None"):
        check_grey_batch(5, np.full(5, -1), None)                                  # bg given
    with pytest.raises(MlhotError, match="AugTable"):
        check_grey_batch(5, None, t1.records)                                      # wrong table kind: bare records
    with pytest.raises(MlhotError, match=r"\[n, 40\]"):
        check_grey_batch(5, None, A.ImageAugTable(t1.records, t1.luts, A.ImageAugmentSpec.for_task("distractor")))   # 128-byte records in an image table
    with pytest.raises(MlhotError, match="6 images"):
        check_grey_batch(6, None, t1)                                              # record count mismatch
    with pytest.raises(MlhotError, match="out of range"):
        check_pool_indices(np.array([0, N_POOL]), np.full(2, -1), N_POOL, 0)       # id out of range (what stage_ids runs before it ships)


def _cfg(**kw):
    base = dict(device=torch.device("cpu"), seed=1, task="shapenet_1d", iterations=1, save_path="/nonexistent", resident_pool=True,
                bg_gen_freq=2, gen_bg=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("task", ["shapenet_1d", "pascal_1d", "distractor"])
def test_trainer_switch_serves_the_grey_tasks(task):
    speaks = dict(grey_pool=lambda source: None, get_batch_ids=lambda **k: None)
    assert A.check_trainer_config_pool(_cfg(task=task), types.SimpleNamespace(data_aug=False, **speaks)) is True
    assert A.check_trainer_config_pool(_cfg(task=task, resident_pool=False), types.SimpleNamespace()) is False
    with pytest.raises(ValueError, match="still augments"):
        A.check_trainer_config_pool(_cfg(task=task), types.SimpleNamespace(data_aug=True, **speaks))
    rgba_only = types.SimpleNamespace(data_aug=False, rgba_pool=lambda source: None, get_batch_ids=lambda **k: None)
    with pytest.raises(ValueError, match=r"rgba_pool.*'shapenet_3d' only.*needs grey_pool"):
        A.check_trainer_config_pool(_cfg(task=task), rgba_only)
    with pytest.raises(ValueError, match="grey_pool"):
        A.check_trainer_config_pool(_cfg(task=task), types.SimpleNamespace(data_aug=False, grey_pool=lambda source: None))       # no get_batch_ids
    with pytest.raises(ValueError, match="no resident route"):
        A.check_trainer_config_pool(_cfg(task="something_else"), types.SimpleNamespace(data_aug=False, **speaks))


# ---- the synthetic loader -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,L", [("shapenet_1d", 3), ("pascal_1d", 1), ("distractor", 2)])
def test_synthetic_loader_twin_property(task, L):
    """Same generator state: get_batch_u8 returns grey_pool()[ids] and the labels of get_batch_ids - what the trainer test rests on."""
    from mlhot.synth import SyntheticGreyPool, shape_images
    a, b = SyntheticGreyPool(task, seed=5, pool=20, H=16, W=16), SyntheticGreyPool(task, seed=5, pool=20, H=16, W=16)
    pool = a.grey_pool("train")
    assert pool.shape == (20, 16, 16, 1) and pool.dtype == np.uint8 and np.array_equal(pool, b.grey_pool("train"))
    stored = shape_images(20, 16, 16, seed=5)[..., None]
    assert np.array_equal(pool, 255 - stored if task == "distractor" else stored)          # Distractor: handed over inverted, once
    sizes = set()
    for source in ("train", "train", "train", "validation", "test", "train"):
        ci, qi, ys, yq = a.get_batch_ids(source, 3, 6)
        xs, xq, ys2, yq2 = b.get_batch_u8(source, 3, 6)
        assert ci.dtype == qi.dtype == np.int32 and qi.shape == (3, 6) and ci.shape[0] == 3 and 0 <= min(ci.min(), qi.min()) and max(ci.max(), qi.max()) < 20
        assert ys.shape == (*ci.shape, L) and yq.shape == (3, 6, L)
        assert np.array_equal(xs, pool[ci]) and np.array_equal(xq, pool[qi]) and xs.shape == (*ci.shape, 16, 16, 1)
        assert torch.equal(ys, ys2) and torch.equal(yq, yq2)
        sizes.add(ci.shape[1]) if source == "train" else None
        assert source == "train" or ci.shape[1] == 6
    assert all(3 <= s <= 6 for s in sizes)
