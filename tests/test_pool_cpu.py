"""The resident image pool without a GPU: the oracle (tests/pool_ref.py) against the reference's float formula, both C entries in the
host build against the oracle bit for bit, the background sampler, and the refusals."""
import types

import numpy as np
import pytest
import torch

from mlhot import augment as A
from tests import augment_img_ref as RI
from tests import pool_ref as PR

SHAPES = [(5, 64, 64), (3, 7, 5), (1, 1, 1)]
ALPHAS = ["all", "none", "mixed"]
N_POOL, N_BANK = 6, 3


def pool_case(n, H, W, alpha, seed=0):
    """(pool uint8 [6, H, W, 4], bank uint8 [3, H, W, 3], ids int32 [n], bg int32 [n]): the same id twice, unsorted ids, the last pool
    image and the last bank image, one image without composition; alpha all 255, none 255, or mixed with 254 right next to 255."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    pool = rng.integers(0, 256, (N_POOL, H, W, 4), dtype=np.uint8)
    if alpha == "all":
        pool[..., 3] = 255
    elif alpha == "none":
        pool[..., 3] = rng.choice(np.array([254, 0, 1, 128, 253], dtype=np.uint8), (N_POOL, H, W))
    else:
        a = rng.choice(np.array([255, 254, 0, 77], dtype=np.uint8), (N_POOL, H, W), p=[0.4, 0.3, 0.15, 0.15])
        flat = a.reshape(N_POOL, -1)
        even, odd = flat[:, 0:flat.shape[1] - 1:2], flat[:, 1::2]                    # pixel pairs: a 255 gets a 254 right behind it
        odd[even == 255] = 254
        pool[..., 3] = a
    bank = rng.integers(0, 256, (N_BANK, H, W, 3), dtype=np.uint8)
    ids = np.array([N_POOL - 1, 2, 2, 0, 4][:n], dtype=np.int32)
    bg = np.array([N_BANK - 1, -1, 0, 1, N_BANK - 1][:n], dtype=np.int32)
    return pool, bank, ids, bg


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run_plain(lib, pool, bank, ids, bg, device="cpu"):
    return lib.pool_ingest_u8(_t(pool, device), _t(ids, device), _t(bank, device), _t(bg, device)).cpu().numpy()


def run_aug(lib, pool, bank, ids, bg, records, luts=None, device="cpu"):
    return lib.pool_augment_ingest_u8_img(_t(pool, device), _t(ids, device), _t(records, device), _t(bank, device), _t(bg, device),
                                          None if luts is None or len(luts) == 0 else _t(luts, device),
                                          _t(A.colour_tables(), device)).cpu().numpy()


def all_off_records(n, H, W):
    recs = A.ImageSampler("shapenet_3d", seed=2).batch(n, 0, H, W).records.copy()
    recs[:, A.F_ON] = 0
    return recs


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
def test_oracle_is_the_reference_formula_on_floats(alpha):
    """rgb * mask + bg * (1 - mask) with mask = alpha < 1.0 on k / 255 floats: a 0/1 mask makes both products and the sum exact, and
    alpha < 1.0 is alpha byte < 255 - so the byte select, divided, has the same bits."""
    pool, bank, ids, bg = pool_case(5, 64, 64, alpha)
    f_pool, f_bank = pool.astype(np.float32) / np.float32(255.0), bank.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(f_pool[..., 3] < 1.0, pool[..., 3] < 255)
    want = PR.reference_formula(f_pool, f_bank, ids, bg)
    assert want.dtype == np.float32
    got = PR.to_float(PR.compose(pool, bank, ids, bg))
    assert same_bits(got, np.ascontiguousarray(want.transpose(0, 3, 1, 2)))
    if alpha != "none":
        assert not np.array_equal(PR.compose(pool, bank, ids, bg), pool[ids][..., :3])


def test_in_place_regeneration_equals_composing_from_the_original():
    """The reference composites in place and cumulatively; a kept pixel never changes and alpha is never written, so epoch 1 then
    epoch 2 in place is epoch 2 from the stored pool."""
    pool, bank, _, _ = pool_case(5, 64, 64, "mixed")
    ids = np.arange(N_POOL)
    images = pool.astype(np.float32) / np.float32(255.0)
    f_bank = bank.astype(np.float32) / np.float32(255.0)
    original = images.copy()
    for epoch in (1, 2):
        bg = PR.bg_indices(7, epoch, ids, N_BANK)
        images[..., :3] = PR.reference_formula(images, f_bank, ids, bg)
    assert np.array_equal(images[..., 3], original[..., 3])
    once = PR.reference_formula(original, f_bank, ids, PR.bg_indices(7, 2, ids, N_BANK))
    assert same_bits(images[..., :3], once)
    assert not np.array_equal(PR.bg_indices(7, 1, ids, N_BANK), PR.bg_indices(7, 2, ids, N_BANK))


# ---- the entries in the host build --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_hostsim_pool_ingest_bit_exact(hostsim, n, H, W, alpha):
    pool, bank, ids, bg = pool_case(n, H, W, alpha)
    assert same_bits(run_plain(hostsim, pool, bank, ids, bg), PR.to_float(PR.compose(pool, bank, ids, bg)))
    none = np.full(n, -1, dtype=np.int32)
    assert same_bits(run_plain(hostsim, pool, bank, ids, none), PR.to_float(pool[ids][..., :3]))
    assert same_bits(run_plain(hostsim, pool, None, ids, None), PR.to_float(pool[ids][..., :3]))          # no bank at all


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_hostsim_without_backgrounds_is_the_plain_ingest(hostsim, n, H, W):
    pool, bank, _, _ = pool_case(n, H, W, "mixed")
    ids = np.arange(N_POOL, dtype=np.int32)
    plain = hostsim.ingest_u8_nhwc(torch.from_numpy(np.ascontiguousarray(pool[..., :3]))).numpy()
    assert same_bits(run_plain(hostsim, pool, bank, ids, np.full(N_POOL, -1, dtype=np.int32)), plain)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_hostsim_all_off_records_give_the_plain_pool_entry(hostsim, n, H, W, alpha):
    pool, bank, ids, bg = pool_case(n, H, W, alpha)
    assert same_bits(run_aug(hostsim, pool, bank, ids, bg, all_off_records(n, H, W)), run_plain(hostsim, pool, bank, ids, bg))


def sequence_case(H, W, n_ctx=6, n_qry=10, seed=11):
    """A structured pool (mlhot.synth.SyntheticViewsRGBA's), n_ctx + n_qry ids with repeats, bg indices of epoch 3, one whole drawn
    shapenet_3d sequence per image."""
    from mlhot.synth import SyntheticViewsRGBA
    data = SyntheticViewsRGBA(seed=seed, objects=2, views=6, bank=4, H=H, W=W)
    pool, bank = data.rgba_pool("train")
    n = n_ctx + n_qry
    ids = np.random.default_rng(seed).integers(0, pool.shape[0], n).astype(np.int32)
    ids[-1] = pool.shape[0] - 1
    bg = PR.bg_indices(seed, 3, ids, bank.shape[0])
    bg[1] = -1
    return pool, bank, ids, bg, A.ImageSampler("shapenet_3d", seed=seed).batch(n_ctx, n_qry, H, W)


@pytest.mark.parametrize("H,W", [(64, 64), (7, 5), (1, 1)])
def test_hostsim_whole_sequences_bit_exact(hostsim, H, W):
    pool, bank, ids, bg, t = sequence_case(H, W)
    got = run_aug(hostsim, pool, bank, ids, bg, t.records, t.luts)
    want = RI.augment_batch(PR.compose(pool, bank, ids, bg), t.records, t.luts, t.pre_op, t.div, t.div2)
    assert same_bits(got, want)
    if H > 1:
        assert not same_bits(got, run_plain(hostsim, pool, bank, ids, bg))


def test_synthetic_pool_has_the_alphas_the_rule_turns_on():
    from mlhot.synth import SyntheticViewsRGBA, SyntheticViewsRGBAHost
    data = SyntheticViewsRGBA(seed=3, objects=2, views=10)
    pool, bank = data.rgba_pool("train")
    a = pool[..., 3]
    assert pool.shape == (20, 64, 64, 4) and bank.shape == (5, 64, 64, 3) and pool.dtype == bank.dtype == np.uint8
    assert (a == 255).any() and (a == 254).any() and (a < 254).any()
    assert ((a[:, :, 1:] == 254) & (a[:, :, :-1] == 255)).any()
    ci, qi, ys, yq = data.get_batch_ids("train", 2, 5)
    assert ci.shape == qi.shape == (2, 5) and ci.dtype == np.int32 and ys.shape == (2, 5, 4) and 0 <= ci.min() and qi.max() < 20
    sampler = A.BackgroundSampler(5, seed=9, bg_gen_freq=2)
    twin = SyntheticViewsRGBAHost(sampler, seed=3, objects=2, views=10)
    xs, xq, ys2, yq2 = twin.get_batch("train", 2, 5)                                   # the same draws, epoch 0: the file's RGB
    assert torch.equal(ys, ys2) and same_bits(xs.numpy().reshape(-1, 3, 64, 64), PR.to_float(pool[ci.reshape(-1)][..., :3]))
    twin.gen_bg(None, data="train")
    ci, qi, _, _ = data.get_batch_ids("train", 2, 5)
    xs, xq, _, _ = twin.get_batch("train", 2, 5)
    want = PR.compose(pool, bank, qi.reshape(-1), PR.bg_indices(9, 1, qi.reshape(-1), 5))
    assert same_bits(xq.numpy().reshape(-1, 3, 64, 64), PR.to_float(want))


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
def test_sampler_is_a_function_of_seed_epoch_and_id():
    state = np.random.get_state()
    s = A.BackgroundSampler(16, seed=2578, bg_gen_freq=500)
    ids = np.array([[5, 9, 5], [0, 31999, 9]])
    a = s.batch(ids, 3)
    assert a.dtype == np.int32 and a.shape == ids.shape and a[0, 0] == a[0, 2] and a[0, 1] == a[1, 2]           # any batch position
    assert np.array_equal(a, PR.bg_indices(2578, 3, ids, 16))
    assert np.array_equal(s.batch(ids[::-1, ::-1], 3), a[::-1, ::-1])
    assert np.array_equal(A.BackgroundSampler(16, seed=2578, bg_gen_freq=7).batch(ids, 3), a)                  # nothing else goes in
    big = np.arange(4000)
    assert not np.array_equal(s.batch(big, 3), s.batch(big, 4)) and not np.array_equal(s.batch(big, 3), A.BackgroundSampler(16, seed=1).batch(big, 3))
    assert (s.batch(ids, 0) == -1).all() and (s.batch(ids, 3, source="validation") == -1).all() and (s.batch(ids, 3, source="test") == -1).all()
    assert [s.epoch(it) for it in (1, 499, 500, 999, 1000)] == [0, 0, 1, 1, 2]
    assert A.BackgroundSampler(16, bg_gen_freq=500, gen_bg=False).epoch(1500) == 0
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


@pytest.mark.parametrize("epoch", [1, 2, 77])
def test_sampler_is_uniform_over_the_bank(epoch):
    """n = 32 000 ids over B = 16: a count is binomial(n, 1/16), sigma = sqrt(n * (1/16) * (15/16)) = 43.3; every count within five."""
    n, B = 32000, 16
    bg = A.BackgroundSampler(B, seed=42).batch(np.arange(n), epoch)
    assert bg.min() == 0 and bg.max() == B - 1
    counts = np.bincount(bg, minlength=B)
    sigma = np.sqrt(n * (1 / B) * (1 - 1 / B))
    print("counts", counts.tolist(), "sigma", sigma)
    assert (np.abs(counts - n / B) <= 5 * sigma).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_wrong_shapes_and_indices_are_refused(hostsim):
    from mlhot.binding import MlhotError
    from mlhot.ingest import check_pool_indices
    ids, rec = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 40, dtype=torch.int32)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)                    # noqa: E731
    with pytest.raises(MlhotError, match="RGBA"):
        hostsim.pool_ingest_u8(u8(3, 8, 8, 3), ids)                                # a pool without alpha
    with pytest.raises(MlhotError, match="bank"):
        hostsim.pool_ingest_u8(u8(3, 8, 8, 4), ids, u8(2, 8, 8, 4))                # a bank with alpha
    with pytest.raises(MlhotError, match="bank"):
        hostsim.pool_ingest_u8(u8(3, 8, 8, 4), ids, u8(2, 8, 4, 3))                # a bank of another geometry
    for shape in ((3, 65, 8, 4), (3, 8, 65, 4)):
        with pytest.raises(MlhotError, match="only"):
            hostsim.pool_augment_ingest_u8_img(u8(*shape), ids, rec)
        assert hostsim.pool_ingest_u8(u8(*shape), ids).shape == (2, 3, *shape[1:3])          # the plain path takes any H, W
    with pytest.raises(MlhotError, match="records"):
        hostsim.pool_augment_ingest_u8_img(u8(3, 8, 8, 4), ids, torch.zeros(2, 32, dtype=torch.int32))
    for bad_ids, bad_bg in (([0, 3], [0, 0]), ([-1, 0], [0, 0]), ([0, 1], [0, 2]), ([0, 1], [-2, 0])):
        with pytest.raises(MlhotError, match="out of range"):
            check_pool_indices(np.array(bad_ids), np.array(bad_bg), 3, 2)
        with pytest.raises(MlhotError, match="out of range"):
            hostsim.pool_ingest_u8(u8(3, 8, 8, 4), torch.tensor(bad_ids, dtype=torch.int32), u8(2, 8, 8, 3), torch.tensor(bad_bg, dtype=torch.int32))
    with pytest.raises(MlhotError, match="out of range"):
        hostsim.pool_ingest_u8(u8(3, 8, 8, 4), ids, None, torch.zeros(2, dtype=torch.int32))         # no bank: every bg must be -1
    check_pool_indices(np.array([[0, 2]]), np.array([[-1, 1]]), 3, 2)


def test_a_float_pool_is_taken_only_when_it_is_exact_bytes(hostsim):
    from mlhot.binding import MlhotError
    from mlhot.ingest import pool_bytes
    pool = np.random.default_rng(0).integers(0, 256, (3, 8, 8, 4), dtype=np.uint8)
    f = pool.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(pool_bytes(f, 4, "the image pool", L=hostsim).numpy(), pool)
    assert pool_bytes(pool, 4, "the image pool", L=hostsim).numpy() is not None
    f[1, 2, 3, 0] = np.nextafter(f[1, 2, 3, 0], np.float32(2.0))
    with pytest.raises(MlhotError, match="not exactly"):
        pool_bytes(f, 4, "the image pool", L=hostsim)
    with pytest.raises(MlhotError, match="channel-last"):
        pool_bytes(pool[..., :3], 4, "the image pool", L=hostsim)


def _cfg(**kw):
    base = dict(device=torch.device("cpu"), seed=1, task="shapenet_3d", iterations=1, save_path="/nonexistent", resident_pool=True,
                bg_gen_freq=2, gen_bg=True)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_the_trainer_refuses_what_the_route_cannot_do():
    from trainer.model_trainer import ModelTrainer
    speaks = dict(rgba_pool=lambda source: None, get_batch_ids=lambda **k: None)
    with pytest.raises(ValueError, match="lacks the protocol"):
        ModelTrainer(None, None, None, _cfg(), types.SimpleNamespace(data_aug=False, get_batch_u8=lambda **k: None))
    with pytest.raises(ValueError, match="still augments"):
        ModelTrainer(None, None, None, _cfg(), types.SimpleNamespace(data_aug=True, **speaks))
    with pytest.raises(ValueError, match="shapenet_3d"):
        ModelTrainer(None, None, None, _cfg(task="distractor"), types.SimpleNamespace(data_aug=False, **speaks))
    assert A.check_trainer_config_pool(_cfg(resident_pool=False), types.SimpleNamespace()) is False
    delattr(cfg := _cfg(), "resident_pool")
    assert A.check_trainer_config_pool(cfg, types.SimpleNamespace()) is False                 # absent = off
    assert A.check_trainer_config_pool(_cfg(), types.SimpleNamespace(data_aug=False, **speaks)) is True
