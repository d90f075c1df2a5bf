"""predict(attention_mass=True) and prune of both model families on the MI355X, at the small sizes of the read-out's
model tests: one ResNet ANP and one vanilla ANP, states of form "keys", "long" and "paged".  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import attention_mass_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64)
MODEL_CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention")),
    "anp_shapenet1d": ("ANPShapeNet1D", dict(CFG1D, task="shapenet_1d", input_dim=3, output_dim=2, agg_mode="attention", dim_r=64)),
}
NQ = 37                         # three tiles, the last of 5 rows
FORMS = [("keys", 5, (2, 5)), ("long", 40, (5, 3)), ("paged", 300, (4, 5))]          # form, capacity, ctx_len of the 5 conditioned slots


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=2, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _images(case, n, seed):
    cfg = MODEL_CASES[case][1]
    g = torch.Generator().manual_seed(seed)
    Hh, W, Cc = cfg["img_size"]
    Cc = Cc - 1 if cfg["task"] == "shapenet_3d" else Cc
    return torch.rand(2, n, Cc, Hh, W, generator=g).to(DEV), torch.rand(2, n, cfg["input_dim"], generator=g).to(DEV)


def _plain(model, state, qx, **kw):
    """predict without the keyword on the route the read-out runs: the vanilla family's composed route, ResNetNP's only one"""
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    return cached.predict(model, state, qx, **kw) if isinstance(model, ResNetNP) else cached.predict(model, state, qx, route="composed", **kw)


def _state(case, form, cap, lens):
    from mlhot import cached
    cx, cy = _images(case, 5, 21)
    return cached.condition(_model(case), cx, cy, ctx_len=list(lens), capacity=cap, form=form)


@pytest.mark.parametrize("form,cap,lens", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_predict_returns_the_mass_beside_an_unchanged_mu(gpulib, case, form, cap, lens):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model, state = _model(case), _state(case, form, cap, lens)
    qx = _images(case, NQ, 22)[0]
    mu, mass = cached.predict(model, state, qx, attention_mass=True)
    heads = state.kh.shape[2]
    assert mass.shape == (2, heads, cap) and mass.dtype == torch.float32
    assert torch.equal(mu, _plain(model, state, qx))
    amu, attn = cached.predict(model, state, qx, return_attention=True)
    assert torch.equal(amu, mu) and torch.equal(mass.cpu(), MR.fold32(attn))
    if isinstance(model, ResNetNP):
        mu2, mass2 = model.predict(state, qx, attention_mass=True)
        assert torch.equal(mu2, mu) and torch.equal(mass2, mass)
    else:
        assert state.route == "composed"
    # rows of w sum to 1: the mass over the valid slots sums to Nq; the slots behind ctx_len are exact zeros
    for t, L in enumerate(lens):
        assert bool((mass[t, :, L:] == 0.0).all()) and float(mass[t, :, :L].min()) > 0.0
        assert float((mass[t, :, :L].double().sum(dim=-1) - NQ).abs().max()) <= NQ * cap * 2.0 ** -23
    # chunked: one fold behind the last chunk, the same bits for every multiple of 16
    for chunk in (16, 32):
        cmu, cmass = cached.predict(model, state, qx, chunk=chunk, attention_mass=True)
        assert torch.equal(cmu, _plain(model, state, qx, chunk=chunk)) and torch.equal(cmass, mass), chunk
    # weighted: the documented order on the read-out's weights; a target of weight 0 adds nothing
    g = torch.Generator().manual_seed(23)
    tw = torch.rand(2, NQ, generator=g)
    tw[:, 20:] = 0.0
    wmu, wmass = cached.predict(model, state, qx, attention_mass=True, target_weight=tw)
    assert torch.equal(wmu, mu) and torch.equal(wmass.cpu(), MR.fold32(attn, tw))
    head = cached.predict(model, state, qx[:, :20], attention_mass=True, target_weight=tw[:, :20].to(DEV))[1]
    assert torch.equal(head, wmass)


@pytest.mark.parametrize("form,cap", [("keys", 12), ("long", 40), ("paged", 300)])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_prune_is_evict_with_the_drop_lists_it_reports(gpulib, case, form, cap):
    """The context holds the target images themselves in slots 1, 4 and 7 of its 9 shots.  Whatever the model's weights make of
    them, the kept slots are the keep[t] largest head-summed masses: wherever the gap between the last kept and the first dropped
    score is above the rounding of the sum over heads and targets, the choice is the float64 ranking's."""
    from mlhot import cached
    from mlhot.context import prune_choice
    model = _model(case)
    cx, cy = _images(case, 9, 31)
    qx = cx[:, [1, 4, 7]].contiguous()
    lens, keep = (9, 6), (3, 4)
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap, form=form)
    mass = cached.predict(model, state, qx, attention_mass=True)[1]
    pruned, drop = cached.prune(model, state, qx, keep)
    score = mass[:, 0]
    for h in range(1, mass.shape[1]):
        score = score + mass[:, h]
    assert drop == prune_choice(score.cpu(), lens, keep) == MR.prune_by_hand(score.cpu().tolist(), lens, list(keep))
    assert [len(d) for d in drop] == [6, 2] and pruned.lens == (3, 4) and pruned.capacity == cap and pruned.form == form
    s64 = mass.double().sum(dim=1).cpu()
    for t in range(2):
        kept = [c for c in range(lens[t]) if c not in drop[t]]
        gap = min(float(s64[t, c]) for c in kept) - max(float(s64[t, c]) for c in drop[t])
        print(f"prune {case} {form} task {t}: kept {kept}, dropped {drop[t]}, gap {gap:.3e} of scores around {float(s64[t, :lens[t]].mean()):.3e}")
        if gap > 16 * 2.0 ** -24 * float(s64[t, :lens[t]].max()):
            assert set(kept) == set(sorted(range(lens[t]), key=lambda c: -float(s64[t, c]))[:keep[t]])
    want = cached.evict(model, state, drop)
    for name in ("kh", "vh"):
        assert torch.equal(getattr(pruned, name), getattr(want, name)), name
    # F_k and M: the buffer's tail behind them is the key launches' scratch, padded with whatever the allocation held
    assert all(torch.equal(a, b) for a, b in zip(pruned.keys.features(), want.keys.features())) and pruned.keys.lens == want.keys.lens
    assert torch.equal(cached.predict(model, pruned, qx), cached.predict(model, want, qx))
    # keep >= lens: nothing goes, the state is evict's with empty lists
    same, none = cached.prune(model, state, qx, 9)
    assert none == [[], []] and same.lens == lens
    assert all(torch.equal(a, b) for a, b in zip(same.keys.features(), cached.evict(model, state, [[], []]).keys.features()))
    # the old state stays valid
    assert torch.equal(cached.predict(model, state, qx, attention_mass=True)[1], mass)
