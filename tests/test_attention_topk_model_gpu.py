"""predict(top_k=) of both model families on the MI355X, at the small sizes of the read-out's model tests: one
ResNet ANP and one vanilla ANP, states of form "keys", "long" and "paged" with ragged ctx_len.  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import attention_topk_ref as TR

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
KS = (1, 3, 16)                 # 16 exceeds every ctx_len here: the padding rule through the model


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


def _consistent(idx, w, attn, lens, cap, k):
    """(idx, w) against the read-out attn [T, heads, Nq, cap] of the same state: shape rules, the gather, torch.topk's values"""
    TR.check_shape_rules(idx, w, lens, cap, k)
    assert torch.equal(w, TR.gather_at(attn, idx))
    for t, n in enumerate(lens):
        j = min(k, n)
        assert torch.equal(w[t, :, :, :j], torch.topk(attn[t, :, :, :n], j, dim=-1).values), t


@pytest.mark.parametrize("form,cap,lens", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_predict_returns_the_top_k_beside_an_unchanged_mu(gpulib, case, form, cap, lens):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model = _model(case)
    cx, cy = _images(case, 5, 21)
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap, form=form)
    qx = _images(case, NQ, 22)[0]
    plain = _plain(model, state, qx)
    amu, attn = cached.predict(model, state, qx, return_attention=True)
    heads = state.kh.shape[2]
    assert heads == 8 and torch.equal(amu, plain)
    for k in KS:
        mu, idx, w = cached.predict(model, state, qx, top_k=k)
        assert idx.shape == (2, heads, NQ, k) and torch.equal(mu, plain), k
        _consistent(idx, w, attn, lens, cap, k)
        if isinstance(model, ResNetNP):
            assert all(torch.equal(a, b) for a, b in zip(model.predict(state, qx, top_k=k), (mu, idx, w)))
        else:
            assert state.route == "composed"
        # per target row: any chunk gives the single call's bits - 7 splits every 16-row tile
        cmu, cidx, cw = cached.predict(model, state, qx, top_k=k, chunk=7)
        assert torch.equal(cmu, _plain(model, state, qx, chunk=7)) and torch.equal(cidx, idx) and torch.equal(cw, w), k


@pytest.mark.parametrize("form,cap", [("keys", 12), ("long", 40), ("paged", 300)])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_after_evict_the_indices_follow_the_new_slot_order(gpulib, case, form, cap):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 9, 31)
    qx = _images(case, 17, 32)[0]
    lens, drop = (9, 6), [[0, 4], [1]]
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap, form=form)
    new = cached.evict(model, state, drop)
    assert new.lens == (7, 5)
    attn = cached.predict(model, new, qx, return_attention=True)[1]
    for k in (3, 16):
        mu, idx, w = cached.predict(model, new, qx, top_k=k)
        assert torch.equal(mu, _plain(model, new, qx))
        _consistent(idx, w, attn, new.lens, cap, k)
        assert int(idx.max()) < max(new.lens)                          # no index of the old order survives
    # the old state stays valid and still speaks in its own slot order
    old = cached.predict(model, state, qx, top_k=3)
    _consistent(old[1], old[2], cached.predict(model, state, qx, return_attention=True)[1], lens, cap, 3)
