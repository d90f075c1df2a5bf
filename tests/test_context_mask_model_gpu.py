"""predict(context_mask=) and mlhot.cached.leave_one_out on the MI355X, on ANPShapeNet1D (the vanilla family) and
the ResNet ANP at the smallest configurations of tests/test_attention_readout_gpu.py: an all-True mask has the unmasked call's bits, a
4-D mask those of its G 3-D calls, chunked equals unchunked, mu does not move with return_attention, the masked prediction equals the
model's own forward on the sub-context, leave_one_out equals the loop, and every refusal is raised before any launch.
Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import context_mask_ref as CM
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64)
SHAPENET = dict(CFG1D, task="shapenet_1d", input_dim=3, output_dim=2)
MODEL_CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention")),
    "anp_shapenet1d": ("ANPShapeNet1D", dict(SHAPENET, agg_mode="attention", dim_r=64)),
    "cnp_shapenet1d_mean": ("CNPShapeNet1D", dict(SHAPENET, agg_mode="mean", dim_r=100)),
}
ATTENTIVE = ["anp_3d", "anp_shapenet1d"]
T, NC, NQ = 2, 5, 7


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _images(case, n, seed):
    cfg = MODEL_CASES[case][1]
    g = torch.Generator().manual_seed(seed)
    Hh, W, Cc = cfg["img_size"]
    Cc = Cc - 1 if cfg["task"] == "shapenet_3d" else Cc
    return torch.rand(T, n, Cc, Hh, W, generator=g).to(DEV), torch.rand(T, n, cfg["input_dim"], generator=g).to(DEV)


def _plain(model, state, qx, **kw):
    """predict without a mask on the route the masked call runs: the vanilla family's composed route, ResNetNP's only one"""
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    return cached.predict(model, state, qx, **kw) if isinstance(model, ResNetNP) else cached.predict(model, state, qx, route="composed", **kw)


def _masks(Nc, G=3, Nq=NQ, seed=2):
    mk = torch.rand(T, G, Nq, Nc, generator=torch.Generator().manual_seed(seed)) < 0.5
    mk[..., 0] = True                                                 # slot 0 is a shot of every task: no row is left empty
    return mk.to(DEV)


def _peak_slot(model, state):
    """The slot index of the shot that holds the batch maximum of dd_k = (c k) P^T over all tasks and heads, in float64 from the
    state's kept key rows: the shot whose dd_k IS the key stabiliser M."""
    kh = state.kh.detach().cpu().double()                             # [T, Nc, H, d]
    valid = torch.arange(state.Nc)[None, :] < torch.tensor(state.lens)[:, None]
    dd = torch.einsum("tnhd,md->tnhm", kh.shape[-1] ** -0.25 * kh, model.attn.projection_matrix.detach().cpu().double())
    dd = torch.where(valid[:, :, None, None], dd, torch.full((), -float("inf"), dtype=torch.float64))
    return int(dd.amax(dim=(0, 2, 3)).argmax())


@pytest.mark.parametrize("form", ["keys", "long"])
@pytest.mark.parametrize("case", ATTENTIVE)
def test_masks_have_the_bits_of_the_calls_they_stand_for(gpulib, case, form):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, NC, 3)
    qx = _images(case, NQ, 4)[0]
    state = cached.condition(model, cx, cy, form=form)
    ones = torch.ones(T, NQ, NC, dtype=torch.bool, device=DEV)
    mu1 = cached.predict(model, state, qx, context_mask=ones)
    assert mu1.shape[:2] == (T, NQ) and torch.equal(mu1, _plain(model, state, qx))              # all True: the unmasked call
    mk = _masks(NC)
    mu = cached.predict(model, state, qx, context_mask=mk)
    assert mu.shape == (T, 3, NQ, mu1.shape[-1]) and mu.is_contiguous()
    for g in range(3):                                                                            # a 4-D mask is its G 3-D calls
        assert torch.equal(mu[:, g], cached.predict(model, state, qx, context_mask=mk[:, g])), g
    assert torch.equal(cached.predict(model, state, qx, context_mask=mk, chunk=3), mu)            # chunked = unchunked
    mu_a, attn = cached.predict(model, state, qx, context_mask=mk, return_attention=True)
    heads = state.kh.shape[2]
    assert torch.equal(mu_a, mu) and attn.shape == (T, 3, heads, NQ, NC)
    keep = mk[:, :, None].expand_as(attn)
    assert bool((attn[~keep] == 0.0).all()) and float(attn[keep].min()) > 0.0
    assert float((attn.double().sum(dim=-1) - 1.0).abs().max()) <= NC * 2.0 ** -23
    mu_c, attn_c = cached.predict(model, state, qx, context_mask=mk, return_attention=True, chunk=2)
    assert torch.equal(mu_c, mu) and torch.equal(attn_c, attn)
    mu3, attn3 = cached.predict(model, state, qx, context_mask=mk[:, 1], return_attention=True)
    assert torch.equal(mu3, mu[:, 1]) and torch.equal(attn3, attn[:, 1])
    if hasattr(model, "condition"):                                                               # ResNetNP: the method is the same call
        assert torch.equal(model.predict(state, qx, context_mask=mk), mu)


@pytest.mark.parametrize("case", ATTENTIVE)
def test_a_masked_prediction_is_the_forward_on_the_sub_context(gpulib, case, monkeypatch):
    """Group g drops one context slot for every task; the reference is the model's own forward on the other slots.  The key
    stabiliser M of the masked call is the state's - the maximum of dd_k over ALL conditioned shots - while the forward on a
    sub-context takes it over the kept shots only.  So the slot that holds the maximum (found in float64) is kept by every mask of
    the comparison: both sides then use one M and the tolerance is the one predict has against forward, U.RTOL, not loosened for the
    eps terms.  The last case drops exactly that slot: the forward would use another M, which moves FAVOR+'s 1e-4 floors (6c-6), so
    it asserts agreement with the float64 statement under the state's M instead - on the attention weights, from the model's own
    query heads."""
    from mlhot import cached
    from networks import _resnet_np
    model = _model(case)
    cx, cy = _images(case, NC, 5)
    qx = _images(case, NQ, 6)[0]
    state = cached.condition(model, cx, cy)
    peak = _peak_slot(model, state)
    drops = [c for c in range(NC) if c != peak]
    mk = torch.ones(T, len(drops), NQ, NC, dtype=torch.bool, device=DEV)
    for g, c in enumerate(drops):
        mk[:, g, :, c] = False
    mu = cached.predict(model, state, qx, context_mask=mk)
    for g, c in enumerate(drops):
        keep = [n for n in range(NC) if n != c]
        with torch.no_grad():
            want = model(cx[:, keep].contiguous(), cy[:, keep].contiguous(), qx, test=True)[0]
        err = U.rel_err(mu[:, g], want)
        print(f"predict(context_mask=) {case} without slot {c} (stabiliser in slot {peak}): {err:.2e} of mu's scale against forward on the sub-context")
        assert err <= U.RTOL, (g, c)
    # the slot that holds M masked: float64 under the state's M
    seen = []
    for mod in (cached, _resnet_np):
        real = mod.favor_query
        monkeypatch.setattr(mod, "favor_query", lambda qh, *a, _real=real, **kw: (seen.append(qh), _real(qh, *a, **kw))[1])
    no_peak = torch.ones(T, 1, NQ, NC, dtype=torch.bool, device=DEV)
    no_peak[..., peak] = False
    _, attn = cached.predict(model, state, qx, context_mask=no_peak, return_attention=True)
    monkeypatch.undo()
    assert len(seen) == 1
    cpu = lambda t: t.detach().cpu().permute(0, 2, 1, 3)
    _, w64 = CM.masked(cpu(seen[0]), cpu(state.kh), cpu(state.vh), model.attn.projection_matrix.detach().cpu(), no_peak.cpu())
    err = U.rel_err(attn, w64)
    print(f"predict(context_mask=) {case} without the stabiliser's slot {peak}: attn {err:.2e} of its scale against float64 under the state's M")
    assert err <= U.RTOL and bool((attn[..., peak] == 0.0).all())


@pytest.mark.parametrize("form", ["keys", "long"])
@pytest.mark.parametrize("case", ATTENTIVE)
def test_leave_one_out_is_the_loop_of_masked_predicts(gpulib, case, form):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, NC, 7)
    qx = _images(case, NQ, 8)[0]
    lens, cap = (2, NC), 8
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap, form=form)
    loo = cached.leave_one_out(model, state, qx)
    assert loo.shape[:3] == (T, cap, NQ) and bool(torch.isfinite(loo).all())
    for c in range(cap):
        mk = torch.ones(T, NQ, cap, dtype=torch.bool, device=DEV)
        mk[..., c] = False
        assert torch.equal(loo[:, c], cached.predict(model, state, qx, context_mask=mk)), c
    plain = _plain(model, state, qx)
    for t, L in enumerate(lens):                                       # dropping a slot that holds no shot drops nothing
        for c in range(L, cap):
            assert torch.equal(loo[t, c], plain[t]), (t, c)
        assert not torch.equal(loo[t, 0], plain[t])
    assert torch.equal(cached.leave_one_out(model, state, qx, chunk=3), loo)
    single = cached.condition(model, cx, cy, ctx_len=[1, NC], capacity=cap, form=form)
    labels, _ = U.launch_labels(gpulib, lambda: pytest.raises(ValueError, cached.leave_one_out, model, single, qx).match("single context shot"))
    assert labels == []


@pytest.mark.parametrize("case", ATTENTIVE)
def test_every_refusal_comes_before_any_launch(gpulib, case):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model = _model(case)
    cx, cy = _images(case, NC, 9)
    qx = _images(case, NQ, 10)[0]
    ones = torch.ones(T, NQ, NC, dtype=torch.bool, device=DEV)
    state = cached.condition(model, cx, cy)
    summary = cached.condition(model, cx, cy, form="summary")
    other = _model("cnp_shapenet1d_mean")
    ox, oy = _images("cnp_shapenet1d_mean", NC, 11)
    latent, empty = cached.condition(other, ox, oy), cached.condition(other, ox[:, :0], oy[:, :0])
    oq = _images("cnp_shapenet1d_mean", NQ, 12)[0]
    hole = ones.clone()
    hole[1, 4] = False

    def refused(match, fn):
        labels, _ = U.launch_labels(gpulib, lambda: pytest.raises(ValueError, fn).match(match))
        assert labels == [], (match, labels)
    refused("summary state keeps no per-shot rows", lambda: cached.predict(model, summary, qx, context_mask=ones))
    refused("has no attention", lambda: cached.predict(other, latent, oq, context_mask=ones))
    refused("has no attention", lambda: cached.predict(other, empty, oq, context_mask=torch.ones(T, NQ, 0, dtype=torch.bool, device=DEV)))
    refused("keeps none of the 5 valid context shots of task 1 for target 4", lambda: cached.predict(model, state, qx, context_mask=hole))
    refused("not made by this model", lambda: cached.predict(model, latent, qx, context_mask=ones))
    if not isinstance(model, ResNetNP):
        for route in ("fused", "fused_summary"):
            refused(f'context_mask= with route "{route}"', lambda: cached.predict(model, state, qx, route=route, context_mask=ones))
        assert cached.predict(model, state, qx) is not None and state.route == "fused"            # the default call keeps its route
    stale = cached.condition(model, cx, cy)
    p = next(model.parameters())
    with torch.no_grad():
        p.add_(0.0)                                                    # a version bump, the values stay
    refused("stale", lambda: cached.predict(model, stale, qx, context_mask=ones))
