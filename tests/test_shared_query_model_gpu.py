"""predict(shared_targets=True) of both model families on the MI355X: one set of target images [Nq, ...] asked of all
T stored contexts.  Vanilla attention models at T = 3 with states of form "keys" and "long" (capacity 40, full and ragged), the
vanilla CNP's three aggregations and an empty state, the ResNet ANP and CNP at the r_anp_shapenet3d / r_cnp_shapenet3d_max fixture
dimensions with T = 2.  Context sizes stay within 40 slots.  Run with -m gpu.

The bar against `predict` on the expanded targets and against the plain forward is U.RTOL of mu's scale, the bound
tests/test_cached_vanilla_gpu.py and tests/test_condition_gpu.py hold predict to against forward - not the bit: the encoder and
LinearFunction may pick their kernel by row count, and the shared call hands them Nq rows where the expanded one hands them T * Nq."""
import functools
import importlib
import types

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64)
SHAPENET = dict(CFG1D, task="shapenet_1d", input_dim=3, output_dim=2)
PASCAL = dict(CFG1D, task="pascal_1d", input_dim=1, output_dim=1)
# case -> (class, tasks per batch, config)
MODEL_CASES = {
    "anp_shapenet1d": ("ANPShapeNet1D", 3, dict(SHAPENET, agg_mode="attention", dim_r=64)),
    "anp_pascal1d": ("ANPVanillaPascal1D", 3, dict(PASCAL, agg_mode="attention", dim_r=64)),
    "cnp_shapenet1d_mean": ("CNPShapeNet1D", 3, dict(SHAPENET, agg_mode="mean", dim_r=100)),
    "cnp_shapenet1d_max": ("CNPShapeNet1D", 3, dict(SHAPENET, agg_mode="max", dim_r=100)),
    "cnp_shapenet1d_baco": ("CNPShapeNet1D", 3, dict(SHAPENET, agg_mode="baco", dim_r=256)),
    "anp_3d": ("ANP", 2, dict(CFG3D, agg_mode="attention")),
    "cnp_3d_max": ("CondNeuralProcess", 2, dict(CFG3D, agg_mode="max")),
}
ATTENTIVE = ["anp_shapenet1d", "anp_pascal1d", "anp_3d"]
LATENT = ["cnp_shapenet1d_mean", "cnp_shapenet1d_max", "cnp_shapenet1d_baco", "cnp_3d_max"]
NC, NQ, CAP = 5, 17, 40
# the states of an attention model: (form, capacity, ctx_len); None = the plain call, every slot a shot
STATES = [("keys", None, None), ("keys", 8, "ragged"), ("long", CAP, None), ("long", CAP, "ragged")]


@functools.lru_cache(maxsize=None)
def _model(case):
    method, T, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _shape(case):
    cfg = MODEL_CASES[case][2]
    Hh, W, Cc = cfg["img_size"]
    return (Cc - 1 if cfg["task"] == "shapenet_3d" else Cc, Hh, W)


def _context(case, n, seed):
    """(images [T, n, C, H, W], labels [T, n, L]) on the device."""
    T, cfg = MODEL_CASES[case][1], MODEL_CASES[case][2]
    g = torch.Generator().manual_seed(seed)
    return torch.rand(T, n, *_shape(case), generator=g).to(DEV), torch.rand(T, n, cfg["input_dim"], generator=g).to(DEV)


def _targets(case, n, seed):
    """[n, C, H, W]: no task axis"""
    return torch.rand(n, *_shape(case), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _expanded(case, qx):
    return qx[None].expand(MODEL_CASES[case][1], *qx.shape).contiguous()


def _lens(case):
    return [3, 5, 1][:MODEL_CASES[case][1]]


def _state(case, form, cap, ragged):
    from mlhot import cached
    model = _model(case)
    cx, cy = _context(case, NC, 3)
    if form == "keys" and cap is None:
        return cached.condition(model, cx, cy), None
    lens = _lens(case) if ragged else None
    return cached.condition(model, cx, cy, ctx_len=lens, capacity=cap, form=form), lens


def _per_task(model, state, qe, **kw):
    """predict on per-task targets, on the route the shared call runs: the vanilla family's composed route, ResNetNP's only one"""
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    return cached.predict(model, state, qe, **kw) if isinstance(model, ResNetNP) else cached.predict(model, state, qe, route="composed", **kw)


def _forward(model, cx, cy, qe, at_most=15):
    """The plain test-mode forward over slices of at most 15 targets (a target's output depends on the context and that target only)"""
    with torch.no_grad():
        return torch.cat([model(cx, cy, qe[:, i:i + at_most].contiguous(), test=True)[0] for i in range(0, qe.shape[1], at_most)], dim=1)


class _Rows:
    """Records the image count of every encoder / trunk call of the binding while it is installed"""

    def __init__(self, gpulib, monkeypatch):
        self.enc, self.trunk = [], []
        enc, trunk = gpulib.enc_vanilla_fwd, gpulib.trunk_fwd

        def enc_vanilla_fwd(a, b, *rest, **kw):
            self.enc.append(a.shape[0] + (0 if b is None else b.shape[0]))
            return enc(a, b, *rest, **kw)

        def trunk_fwd(passes, *rest, **kw):
            self.trunk.extend(img.shape[0] for img, _ in passes)
            return trunk(passes, *rest, **kw)
        monkeypatch.setattr(gpulib, "enc_vanilla_fwd", enc_vanilla_fwd)
        monkeypatch.setattr(gpulib, "trunk_fwd", trunk_fwd)

    calls = property(lambda self: self.enc + self.trunk)


@pytest.mark.parametrize("form,cap,ragged", STATES, ids=[f"{f}-{'ragged' if r else 'full'}" for f, _, r in STATES])
@pytest.mark.parametrize("case", ATTENTIVE)
def test_attention_models(gpulib, monkeypatch, case, form, cap, ragged):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model, T = _model(case), MODEL_CASES[case][1]
    state, lens = _state(case, form, cap, ragged)
    assert state.kind == "attention" and state.form == form and state.keys.route == ("cached" if form == "keys" else "long")
    qx = _targets(case, NQ, 4)
    qe = _expanded(case, qx)
    rows = _Rows(gpulib, monkeypatch)
    mu = cached.predict(model, state, qx, shared_targets=True)
    seen = rows.calls
    monkeypatch.undo()
    # 5. the encoder sees Nq images, not T * Nq: one vanilla encoder call, or the target and the decoder trunk pass
    assert seen == ([NQ, NQ] if isinstance(model, ResNetNP) else [NQ]), seen
    assert mu.shape[:2] == (T, NQ) and bool(torch.isfinite(mu).all())
    if isinstance(model, ResNetNP):
        assert torch.equal(model.predict(state, qx, shared_targets=True), mu)          # the method is the same call
    else:
        assert state.route == "composed"
    # 1. against predict on the expanded targets
    want = _per_task(model, state, qe)
    e1 = U.rel_err(mu, want)
    # 3. the attention: exact zeros behind ctx_len, rows that sum to 1, mu unmoved; against the per-task read-out
    mu_a, attn = cached.predict(model, state, qx, shared_targets=True, return_attention=True)
    slots = state.Nc
    assert attn.shape == (T, 8, NQ, slots) and torch.equal(mu_a, mu)
    assert bool(torch.isfinite(attn).all()) and float(attn.min()) >= 0.0
    excess = float((attn.double().sum(dim=-1) - 1.0).abs().max())
    assert excess <= AC.rowsum_bound(slots), excess
    for t, L in enumerate(lens if lens is not None else [NC] * T):
        assert bool((attn[t, :, :, L:] == 0.0).all()) and float(attn[t, :, :, :L].min()) > 0.0, t
    want_attn = _per_task(model, state, qe, return_attention=True)[1]
    ea = U.rel_err(attn, want_attn)
    line = f"predict(shared_targets=True) {case} {form} {'ragged' if ragged else 'full'}: mu {e1:.2e} of its scale against predict on the expanded targets, attn {ea:.2e}"
    # 2. against the plain forward (a ragged state has no single forward call: its tasks differ in size)
    if not ragged:
        cx, cy = _context(case, NC, 3)
        e2 = U.rel_err(mu, _forward(model, cx, cy, qe))
        line += f", mu {e2:.2e} against forward"
    print(line)
    assert e1 <= U.RTOL and ea <= U.RTOL, line
    if not ragged:
        assert e2 <= U.RTOL, line
    # 4. chunked equals unchunked to the bit
    for chunk in (1, 16):
        assert torch.equal(cached.predict(model, state, qx, shared_targets=True, chunk=chunk), mu), chunk
    cmu, cattn = cached.predict(model, state, qx, shared_targets=True, chunk=16, return_attention=True)
    assert torch.equal(cmu, mu) and torch.equal(cattn, attn)


@pytest.mark.parametrize("kind", ["latent", "empty"])
@pytest.mark.parametrize("case", LATENT)
def test_latent_and_empty_states(gpulib, monkeypatch, case, kind):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model, T = _model(case), MODEL_CASES[case][1]
    cx, cy = _context(case, NC if kind == "latent" else 0, 3)
    state = cached.condition(model, cx, cy)
    assert state.kind == kind
    qx = _targets(case, NQ, 4)
    qe = _expanded(case, qx)
    rows = _Rows(gpulib, monkeypatch)
    mu = cached.predict(model, state, qx, shared_targets=True)
    seen = rows.calls
    monkeypatch.undo()
    assert seen == [NQ], seen                                                          # ResNet: the decoder trunk pass alone
    assert mu.shape[:2] == (T, NQ) and bool(torch.isfinite(mu).all())
    e1, e2 = U.rel_err(mu, _per_task(model, state, qe)), U.rel_err(mu, _forward(model, cx, cy, qe))
    line = f"predict(shared_targets=True) {case} {kind}: mu {e1:.2e} of its scale against predict on the expanded targets, {e2:.2e} against forward"
    print(line)
    assert e1 <= U.RTOL and e2 <= U.RTOL, line
    for chunk in (1, 16):
        assert torch.equal(cached.predict(model, state, qx, shared_targets=True, chunk=chunk), mu), chunk
    with pytest.raises(ValueError, match="has no attention"):
        cached.predict(model, state, qx, shared_targets=True, return_attention=True)
    if isinstance(model, ResNetNP):
        assert torch.equal(model.predict(state, qx, shared_targets=True), mu)


@pytest.mark.parametrize("case", ["anp_shapenet1d", "anp_3d"])
def test_every_refusal_comes_before_any_launch(gpulib, monkeypatch, case):
    """6. and 7.: each refusal is a ValueError naming what was asked, the encoder wrapper records no call, and no kernel is launched"""
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model, T = _model(case), MODEL_CASES[case][1]
    cx, cy = _context(case, NC, 3)
    qx = _targets(case, NQ, 4)
    qe = _expanded(case, qx)
    state = cached.condition(model, cx, cy)
    summary = cached.condition(model, cx, cy, form="summary")
    paged = cached.condition(model, cx, cy, form="paged", capacity=300)
    other = _model("anp_pascal1d" if case == "anp_shapenet1d" else "cnp_3d_max")
    foreign = cached.condition(other, *_context("anp_pascal1d" if case == "anp_shapenet1d" else "cnp_3d_max", NC, 3))
    refused = [
        (dict(context_mask=torch.ones(T, NQ, NC, dtype=torch.bool, device=DEV)), state, qx, "shared_targets=True with context_mask="),
        (dict(attention_mass=True), state, qx, "shared_targets=True with attention_mass=True"),
        (dict(target_weight=torch.ones(T, NQ, device=DEV)), state, qx, "shared_targets=True with target_weight="),
        (dict(top_k=3), state, qx, "shared_targets=True with top_k="),
        ({}, summary, qx, "this state is a 'summary' state"),
        ({}, paged, qx, "this state is a 'paged' state"),
        ({}, state, qe, "no task axis"),
        ({}, foreign, qx, "not made by this model"),
        (dict(chunk=0), state, qx, "chunk must be a positive"),
    ]
    if not isinstance(model, ResNetNP):
        refused += [(dict(route="fused"), state, qx, 'shared_targets=True with route "fused"'),
                    (dict(route="fused_summary"), summary, qx, "this state is a 'summary' state")]
    rows = _Rows(gpulib, monkeypatch)

    def check(kw, st, x, says):
        def refusal():
            with pytest.raises(ValueError, match=says):
                cached.predict(model, st, x, shared_targets=True, **kw)
        launched, _ = U.launch_labels(gpulib, refusal)
        assert launched == [] and rows.calls == [], (says, launched, rows.calls)
    for item in refused:
        check(*item)
    model.train()
    try:
        check({}, state, qx, "eval")
    finally:
        model.eval()
    # 7. after a weight update the state is stale, for the shared call as for the plain one
    p = next(model.parameters())
    with torch.no_grad():
        p.add_(0.0)
    check({}, state, qx, "stale")
    with pytest.raises(ValueError, match="stale"):
        cached.predict(model, state, qe)
    assert rows.calls == []
    monkeypatch.undo()
    fresh = cached.condition(model, cx, cy)                                            # ... and a fresh state serves again
    assert cached.predict(model, fresh, qx, shared_targets=True).shape[:2] == (T, NQ)
