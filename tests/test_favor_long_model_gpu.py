"""condition(form="long") / extend / predict on the MI355X, both families at 40 context shots - beyond the default
form's 32: predict against the model's own forward, growth in two steps against a one-off condition, chunked against unchunked, the
attention read-out above 32 shots, and agreement with the summary form on the same context.  The bar is the cached tests' 1e-4 of
mu's scale (U.RTOL).  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, NC, NQ = 2, 40, 7
CASES = {
    "vanilla_anp": ("ANPShapeNet1D", dict(seed=2578, img_size=[128, 128, 1], input_dim=3, output_dim=2, agg_mode="attention", img_agg="", dim_w=64,
                                          n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d"), (1, 128, 128), 3),
    "resnet_anp": ("ANP", dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
                               agg_mode="attention"), (3, 64, 64), 4),
}


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg, _, _ = CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _batch(case):
    _, _, img, L = CASES[case]
    g = torch.Generator().manual_seed(11)
    return tuple(t.to(DEV) for t in (torch.rand(T, NC, *img, generator=g), torch.rand(T, NC, L, generator=g), torch.rand(T, NQ, *img, generator=g)))


def _rowsum_excess(w):
    return float((w.double().sum(dim=-1) - 1.0).abs().max())


@pytest.mark.parametrize("case", list(CASES))
def test_predict_on_a_long_state_is_the_forward(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="long")
    assert state.form == "long" and state.lens == (NC, NC) and state.capacity == NC and state.Nc == NC
    assert state.keys.route == "long" and state.kh.shape[:2] == (T, NC) and state.vh.shape == state.kh.shape
    with torch.no_grad():
        want = model(cx, cy, qx, test=True)[0]
    got = cached.predict(model, state, qx)
    err = U.rel_err(got, want)
    print(f"long predict {case} {NC} shots, {NQ} targets: {err:.2e} of mu's scale against forward(test=True)")
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL
    if case == "vanilla_anp":
        assert state.route == "composed"
        with pytest.raises(ValueError, match='route "fused"'):
            cached.predict(model, state, qx, route="fused")
    else:
        assert torch.equal(model.predict(model.condition(cx, cy, form="long"), qx), got)            # the methods are the same calls
    assert torch.equal(cached.predict(model, state, qx, chunk=3), got)


@pytest.mark.parametrize("case", list(CASES))
def test_extend_in_two_steps_equals_conditioning_on_all_shots(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    first = cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous(), capacity=NC, form="long")
    assert first.lens == (20, 20) and first.capacity == NC
    mid = cached.extend(model, first, cx[:, 20:30].contiguous(), cy[:, 20:30].contiguous())
    grown = cached.extend(model, mid, cx[:, 30:].contiguous(), cy[:, 30:].contiguous())
    assert mid.lens == (30, 30) and grown.lens == (NC, NC) and grown.form == "long" and first.lens == (20, 20)
    once = cached.condition(model, cx, cy, form="long")
    got, want = cached.predict(model, grown, qx), cached.predict(model, once, qx)
    err = U.rel_err(got, want)
    print(f"long extend {case} 20 + 10 + 10 against condition on {NC}: {err:.2e} of mu's scale")
    assert err <= U.RTOL
    with pytest.raises(ValueError, match="would hold 41 context shots, the state's capacity is 40"):
        cached.extend(model, grown, cx[:, :1].contiguous(), cy[:, :1].contiguous())
    short = cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous(), form="long")   # one chunk: the cached kernels' bits
    keys = cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous(), ctx_len=[20, 20])
    assert keys.form == "keys" and keys.keys.route == "cached"
    kw = {} if case == "resnet_anp" else {"route": "composed"}
    assert torch.equal(cached.predict(model, short, qx), cached.predict(model, keys, qx, **kw))
    assert U.rel_err(cached.predict(model, first, qx), cached.predict(model, short, qx)) <= U.RTOL    # the old state still serves its 20


@pytest.mark.parametrize("case", list(CASES))
def test_attention_above_32_shots(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    lens, cap = (NC, 33), 48
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap, form="long")
    mu, attn = cached.predict(model, state, qx, return_attention=True)
    heads = state.kh.shape[2]
    assert attn.shape == (T, heads, NQ, cap) and attn.dtype == torch.float32
    kw = {} if case == "resnet_anp" else {"route": "composed"}
    assert torch.equal(mu, cached.predict(model, state, qx, **kw))
    assert bool(torch.isfinite(attn).all()) and float(attn.min()) >= 0.0
    for t, L in enumerate(lens):
        assert bool((attn[t, :, :, L:] == 0.0).all()) and float(attn[t, :, :, :L].min()) > 0.0, t
    excess = _rowsum_excess(attn)
    print(f"long predict(return_attention=True) {case} ctx_len={lens} of {cap} slots: |sum_n attn - 1| {excess:.2e} "
          f"({excess / AC.rowsum_bound(cap):.2f} of the bound)")
    assert excess <= AC.rowsum_bound(cap)
    cmu, cattn = cached.predict(model, state, qx, chunk=3, return_attention=True)
    assert torch.equal(cmu, mu) and torch.equal(cattn, attn)
    # float64 weights from the model's own head projections, caught at the call
    from networks import _resnet_np
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        for mod in (cached, _resnet_np):
            real = mod.favor_query
            mp.setattr(mod, "favor_query", lambda qh, *a, _real=real, **k: (seen.append(qh), _real(qh, *a, **k))[1])
        cached.predict(model, state, qx, return_attention=True)
    assert len(seen) == 1
    cpu = lambda t: t.detach().cpu().permute(0, 2, 1, 3)
    w64 = AR.weights(cpu(seen[0]), cpu(state.kh), model.attn.projection_matrix.detach().cpu(), state.keys.lens)
    err = U.rel_err(attn, w64)
    print(f"long predict(return_attention=True) {case}: attn {err:.2e} of its scale against float64 on the model's head projections")
    assert err <= U.RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_long_and_summary_agree_on_the_same_context(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    long, summary = cached.condition(model, cx, cy, form="long"), cached.condition(model, cx, cy, form="summary")
    got, want = cached.predict(model, long, qx), cached.predict(model, summary, qx)
    err = U.rel_err(got, want)
    print(f"{case} {NC} shots: form long against form summary {err:.2e} of mu's scale")
    assert err <= U.RTOL
    with pytest.raises(ValueError, match="has form 'long'"):
        cached.merge(model, [long])
    with pytest.raises(ValueError, match="summary state keeps no per-shot rows"):                    # the summary still has nothing to read out
        cached.predict(model, summary, qx, return_attention=True)
