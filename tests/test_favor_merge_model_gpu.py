"""mlhot.cached.merge on the MI355X, both families: a context of 40 shots per task conditioned as two shards of 17
and 23 and merged, against condition(form="summary") on the whole context; a ragged shard pair; extend on a merged state; chunked
against unchunked predict.  The bar is U.RTOL of mu's scale - the one tests/test_cached_summary_gpu.py holds the summary form's
predict to (against the per-shot form and against a one-off condition); no new number is chosen here.  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 2
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
def _batch(case, Nc=40, Nq=9):
    _, _, img, L = CASES[case]
    g = torch.Generator().manual_seed(23)
    return tuple(t.to(DEV) for t in (torch.rand(T, Nc, *img, generator=g), torch.rand(T, Nc, L, generator=g), torch.rand(T, Nq, *img, generator=g)))


@functools.lru_cache(maxsize=None)
def _shards(case):
    """(shard a: shots 0 .. 16, shard b: shots 17 .. 39), each conditioned on its own, and the state of the whole context."""
    from mlhot import cached
    model = _model(case)
    cx, cy, _ = _batch(case)
    a = cached.condition(model, cx[:, :17].contiguous(), cy[:, :17].contiguous(), form="summary")
    b = cached.condition(model, cx[:, 17:].contiguous(), cy[:, 17:].contiguous(), form="summary")
    return a, b, cached.condition(model, cx, cy, form="summary")


@pytest.mark.parametrize("case", list(CASES))
def test_two_shards_merged_against_the_whole_context(gpulib, case):
    from mlhot import cached
    model = _model(case)
    _, _, qx = _batch(case)
    a, b, whole = _shards(case)
    merged = cached.merge(model, [a, b])
    assert merged.form == "summary" and merged.kind == "attention" and merged.lens == (40, 40) and merged.Nc == 40 and merged.capacity is None
    assert merged.keys.route == "summary" and merged.vh is None and merged.kh is None and a.lens == (17, 17) and b.lens == (23, 23)
    got, want = cached.predict(model, merged, qx), cached.predict(model, whole, qx)
    err = U.rel_err(got, want)
    print(f"merge {case} 17 + 23 shots against condition on all 40: {err:.2e} of mu's scale")
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL
    assert merged.keys.summary()[4].item() == whole.keys.summary()[4].item()          # one stabiliser: the maximum over all 40 shots
    assert torch.equal(cached.predict(model, merged, qx, chunk=4), got)                # chunked and unchunked, bit for bit
    back = cached.predict(model, cached.merge(model, [b, a]), qx)                      # the other order: the same context
    assert U.rel_err(back, want) <= U.RTOL
    if hasattr(model, "predict"):
        assert torch.equal(model.predict(merged, qx), got)


@pytest.mark.parametrize("case", list(CASES))
def test_a_ragged_shard_pair(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    # task 0: 17 + 23 shots; task 1: the first 5 of shard a and the first 12 of shard b
    a = cached.condition(model, cx[:, :17].contiguous(), cy[:, :17].contiguous(), ctx_len=[17, 5], form="summary")
    b = cached.condition(model, cx[:, 17:].contiguous(), cy[:, 17:].contiguous(), ctx_len=[23, 12], form="summary")
    merged = cached.merge(model, [a, b])
    assert merged.lens == (40, 17) and merged.Nc == 40
    jx, jy = cx.clone(), cy.clone()
    jx[1, 5:17], jy[1, 5:17] = cx[1, 17:29], cy[1, 17:29]                              # task 1's 17 shots, packed to the front
    once = cached.condition(model, jx, jy, ctx_len=[40, 17], form="summary")
    err = U.rel_err(cached.predict(model, merged, qx), cached.predict(model, once, qx))
    print(f"merge {case} ctx_len [17, 5] + [23, 12] against condition(ctx_len=[40, 17]): {err:.2e} of mu's scale")
    assert err <= U.RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_extend_on_a_merged_state(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    a = cached.condition(model, cx[:, :10].contiguous(), cy[:, :10].contiguous(), form="summary")
    b = cached.condition(model, cx[:, 10:25].contiguous(), cy[:, 10:25].contiguous(), form="summary")
    merged = cached.merge(model, [a, b])
    grown = cached.extend(model, merged, cx[:, 25:].contiguous(), cy[:, 25:].contiguous())
    assert grown.lens == (40, 40) and merged.lens == (25, 25) and grown.form == "summary"
    got, want = cached.predict(model, grown, qx), cached.predict(model, _shards(case)[2], qx)
    err = U.rel_err(got, want)
    print(f"merge {case} 10 + 15, then extend by 15, against condition on all 40: {err:.2e} of mu's scale")
    assert err <= U.RTOL
    assert torch.equal(cached.predict(model, grown, qx, chunk=2), got)
    three = cached.merge(model, [merged, cached.condition(model, cx[:, 25:].contiguous(), cy[:, 25:].contiguous(), form="summary")])
    assert three.lens == (40, 40) and U.rel_err(cached.predict(model, three, qx), want) <= U.RTOL      # a merged state merges again


def test_refusals_with_real_states(gpulib):
    from mlhot import cached
    model = _model("vanilla_anp")
    cx, cy, _ = _batch("vanilla_anp")
    a, b, _ = _shards("vanilla_anp")
    keys = cached.condition(model, cx[:, :5].contiguous(), cy[:, :5].contiguous())
    with pytest.raises(ValueError, match=r"states\[1\] has form 'keys'"):
        cached.merge(model, [a, keys])
    with pytest.raises(ValueError, match="not made by this model"):
        cached.merge(_model("resnet_anp"), [a, b])
