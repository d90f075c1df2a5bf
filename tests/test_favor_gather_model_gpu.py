"""mlhot.cached.select on the MI355X, both families: objects conditioned apart in batches (a0, a1) and (b0, b1) and
queried as the batch (a1, b0), against a second instance of the model with tasks_per_batch = 4 and the same parameters run on the
UNION batch (a0, a1, b0, b1) - whose key stabiliser is the selected state's, the maximum over both source batches; two pairs per task
against merge, bit for bit; extend on a selected state; every refusal.  The bar is U.RTOL of mu's scale, the one
tests/test_cached_summary_gpu.py holds the summary form's predict to.  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, NC, NQ = 2, 5, 7
CASES = {
    "vanilla_anp": ("ANPShapeNet1D", dict(seed=2578, img_size=[128, 128, 1], input_dim=3, output_dim=2, agg_mode="attention", img_agg="", dim_w=64,
                                          n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d"), (1, 128, 128), 3),
    "resnet_anp": ("ANP", dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
                               agg_mode="attention"), (3, 64, 64), 4),
}
LATENT = ("CNPShapeNet1D", dict(CASES["vanilla_anp"][1], agg_mode="mean", dim_r=100))


def _build(method, cfg, tasks):
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=tasks, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _model(case):
    return _build(*CASES[case][:2], T)


@functools.lru_cache(maxsize=None)
def _batches(case):
    """(ctx images, ctx labels, targets) of the batches a = (a0, a1) and b = (b0, b1)."""
    _, _, img, L = CASES[case]
    g = torch.Generator().manual_seed(41)
    return tuple(tuple(t.to(DEV) for t in (torch.rand(T, NC, *img, generator=g), torch.rand(T, NC, L, generator=g), torch.rand(T, NQ, *img, generator=g)))
                 for _ in range(2))


@functools.lru_cache(maxsize=None)
def _conditioned(case):
    from mlhot import cached
    return tuple(cached.condition(_model(case), cx, cy, form="summary") for cx, cy, _ in _batches(case))


@pytest.mark.parametrize("case", list(CASES))
def test_tasks_picked_across_two_batches_against_the_union_batch(gpulib, case):
    from mlhot import cached
    model = _model(case)
    (ax, ay, aq), (bx, by, bq) = _batches(case)
    a, b = _conditioned(case)
    picked = cached.select(model, [a, b], [(0, 1), (1, 0)])                             # the batch (a1, b0)
    assert picked.form == "summary" and picked.kind == "attention" and picked.T == T and picked.lens == (NC, NC) and picked.Nc == NC
    assert picked.keys.route == "summary" and picked.vh is None and picked.kh is None and picked.capacity is None and picked.wq is a.wq
    assert picked.keys.summary()[4].item() == max(a.keys.summary()[4].item(), b.keys.summary()[4].item())
    qx = torch.stack([aq[1], bq[0]])
    got = cached.predict(model, picked, qx)
    four = _build(*CASES[case][:2], 2 * T)
    four.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = four(torch.cat([ax, bx]), torch.cat([ay, by]), torch.cat([aq, bq]), test=True)[0][1:3]
    err = U.rel_err(got, want)
    print(f"select {case} (a1, b0) against forward on the union batch (a0, a1, b0, b1), rows 1 and 2: {err:.2e} of mu's scale")
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL
    assert torch.equal(cached.predict(model, picked, qx, chunk=3), got)                 # chunked and unchunked, bit for bit
    with pytest.raises(ValueError, match="return_attention=True - a summary state keeps no per-shot rows"):
        cached.predict(model, picked, qx, return_attention=True)
    twice = cached.select(model, [a, b], [(1, 0), (1, 0)])                              # the same object in both slots
    mu = cached.predict(model, twice, torch.stack([bq[0], bq[0]]))
    assert torch.equal(mu[0], mu[1])
    assert cached.supports(model)[0] and a.lens == (NC, NC) and b.lens == (NC, NC)


@pytest.mark.parametrize("case", list(CASES))
def test_two_pairs_per_task_equal_merge(gpulib, case):
    from mlhot import cached
    model = _model(case)
    a, b = _conditioned(case)
    qx = _batches(case)[0][2]
    both = cached.select(model, [a, b], [[(0, 0), (1, 0)], [(0, 1), (1, 1)]])
    merged = cached.merge(model, [a, b])
    assert both.lens == merged.lens == (2 * NC, 2 * NC)
    assert torch.equal(cached.predict(model, both, qx), cached.predict(model, merged, qx))


@pytest.mark.parametrize("case", list(CASES))
def test_extend_on_a_selected_state(gpulib, case):
    from mlhot import cached
    model = _model(case)
    _, _, img, L = CASES[case]
    a, b = _conditioned(case)
    g = torch.Generator().manual_seed(43)
    nx, ny = torch.rand(T, 3, *img, generator=g).to(DEV), torch.rand(T, 3, L, generator=g).to(DEV)      # 3 more shots for a1 and for b0
    picks = [(0, 1), (1, 0)]
    grown = cached.extend(model, cached.select(model, [a, b], picks), nx, ny)
    # the same shots into the sources: a1 is task 1 of a, b0 task 0 of b; the other task of each takes nothing
    a2 = cached.extend(model, a, torch.stack([nx[1], nx[0]]), torch.stack([ny[1], ny[0]]), new_len=[0, 3])
    b2 = cached.extend(model, b, torch.stack([nx[1], nx[0]]), torch.stack([ny[1], ny[0]]), new_len=[3, 0])
    later = cached.select(model, [a2, b2], picks)
    assert grown.lens == later.lens == (NC + 3, NC + 3) and grown.form == "summary"
    qx = _batches(case)[0][2]
    got, want = cached.predict(model, grown, qx), cached.predict(model, later, qx)
    err = U.rel_err(got, want)
    print(f"select {case}, then extend by 3, against select of the extended states: {err:.2e} of mu's scale")
    assert err <= U.RTOL


def test_refusals_with_real_states(gpulib):
    from mlhot import cached
    model = _model("vanilla_anp")
    (ax, ay, _), _ = _batches("vanilla_anp")
    a, b = _conditioned("vanilla_anp")
    ok = [(0, 1), (1, 0)]
    with pytest.raises(ValueError, match=r"select: states\[1\] has form 'keys'"):
        cached.select(model, [a, cached.condition(model, ax, ay)], ok)
    with pytest.raises(ValueError, match=r"select: states\[1\] has form 'long'"):
        cached.select(model, [a, cached.condition(model, ax, ay, form="long")], ok)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.select(_model("resnet_anp"), [a, b], ok)
    with pytest.raises(ValueError, match=r"picks\[0\] is empty"):
        cached.select(model, [a, b], [[], (1, 0)])
    with pytest.raises(ValueError, match=r"picks\[1\] names \(0, 1\) twice"):
        cached.select(model, [a, b], [(0, 0), [(0, 1), (0, 1)]])
    with pytest.raises(ValueError, match=r"names task 2 of states\[0\]"):
        cached.select(model, [a, b], [(0, 2), (1, 0)])
    latent = _build(*LATENT, T)
    z = cached.condition(latent, ax, ay)
    with pytest.raises(ValueError, match=r"states\[0\] is a 'latent' state"):
        cached.select(latent, [z], [(0, 0), (0, 1)])
    mine = _build(*CASES["vanilla_anp"][:2], T)                                        # a model of this test's own: it is about to change
    s = cached.condition(mine, ax, ay, form="summary")
    mine.train()
    with pytest.raises(ValueError, match="select is a test-mode path"):
        cached.select(mine, [s], [(0, 0), (0, 1)])
    mine.eval()
    assert cached.select(mine, [s], [(0, 1), (0, 0)]).lens == (NC, NC)
    with torch.no_grad():
        next(mine.parameters()).add_(1.0)
    with pytest.raises(ValueError, match="stale - a parameter of the model changed"):
        cached.select(mine, [s], [(0, 0), (0, 1)])
