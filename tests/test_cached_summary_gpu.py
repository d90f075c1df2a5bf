"""condition(form="summary") / extend / predict on the MI355X: 40 context shots - beyond the per-shot form's 32 -
against the per-shot mathematics (mlhot_favor_fwd on the kept keys of all 40 shots), growth against a one-off condition, chunked
against unchunked, agreement with the default form below the cap, stale and foreign states.  The bar is the cached tests' 1e-4 of mu's
scale.  Run with -m gpu."""
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


def _build(case):
    method, cfg, _, _ = CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _model(case):
    return _build(case)


@functools.lru_cache(maxsize=None)
def _batch(case, Nc=40, Nq=17):
    _, _, img, L = CASES[case]
    g = torch.Generator().manual_seed(11)
    return tuple(t.to(DEV) for t in (torch.rand(T, Nc, *img, generator=g), torch.rand(T, Nc, L, generator=g), torch.rand(T, Nq, *img, generator=g)))


def _per_shot_state(model, cx, cy):
    """The state of the per-shot mathematics for any number of shots: the kept keys (favor_keys' "plain" route above 32 shots, so
    predict runs mlhot_favor_fwd on them) and the value heads."""
    from mlhot import cached
    from mlhot.ops import favor_keys
    from networks._resnet_np import ContextState, ResNetNP
    Nc = cx.shape[1]
    with torch.no_grad():
        if isinstance(model, ResNetNP):
            kh, vh = model._shot_rows(cx.reshape(T * Nc, *cx.shape[2:]), cy.reshape(T * Nc, -1))
        else:
            kh, vh = cached._shot_rows(model, cx.reshape(T * Nc, *cx.shape[2:]), cy.reshape(T * Nc, -1))
        kh, vh = kh.reshape(T, Nc, *kh.shape[1:]).contiguous(), vh.reshape(T, Nc, *vh.shape[1:]).contiguous()
        keys = favor_keys(kh, model.attn.projection_matrix)
        assert keys.route == ("plain" if Nc > 32 else "cached")
        if isinstance(model, ResNetNP):
            return ContextState(model, T, Nc, model._fingerprint(), "attention", keys=keys, vh=vh)
        return cached.VanillaContextState(model, T, Nc, cached._fingerprint(model), "attention", keys=keys, vh=vh, wq=cached._stacked(model._W_q))


@pytest.mark.parametrize("case", list(CASES))
def test_forty_shots_against_the_per_shot_form(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="summary")
    assert state.form == "summary" and state.lens == (40, 40) and state.capacity is None and state.vh is None and state.kh is None
    assert state.keys.route == "summary"
    ref = _per_shot_state(model, cx, cy)
    for Nq in (3, 17):
        got = cached.predict(model, state, qx[:, :Nq].contiguous())
        want = cached.predict(model, ref, qx[:, :Nq].contiguous(), **({} if case == "resnet_anp" else {"route": "composed"}))
        err = U.rel_err(got, want)
        print(f"summary predict {case} 40 shots, {Nq} targets: {err:.2e} of mu's scale against the per-shot form")
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL
    if case == "vanilla_anp":
        assert state.route == "composed"
    full = cached.predict(model, state, qx)
    assert torch.equal(cached.predict(model, state, qx, chunk=3), full)


@pytest.mark.parametrize("case", list(CASES))
def test_extend_equals_a_one_off_condition(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    # task 1's 31 shots: its first 20 slots, then the first 11 of the next 20
    first = cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous(), form="summary")
    grown = cached.extend(model, first, cx[:, 20:].contiguous(), cy[:, 20:].contiguous(), new_len=[20, 11])
    assert grown.lens == (40, 31) and first.lens == (20, 20) and grown.form == "summary"
    once = cached.condition(model, cx, cy, ctx_len=[40, 31], form="summary")
    assert once.lens == (40, 31)
    got, want = cached.predict(model, grown, qx), cached.predict(model, once, qx)
    err = U.rel_err(got, want)
    print(f"summary extend {case} 20 + [20, 11] against condition(ctx_len=[40, 31]): {err:.2e} of mu's scale")
    assert err <= U.RTOL
    again = cached.predict(model, first, qx)                          # the old state still serves its 20 shots
    assert U.rel_err(again, cached.predict(model, cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous()), qx)) <= U.RTOL
    if hasattr(model, "extend"):                                      # the ResNet family's methods take the same arguments
        assert torch.equal(model.predict(model.extend(first, cx[:, 20:].contiguous(), cy[:, 20:].contiguous(), new_len=[20, 11]), qx), got)


@pytest.mark.parametrize("case", list(CASES))
def test_both_forms_agree_below_the_cap(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    cx, cy = cx[:, :15].contiguous(), cy[:, :15].contiguous()
    keys, summary = cached.condition(model, cx, cy), cached.condition(model, cx, cy, form="summary")
    assert keys.form == "keys" and keys.keys.route == "cached" and summary.keys.route == "summary"
    err = U.rel_err(cached.predict(model, summary, qx), cached.predict(model, keys, qx))
    print(f"{case} 15 shots: form summary against the default form {err:.2e} of mu's scale")
    assert err <= U.RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_stale_and_foreign_states_are_refused(gpulib, case):
    from mlhot import cached
    model, other = _build(case), _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="summary")
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(other, state, qx)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.extend(other, state, cx, cy)
    if case == "vanilla_anp":
        with pytest.raises(ValueError, match='route "fused"'):
            cached.predict(model, state, qx, route="fused")
    cached.predict(model, state, qx)
    with torch.no_grad():
        next(model.parameters()).mul_(1.0)                            # a weight update, whatever its size
    with pytest.raises(ValueError, match="stale"):
        cached.predict(model, state, qx)
    with pytest.raises(ValueError, match="stale"):
        cached.extend(model, state, cx, cy)
