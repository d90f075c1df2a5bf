"""predict(route="fused_summary") on whole models on the MI355X: ANPShapeNet1D and ANPVanillaPascal1D at T = 2 with
40 context shots and 17 targets - against the per-shot mathematics and the plain forward, chunked against unchunked, on states that
extend, merge and select built, and the existing routes as they were.  The bar is the cached tests' U.RTOL of mu's scale.
Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 2
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64, agg_mode="attention",
             dim_r=64)
CASES = {
    "anp_shapenet1d": ("ANPShapeNet1D", dict(CFG1D, task="shapenet_1d", input_dim=3, output_dim=2), 3),
    "anp_pascal1d": ("ANPVanillaPascal1D", dict(CFG1D, task="pascal_1d", input_dim=1, output_dim=1), 1),
}


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg, _ = CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _batch(case, Nc=40, Nq=17):
    L = CASES[case][2]
    g = torch.Generator().manual_seed(11)
    return tuple(t.to(DEV) for t in (torch.rand(T, Nc, 1, 128, 128, generator=g), torch.rand(T, Nc, L, generator=g), torch.rand(T, Nq, 1, 128, 128, generator=g)))


def _per_shot_state(model, cx, cy):
    """tests/test_cached_summary_gpu.py's yardstick: the kept keys of all shots (favor_keys' "plain" route above 32) and the value heads."""
    from mlhot import cached
    from mlhot.ops import favor_keys
    Nc = cx.shape[1]
    with torch.no_grad():
        kh, vh = cached._shot_rows(model, cx.reshape(T * Nc, *cx.shape[2:]), cy.reshape(T * Nc, -1))
        kh, vh = kh.reshape(T, Nc, *kh.shape[1:]).contiguous(), vh.reshape(T, Nc, *vh.shape[1:]).contiguous()
        keys = favor_keys(kh, model.attn.projection_matrix)
        assert keys.route == "plain"
        return cached.VanillaContextState(model, T, Nc, cached._fingerprint(model), "attention", keys=keys, vh=vh, wq=cached._stacked(model._W_q))


@pytest.mark.parametrize("case", list(CASES))
def test_forty_shots_against_the_per_shot_form_and_the_plain_forward(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="summary")
    got = cached.predict(model, state, qx, route="fused_summary")
    assert state.route == "fused_summary"
    want = cached.predict(model, _per_shot_state(model, cx, cy), qx, route="composed")
    with torch.no_grad():
        plain = model(cx, cy, qx, test=True)[0]
    e1, e2 = U.rel_err(got, want), U.rel_err(got, plain)
    print(f"fused_summary predict {case} 40 shots, 17 targets: {e1:.2e} of mu's scale against the per-shot form, {e2:.2e} against the plain forward")
    assert got.shape == want.shape == plain.shape and bool(torch.isfinite(got).all())
    assert e1 <= U.RTOL and e2 <= U.RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_chunked_equals_unchunked(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="summary")
    full = cached.predict(model, state, qx, route="fused_summary")
    assert torch.equal(cached.predict(model, state, qx, chunk=3, route="fused_summary"), full) and state.route == "fused_summary"


@pytest.mark.parametrize("case", list(CASES))
def test_states_of_extend_merge_and_select_are_served(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    first = cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous(), form="summary")
    second = cached.condition(model, cx[:, 20:].contiguous(), cy[:, 20:].contiguous(), form="summary")
    states = {
        "extend": cached.extend(model, first, cx[:, 20:].contiguous(), cy[:, 20:].contiguous(), new_len=[20, 11]),
        "merge": cached.merge(model, [first, second]),
        "select": cached.select(model, [first, second], [(0, 1), (1, 0)]),
    }
    assert states["extend"].lens == (40, 31) and states["merge"].lens == (40, 40) and states["select"].lens == (20, 20)
    for name, state in states.items():
        got = cached.predict(model, state, qx, route="fused_summary")
        assert state.route == "fused_summary"
        want = cached.predict(model, state, qx, route="composed")
        err = U.rel_err(got, want)
        print(f"fused_summary predict {case} after {name}: {err:.2e} of mu's scale against the composed route on the same state")
        assert bool(torch.isfinite(got).all()) and err <= U.RTOL, name


@pytest.mark.parametrize("case", list(CASES))
def test_the_existing_routes_are_as_they_were(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="summary")
    cached.predict(model, state, qx, route="fused_summary")
    default = cached.predict(model, state, qx)
    assert state.route == "composed"
    assert torch.equal(default, cached.predict(model, state, qx, route="composed"))
    with pytest.raises(ValueError, match='route "fused"'):
        cached.predict(model, state, qx, route="fused")
    keys = cached.condition(model, cx[:, :15].contiguous(), cy[:, :15].contiguous())
    with pytest.raises(ValueError, match="this state is 'keys'"):
        cached.predict(model, keys, qx, route="fused_summary")
    cached.predict(model, keys, qx)
    assert keys.route == "fused"
