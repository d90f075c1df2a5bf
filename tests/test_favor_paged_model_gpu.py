"""condition(form="paged") / extend / predict / leave_one_out on the MI355X, both families at 300 context shots -
beyond the long form's 256: predict against the model's own forward and against the summary form, growth in three steps against a
one-off condition, the attention read-out across the page edge, masks and leave-one-out.  The bars are the long and the masked model
tests' own: U.RTOL of mu's scale against forward, Nc 2^-23 for the row sum of the weights.  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import context_mask_ref as CM
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, NC, NQ, NLOO = 2, 300, 7, 260
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


def _plain(model, state, qx, **kw):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    return cached.predict(model, state, qx, **kw) if isinstance(model, ResNetNP) else cached.predict(model, state, qx, route="composed", **kw)


def _query_heads(model, call):
    """The query heads [T, H, Nq, d] (CPU) the one favor_query call of `call` saw, and call's result."""
    from mlhot import cached
    from networks import _resnet_np
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        for mod in (cached, _resnet_np):
            real = mod.favor_query
            mp.setattr(mod, "favor_query", lambda qh, *a, _real=real, **k: (seen.append(qh), _real(qh, *a, **k))[1])
        res = call()
    assert len(seen) == 1
    return seen[0].detach().cpu().permute(0, 2, 1, 3), res


def _cpu(t):
    return t.detach().cpu().permute(0, 2, 1, 3)


@pytest.mark.parametrize("case", list(CASES))
def test_predict_on_a_paged_state_is_the_forward_and_the_summary(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="paged")
    assert state.form == "paged" and state.lens == (NC, NC) and state.capacity == NC and state.Nc == NC
    assert state.keys.route == "paged" and state.kh.shape[:2] == (T, NC) and state.vh.shape == state.kh.shape
    with torch.no_grad():
        want = model(cx, cy, qx, test=True)[0]
    got = cached.predict(model, state, qx)
    err = U.rel_err(got, want)
    print(f"paged predict {case} {NC} shots, {NQ} targets: {err:.2e} of mu's scale against forward(test=True)")
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL
    serr = U.rel_err(got, cached.predict(model, cached.condition(model, cx, cy, form="summary"), qx))
    print(f"{case} {NC} shots: form paged against form summary {serr:.2e} of mu's scale")
    assert serr <= U.RTOL
    if case == "vanilla_anp":
        assert state.route == "composed"
        for route in ("fused", "fused_summary"):
            with pytest.raises(ValueError, match=f'route "{route}"'):
                cached.predict(model, state, qx, route=route)
    else:
        assert torch.equal(model.predict(model.condition(cx, cy, form="paged"), qx), got)            # the methods are the same calls
    assert torch.equal(cached.predict(model, state, qx, chunk=3), got)
    with pytest.raises(ValueError, match="has form 'paged'"):
        cached.merge(model, [state])


def _grown_and_once(case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    first = cached.condition(model, cx[:, :200].contiguous(), cy[:, :200].contiguous(), capacity=NC, form="paged")
    assert first.lens == (200, 200) and first.capacity == NC
    mid = cached.extend(model, first, cx[:, 200:260].contiguous(), cy[:, 200:260].contiguous())
    grown = cached.extend(model, mid, cx[:, 260:].contiguous(), cy[:, 260:].contiguous())
    assert mid.lens == (260, 260) and grown.lens == (NC, NC) and grown.form == "paged" and first.lens == (200, 200)
    return model, grown, cached.condition(model, cx, cy, form="paged"), cx, cy, qx


@pytest.mark.parametrize("case", list(CASES))
def test_extend_grows_a_paged_state_across_the_page_edge(gpulib, case):
    """The growth itself: lens, the capacity's refusal, and - given the SAME per-shot rows - the bits of a one-off state."""
    from mlhot import cached
    from mlhot.ops import favor_keys_paged, favor_query
    model, grown, once, cx, cy, qx = _grown_and_once(case)
    with pytest.raises(ValueError, match="would hold 301 context shots, the state's capacity is 300"):
        cached.extend(model, grown, cx[:, :1].contiguous(), cy[:, :1].contiguous())
    again = favor_keys_paged(grown.kh, model.attn.projection_matrix, lens=[NC, NC])          # the kept rows, conditioned in one piece
    for a, b in zip(again.features(), grown.keys.features()):
        assert torch.equal(a, b)
    assert U.rel_err(cached.predict(model, grown, qx), cached.predict(model, once, qx)) <= U.RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_extend_in_three_steps_equals_conditioning_on_all_shots(gpulib, case):
    """extend 200 + 60 + 40 is torch.equal to conditioning on 300: the paged form runs the Linears of its per-shot stage through the
    row-invariant kernel (mlhot.ops.linear_rows_any), the encoders are per image, and the paged kernels give equal bits on equal
    rows - so the per-shot rows, the key state and mu are the one-off state's, bit for bit."""
    from mlhot import cached
    model, grown, once, cx, cy, qx = _grown_and_once(case)
    got, want = cached.predict(model, grown, qx), cached.predict(model, once, qx)
    print(f"paged extend {case} 200 + 60 + 40 against condition on {NC}: {U.rel_err(got, want):.2e} of mu's scale, "
          f"key rows equal: {torch.equal(grown.kh, once.kh)}, value rows equal: {torch.equal(grown.vh, once.vh)}")
    assert torch.equal(grown.kh, once.kh) and torch.equal(grown.vh, once.vh)
    for x, y in zip(grown.keys.features(), once.keys.features()):
        assert torch.equal(x, y)
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_attention_across_the_page_edge(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    lens, cap = (NC, 257), 320
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap, form="paged")
    mu, attn = cached.predict(model, state, qx, return_attention=True)
    heads = state.kh.shape[2]
    assert attn.shape == (T, heads, NQ, cap) and attn.dtype == torch.float32
    assert torch.equal(mu, _plain(model, state, qx))
    assert bool(torch.isfinite(attn).all()) and float(attn.min()) >= 0.0
    for t, L in enumerate(lens):
        assert bool((attn[t, :, :, L:] == 0.0).all()) and float(attn[t, :, :, :L].min()) > 0.0, t
    excess = float((attn.double().sum(dim=-1) - 1.0).abs().max())
    print(f"paged predict(return_attention=True) {case} ctx_len={lens} of {cap} slots: |sum_n attn - 1| {excess:.2e} "
          f"({excess / AC.rowsum_bound(cap):.2f} of the bound)")
    assert excess <= AC.rowsum_bound(cap)
    cmu, cattn = cached.predict(model, state, qx, chunk=3, return_attention=True)
    assert torch.equal(cmu, mu) and torch.equal(cattn, attn)
    qh, _ = _query_heads(model, lambda: cached.predict(model, state, qx, return_attention=True))
    w64 = AR.weights(qh, _cpu(state.kh), model.attn.projection_matrix.detach().cpu(), state.keys.lens)
    err = U.rel_err(attn, w64)
    print(f"paged predict(return_attention=True) {case}: attn {err:.2e} of its scale against float64 on the model's head projections")
    assert err <= U.RTOL


@pytest.mark.parametrize("case", list(CASES))
def test_masks_have_the_bits_of_the_calls_they_stand_for(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    state = cached.condition(model, cx, cy, form="paged")
    ones = torch.ones(T, NQ, NC, dtype=torch.bool, device=DEV)
    mu1 = cached.predict(model, state, qx, context_mask=ones)
    assert mu1.shape[:2] == (T, NQ) and torch.equal(mu1, _plain(model, state, qx))              # all True: the unmasked call
    mk = torch.rand(T, 3, NQ, NC, generator=torch.Generator().manual_seed(2)) < 0.5
    mk[..., 0] = True
    mk[:, 1, :, :256] = False                                                                     # a group that drops the whole first page
    mk = mk.to(DEV)
    mu = cached.predict(model, state, qx, context_mask=mk)
    assert mu.shape == (T, 3, NQ, mu1.shape[-1]) and mu.is_contiguous()
    for g in range(3):                                                                            # a 4-D mask is its G 3-D calls
        assert torch.equal(mu[:, g], cached.predict(model, state, qx, context_mask=mk[:, g])), g
    assert torch.equal(cached.predict(model, state, qx, context_mask=mk, chunk=3), mu)            # chunked = unchunked
    mu_a, attn = cached.predict(model, state, qx, context_mask=mk, return_attention=True)
    assert torch.equal(mu_a, mu) and attn.shape == (T, 3, state.kh.shape[2], NQ, NC)
    keep = mk[:, :, None].expand_as(attn)
    assert bool((attn[~keep] == 0.0).all()) and float(attn[keep].min()) > 0.0
    assert float((attn.double().sum(dim=-1) - 1.0).abs().max()) <= NC * 2.0 ** -23


def _peak_slot(model, state):
    """tests/test_context_mask_model_gpu.py's: the slot of the shot whose dd_k is the key stabiliser M, in float64"""
    kh = state.kh.detach().cpu().double()
    valid = torch.arange(state.Nc)[None, :] < torch.tensor(state.lens)[:, None]
    dd = torch.einsum("tnhd,md->tnhm", kh.shape[-1] ** -0.25 * kh, model.attn.projection_matrix.detach().cpu().double())
    dd = torch.where(valid[:, :, None, None], dd, torch.full((), -float("inf"), dtype=torch.float64))
    return int(dd.amax(dim=(0, 2, 3)).argmax())


@pytest.mark.parametrize("case", list(CASES))
def test_leave_one_out_is_predict_on_the_sub_context(gpulib, case):
    """DESIGN.md 6c-10's reasoning, at 260 shots: the masked call keeps the state's stabiliser M.  A group that drops a shot which
    does not hold M is compared with predict on the sub-context (the same M on both sides) at U.RTOL, the bar predict has against
    forward; the group that drops the shot that holds M would meet another M there, which moves FAVOR+'s 1e-4 floors (6c-6), so it
    is held to the float64 statement under the state's M instead - on the attention weights, from the model's own query heads."""
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    cx, cy = cx[:, :NLOO].contiguous(), cy[:, :NLOO].contiguous()
    state = cached.condition(model, cx, cy, form="paged")
    loo = cached.leave_one_out(model, state, qx)
    assert loo.shape[:3] == (T, NLOO, NQ) and bool(torch.isfinite(loo).all())
    peak = _peak_slot(model, state)
    others = [c for c in (3, 258, 259) if c != peak][:2]                # a slot of the first page, one of the second
    for c in others:
        keep = [n for n in range(NLOO) if n != c]
        sub = cached.condition(model, cx[:, keep].contiguous(), cy[:, keep].contiguous(), form="paged")
        err = U.rel_err(loo[:, c], _plain(model, sub, qx))
        print(f"leave_one_out {case} {NLOO} shots without slot {c} (stabiliser in slot {peak}): {err:.2e} of mu's scale against predict on the sub-context")
        assert err <= U.RTOL, c
    no_peak = torch.ones(T, 1, NQ, NLOO, dtype=torch.bool, device=DEV)
    no_peak[..., peak] = False
    qh, (mu, attn) = _query_heads(model, lambda: cached.predict(model, state, qx, context_mask=no_peak, return_attention=True))
    assert torch.equal(mu[:, 0], loo[:, peak])
    _, w64 = CM.masked(qh, _cpu(state.kh), _cpu(state.vh), model.attn.projection_matrix.detach().cpu(), no_peak.cpu())
    err = U.rel_err(attn, w64)
    print(f"leave_one_out {case} without the stabiliser's slot {peak}: attn {err:.2e} of its scale against float64 under the state's M")
    assert err <= U.RTOL and bool((attn[..., peak] == 0.0).all())
    assert torch.equal(cached.leave_one_out(model, state, qx, chunk=3), loo)


@pytest.mark.parametrize("k0,k1,n", [(3, 0, 16), (64, 16, 100), (256, 4, 256), (64, 3, 100)])
def test_the_per_shot_linears_do_not_depend_on_the_row_count(gpulib, k0, k1, n):
    """mlhot.ops.linear_rows_any, what the paged per-shot stage runs: a last source of any width (zero columns pad it), the value of
    the plain Linear, and bits per row that are the same alone, in a slice either side of 512 rows and among 600."""
    from mlhot.ops import linear_rows_any
    g = torch.Generator().manual_seed(k0 + k1 + n)
    xs = [torch.randn(600, k, generator=g).to(DEV) for k in (k0, k1) if k]
    w, b = torch.randn(n, k0 + k1, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    full = linear_rows_any([(x, 1, 0) for x in xs], w, b, "relu")
    want = torch.relu(torch.cat(xs, dim=1).double().cpu() @ w.double().cpu().T + b.double().cpu())
    err = U.rel_err(full, want)
    print(f"linear_rows_any [{k0} | {k1}] -> {n}: {err:.2e} of its scale against float64")
    assert full.shape == (600, n) and err <= U.RTOL
    for lo, hi in ((0, 1), (0, 400), (400, 520), (83, 600)):
        assert torch.equal(linear_rows_any([(x[lo:hi].contiguous(), 1, 0) for x in xs], w, b, "relu"), full[lo:hi]), (lo, hi)
