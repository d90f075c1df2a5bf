"""The top-k attention read-out without a GPU: the torch statement of the definition (tests/attention_topk_ref.py)
against float64 over the case table, the tie and padding rules, why values but not indices are comparable with a top-k over w, and
every refusal of favor_query(topk=) and predict(top_k=) - raised on the host before a tensor reaches a kernel."""
import importlib
import types

import pytest
import torch

from tests import attention_topk_cases as TC
from tests import attention_topk_ref as TR
from tests import favor_cached_ref as R
from tests import ragged_ref as RR
from tests import util as U

T, H = TC.T, TC.H


def _scores64(q, k, proj, lens):
    """The un-normalised S [T, H, Nq, Nc] of the float64 read-out (tests/attention_readout_ref.weights divides it by its row sum)"""
    fk = R.key_features(k, proj)[0] if lens is None else RR.key_features(k, proj, lens)[0]
    return torch.einsum("thnm,thcm->thnc", R.query_features(q, proj), fk)


def _kernel_statement(S32, lens, k):
    """What the kernels are defined to do, in fp32 torch: rank the valid slots by S, divide the k chosen by the row's D"""
    T_, _, _, Nc = S32.shape
    D = torch.zeros(S32.shape[:3], dtype=torch.float32)
    for c in range(Nc):                                                            # D's own order: the columns ascending
        keep = torch.tensor([c < n for n in TR.valid_counts(lens, T_, Nc)])[:, None, None]
        D = torch.where(keep, D + S32[..., c], D)
    idx, s = TR.topk_of(S32, lens, k)
    wk = torch.where(idx >= 0, s / D[..., None], torch.zeros(()))
    return idx.int(), wk, S32 / D[..., None]


@pytest.mark.parametrize("form,Nc,m,lens", TC.CASES, ids=[TC.case_id(c) for c in TC.CASES])
def test_the_statement_against_float64(form, Nc, m, lens):
    q, k, _, p, _ = TC.inputs(Nc, m)
    S64 = _scores64(q, k, p, lens)
    w64 = S64 / S64.sum(dim=-1, keepdim=True)
    for kk in TC.KS:
        idx, wk, w32 = _kernel_statement(S64.float(), lens, kk)
        TR.check_shape_rules(idx, wk, lens, Nc, kk)
        # the VALUES are those of a top-k over w, whichever of two equal w the indices name
        assert torch.equal(wk, TR.topk_of(w32, lens, kk)[1]) and torch.equal(wk, TR.gather_at(w32, idx))
        at = TR.gather_at(w64, idx.long())
        assert U.rel_err(wk, at) <= U.RTOL and U.rel_err(wk, TR.topk_of(w64, lens, kk)[1]) <= U.RTOL


def test_ties_go_to_the_lower_slot_and_padding_is_exact():
    s = torch.tensor([[[[3.0, 7.0, 7.0, 1.0, 7.0, 9.0]]], [[[2.0, 2.0, 2.0, 2.0, 5.0, 5.0]]]])
    idx, val = TR.topk_of(s, (5, 3), 4)
    assert idx.tolist() == [[[[1, 2, 4, 0]]], [[[0, 1, 2, -1]]]]                 # 9.0 and the 5.0s lie behind lens
    assert val.tolist() == [[[[7.0, 7.0, 7.0, 3.0]]], [[[2.0, 2.0, 2.0, 0.0]]]]
    idx, val = TR.topk_of(s, None, 16)                                           # k > Nc
    assert idx[0, 0, 0].tolist() == [5, 1, 2, 4, 0, 3] + [-1] * 10 and idx[1, 0, 0].tolist() == [4, 5, 0, 1, 2, 3] + [-1] * 10
    assert bool((val[..., 6:] == 0.0).all()) and not bool(torch.signbit(val[..., 6:]).any())
    assert TR.gather_at(s, idx)[0, 0, 0, :7].tolist() == [9.0, 7.0, 7.0, 7.0, 3.0, 1.0, 0.0]


def test_division_by_the_rows_d_keeps_the_order_but_may_merge_neighbours():
    """S / D is monotone in S: ranking by S and dividing k numbers gives the values of a top-k over w.  Two neighbouring S can round
    to ONE w, and then a top-k over w (ties to the lower slot) may name the other slot: indices are comparable through the gather
    only."""
    g = torch.Generator().manual_seed(5)
    S = torch.rand(4, 2, 64, 48, generator=g) + 0.5
    up = torch.nextafter(S[..., 7], torch.full((), 9.0))
    S[..., 30] = up                                                              # slot 30 one ulp above slot 7
    D = S.sum(dim=-1, keepdim=True)
    w = S / D
    idx, s = TR.topk_of(S, None, 16)
    assert torch.equal(s / D, TR.topk_of(w, None, 16)[1]) and torch.equal(s / D, TR.gather_at(w, idx))
    merged = w[..., 30] == w[..., 7]
    assert bool(merged.any()) and bool((S[..., 30] > S[..., 7]).all())           # the premise: some pairs did round together
    by_w = TR.topk_of(w, None, 48)[0]
    by_s = TR.topk_of(S, None, 48)[0]
    pos = lambda order, c: (order == c).nonzero()[:, -1].reshape(order.shape[:3])
    assert bool((pos(by_s, 30) < pos(by_s, 7)).all())                            # by S: 30 always first
    assert bool((pos(by_w, 7) < pos(by_w, 30))[merged].all())                    # by w: the tie goes to slot 7


# ---- favor_query(topk=) ----------------------------------------------------------------------------------------------------------
def test_favor_query_topk_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_query
    qh, kh, proj = torch.randn(1, 5, 2, 16), torch.randn(1, 3, 2, 16), torch.randn(32, 16)
    cached = FavorKeyState("cached", (1, 3, 2, 16, 32), buf=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="topk= with weights=True.*never stored"):
        favor_query(qh, cached, kh, proj, weights=True, topk=3)
    with pytest.raises(ValueError, match="topk= with mask=.*no reduced form"):
        favor_query(qh, cached, kh, proj, mask=torch.ones(1, 5, 3, dtype=torch.bool), topk=3)
    with pytest.raises(ValueError, match="topk= with mass=.*one per call"):
        favor_query(qh, cached, kh, proj, mass=True, topk=3)
    for bad in (0, 17, -1, True, False, 2.0, "3", (3,)):
        with pytest.raises(ValueError, match=r"topk must be an integer in 1 \.\. 16"):
            favor_query(qh, cached, kh, proj, topk=bad)
    summary = FavorKeyState("summary", (1, 3, 2, 16, 32), buf=torch.zeros(16, dtype=torch.uint8), lens=(3,))
    with pytest.raises(MlhotError, match="topk= - a summary state keeps no per-shot rows"):
        favor_query(qh, summary, None, proj, topk=3)
    plain = FavorKeyState("plain", (1, 40, 2, 16, 32), kh=torch.randn(1, 40, 2, 16))
    with pytest.raises(MlhotError, match=r"topk= needs the cached kernels' envelope \(Nc <= 32"):
        favor_query(qh, plain, torch.randn(1, 40, 2, 16), proj, topk=3)
    with pytest.raises(MlhotError, match="ROCm device"):                       # a served state gets as far as asking for the device
        favor_query(qh, cached, kh, proj, topk=3)


def test_the_three_entries_are_declared_once_and_alike():
    from mlhot.binding import SIGNATURES
    keys, long_, paged = (SIGNATURES[f"mlhot_favor_query_{f}topk_fwd"] for f in ("", "long_", "paged_"))
    assert long_ == paged and len(long_[1]) == len(keys[1]) + 1                # lens is the one argument more
    assert len(keys[1]) == len(SIGNATURES["mlhot_favor_query_fwd"][1]) + 3     # k, idx, wk


# ---- predict(top_k=): the entry checks -------------------------------------------------------------------------------------------
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape")
CFG1D = dict(img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", input_dim=3, output_dim=2)


def _cpu_model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), seed=2578, temperature=0.07, tasks_per_batch=2, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval()


def _attention_state(model, heads, d, route="cached", form="keys"):
    """A hand-built attention state of `model` with three context slots - enough for every check that precedes the first launch."""
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    m = model.attn.projection_matrix.shape[0]
    keys = FavorKeyState(route, (2, 3, heads, d, m), buf=torch.zeros(16, dtype=torch.uint8), lens=(3, 3) if form == "summary" else None)
    rows = None if form == "summary" else torch.zeros(2, 3, heads, d)
    return ContextState(model, 2, 3, fingerprint(model), "attention", keys=keys, vh=rows, kh=rows, form=form, lens=(3, 3))


def _common_refusals(predict, state, qx):
    with pytest.raises(ValueError, match="top_k= with return_attention=True.*never stored"):
        predict(state, qx, top_k=3, return_attention=True)
    with pytest.raises(ValueError, match="top_k= with context_mask=.*no reduced form"):
        predict(state, qx, top_k=3, context_mask=torch.ones(2, 4, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="top_k= with attention_mass=True.*one per call"):
        predict(state, qx, top_k=3, attention_mass=True)
    for bad in (0, 17, -2, True, False, 3.0, "3", [3], torch.tensor(3)):
        with pytest.raises(ValueError, match=r"top_k must be an integer in 1 \.\. 16"):
            predict(state, qx, top_k=bad)
    with pytest.raises(ValueError, match="chunk must be a positive"):
        predict(state, qx, top_k=3, chunk=0)
    with pytest.raises(ValueError, match="same tasks"):
        predict(state, qx[:1], top_k=3)


def test_resnet_predict_refuses_before_any_launch():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, 4, 3, 64, 64)
    cnp = _cpu_model("CondNeuralProcess", agg_mode="max", **CFG3D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 256), rs=torch.zeros(2, 3, 256))
    empty = ContextState(cnp, 2, 0, fingerprint(cnp), "empty")
    for state in (latent, empty):
        with pytest.raises(ValueError, match="top_k= - .*has no attention"):
            cnp.predict(state, qx, top_k=3)
        with pytest.raises(ValueError, match="top_k= - .*has no attention"):
            cached.predict(cnp, state, qx, top_k=3)
    anp = _cpu_model("ANP", agg_mode="attention", **CFG3D)
    summary = _attention_state(anp, 8, 256, route="summary", form="summary")
    with pytest.raises(ValueError, match="top_k= - a summary state keeps no per-shot rows"):
        anp.predict(summary, qx, top_k=3)
    with pytest.raises(ValueError, match="top_k= needs the cached kernels' envelope"):
        anp.predict(_attention_state(anp, 8, 256, route="plain"), qx, top_k=3)
    with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
        cached.predict(anp, _attention_state(anp, 8, 256), qx, route="composed", top_k=3)
    with pytest.raises(ValueError, match="not made by this model"):
        anp.predict(latent, qx, top_k=3)
    state = _attention_state(anp, 8, 256)
    _common_refusals(anp.predict, state, qx)
    _common_refusals(lambda s, x, **kw: cached.predict(anp, s, x, **kw), state, qx)
    anp.train()
    with pytest.raises(ValueError, match="eval"):
        anp.predict(state, qx, top_k=3)


def test_vanilla_predict_refuses_before_any_launch():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, 4, 1, 128, 128)
    anp = _cpu_model("ANPShapeNet1D", agg_mode="attention", dim_r=64, **CFG1D)
    state = _attention_state(anp, 8, 64)
    for route in ("fused", "fused_summary"):
        with pytest.raises(ValueError, match=f'top_k= with route "{route}"'):
            cached.predict(anp, state, qx, route=route, top_k=3)
    with pytest.raises(ValueError, match="route must be one of"):
        cached.predict(anp, state, qx, route="both", top_k=3)
    summary = _attention_state(anp, 8, 64, route="summary", form="summary")
    with pytest.raises(ValueError, match="top_k= - a summary state keeps no per-shot rows"):
        cached.predict(anp, summary, qx, top_k=3)
    cnp = _cpu_model("CNPShapeNet1D", agg_mode="mean", dim_r=100, **CFG1D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 64), rs=torch.zeros(2, 3, 100))
    with pytest.raises(ValueError, match="top_k= - .*has no attention"):
        cached.predict(cnp, latent, qx, top_k=3)
    _common_refusals(lambda s, x, **kw: cached.predict(anp, s, x, **kw), state, qx)
    # the read-out's and the mass's own refusals keep their words
    with pytest.raises(ValueError, match='return_attention=True with route "fused"'):
        cached.predict(anp, state, qx, route="fused", return_attention=True)
    with pytest.raises(ValueError, match='attention_mass=True with route "fused"'):
        cached.predict(anp, state, qx, route="fused", attention_mass=True)
