"""The attention mass without a GPU: `fold32`, the kernels' documented fp32 order written in numpy
(tests/attention_mass_ref.py), against the float64 statement; prune's slot choice on hand-made masses; and every refusal of
favor_query(mass=True), predict(attention_mass=True) and prune - all raised on the host before any tensor reaches a kernel."""
import importlib
import types

import numpy as np
import pytest
import torch

from tests import attention_mass_cases as MC
from tests import attention_mass_ref as MR
from tests import attention_readout_ref as AR


# ---- fold32 against float64 ------------------------------------------------------------------------------------------------------
CPU_CASES = [c for c in MC.CASES if c[1] in (1, 32, 33, 257)]


@pytest.mark.parametrize("form,Nc,m,lens", CPU_CASES, ids=[MC.case_id(c) for c in CPU_CASES])
def test_fold32_agrees_with_the_float64_definition(form, Nc, m, lens):
    """w64 rounded to float32 stands for the read-out's w.  Plain sum: Nq - 1 adds of non-negative terms, |err| <= (Nq - 1) u |exact|
    to first order, u = 2^-24.  With tw one more rounding per term.  The bar is the GPU test's (Nq + 2) u, with the exact sum taken
    over the SAME float32 weights, so the rounding of w64 to float32 is not in it."""
    q, k, _, p, tw = MC.inputs(Nc, m)
    w64 = AR.weights(q, k, p, lens)
    assert float((MR.mass64(q, k, p, lens) - w64.sum(dim=2)).abs().max()) == 0.0
    assert float((MR.mass64(q, k, p, lens, tw) - (w64 * tw.double()[:, None, :, None]).sum(dim=2)).abs().max()) == 0.0
    w32 = w64.float()
    invalid = ~MC.valid(lens, Nc)[:, None, :].expand(MC.T, MC.H, Nc)
    for Nq in MC.NQS:
        for weight in (None, tw[:, :Nq]):
            got = MR.fold32(w32[:, :, :Nq], weight)
            want = MR.mass64_of(w32[:, :, :Nq], weight)
            assert got.dtype == torch.float32 and got.shape == (MC.T, MC.H, Nc)
            assert bool((got[invalid] == 0.0).all()) and bool((want[invalid] == 0.0).all())
            assert bool(((got.double() - want).abs() <= (Nq + 2) * 2.0 ** -24 * want).all()), (Nq, weight is None)
    # one tile, no weights, one row: the fold is the row itself, bit for bit
    assert torch.equal(MR.fold32(w32[:, :, :1]), w32[:, :, 0])


def test_fold32_is_two_level_and_chunk_invariant():
    """The order is tiles-then-fold, not one chain over all rows: the two differ in general, and the tile partials of pieces cut at
    multiples of 16 concatenate to the whole's."""
    g = torch.Generator().manual_seed(5)
    w = torch.rand(2, 2, 100, 7, generator=g)
    tw = torch.rand(2, 100, generator=g)
    whole = MR.tile_partials32(w, tw)
    assert whole.shape == (2, 2, 7, 7)
    for step in (16, 32, 48):
        pieces = [MR.tile_partials32(w[:, :, i:i + step], tw[:, i:i + step]) for i in range(0, 100, step)]
        assert np.array_equal(np.concatenate(pieces, axis=2), whole), step
    chain = np.zeros((2, 2, 7), dtype=np.float32)
    for n in range(100):
        chain = (chain + (tw.numpy()[:, None, n, None] * w.numpy()[:, :, n]).astype(np.float32)).astype(np.float32)
    assert not np.array_equal(chain, MR.fold_tiles32(whole))
    pieces = [MR.tile_partials32(w[:, :, i:i + 24]) for i in range(0, 100, 24)]                 # 24: a chunk that splits a tile
    assert np.concatenate(pieces, axis=2).shape[2] != MR.tile_partials32(w).shape[2]


# ---- prune's slot choice ---------------------------------------------------------------------------------------------------------
def test_prune_choice_on_hand_made_masses():
    from mlhot.context import prune_choice
    score = [[5.0, 1.0, 3.0, 1.0, 4.0, 9.0], [2.0, 2.0, 2.0, 2.0, 7.0, 7.0]]
    # slot 5 of task 0 and slots 4, 5 of task 1 lie behind lens: whatever they hold is never chosen, never dropped
    assert prune_choice(score, (5, 4), 3) == [[1, 3], [3]]                       # task 1: all equal, the lower indices stay
    assert prune_choice(score, (5, 4), (1, 2)) == [[1, 2, 3, 4], [2, 3]]         # per-task keep
    assert prune_choice(score, (5, 4), (4, 4)) == [[3], []]                      # the tie 1.0 == 1.0: slot 1 stays, slot 3 goes
    assert prune_choice(score, (5, 4), (5, 9)) == [[], []]                       # keep >= lens: untouched
    assert prune_choice(torch.tensor(score), (6, 6), 2) == [[1, 2, 3, 4], [0, 1, 2, 3]]
    assert prune_choice(np.array(score), (6, 6), torch.tensor([2, 6])) == [[1, 2, 3, 4], []]
    g = torch.Generator().manual_seed(3)
    for _ in range(20):                                                          # against the slow statement, ties included
        s = torch.randint(0, 4, (3, 12), generator=g).float()
        lens = tuple(int(x) for x in torch.randint(1, 13, (3,), generator=g))
        keep = [int(x) for x in torch.randint(1, 13, (3,), generator=g)]
        drop = prune_choice(s, lens, keep)
        assert drop == MR.prune_by_hand(s.tolist(), lens, keep)
        for t in range(3):
            kept = [c for c in range(lens[t]) if c not in drop[t]]
            assert kept == sorted(kept) and len(kept) == min(keep[t], lens[t])    # evict keeps the survivors in their order
            assert all(c < lens[t] for c in drop[t]) and drop[t] == sorted(set(drop[t]))


def test_prune_choice_refuses_a_bad_keep():
    from mlhot.context import prune_choice
    score = [[1.0, 2.0], [3.0, 4.0]]
    for keep, match in ((0, "at least 1"), ((1, 0), "at least 1"), (-1, "at least 1"), ((1,), "1 entries for 2 tasks"), (1.5, "int"),
                        ((1, 1.0), "integers"), (True, "integers"), ("ab", "integers")):
        with pytest.raises(ValueError, match=match):
            prune_choice(score, (2, 2), keep)


# ---- favor_query(mass=True) ------------------------------------------------------------------------------------------------------
def test_favor_query_mass_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_query
    qh, kh, proj = torch.randn(1, 5, 2, 16), torch.randn(1, 3, 2, 16), torch.randn(32, 16)
    cached = FavorKeyState("cached", (1, 3, 2, 16, 32), buf=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mass=True with weights=True.*never stored"):
        favor_query(qh, cached, kh, proj, weights=True, mass=True)
    with pytest.raises(ValueError, match="mass=True with mask=.*no reduced form"):
        favor_query(qh, cached, kh, proj, mask=torch.ones(1, 5, 3, dtype=torch.bool), mass=True)
    with pytest.raises(ValueError, match="target_weight= weighs the targets of mass=True"):
        favor_query(qh, cached, kh, proj, target_weight=torch.ones(1, 5))
    summary = FavorKeyState("summary", (1, 3, 2, 16, 32), buf=torch.zeros(16, dtype=torch.uint8), lens=(3,))
    with pytest.raises(MlhotError, match="mass=True - a summary state keeps no per-shot rows"):
        favor_query(qh, summary, None, proj, mass=True)
    plain = FavorKeyState("plain", (1, 40, 2, 16, 32), kh=torch.randn(1, 40, 2, 16))
    with pytest.raises(MlhotError, match=r"mass=True needs the cached kernels' envelope \(Nc <= 32"):
        favor_query(qh, plain, torch.randn(1, 40, 2, 16), proj, mass=True)
    with pytest.raises(MlhotError, match="ROCm device"):                       # a served state gets as far as asking for the device
        favor_query(qh, cached, kh, proj, mass=True)


def test_target_weight_is_checked_on_the_host():
    from mlhot.ops import target_weight_arg
    assert target_weight_arg("predict", None, 2, 4, "cpu", ValueError) is None
    ok = target_weight_arg("predict", torch.tensor([[0.0, 1.0, 2.5, 0.0]] * 2, dtype=torch.float64), 2, 4, "cpu", ValueError)
    assert ok.dtype == torch.float32 and ok.is_contiguous() and ok.shape == (2, 4)
    for bad, match in ((torch.ones(2, 5), r"\[T=2, Nq=4\]"), (torch.ones(4), r"\[T=2, Nq=4\]"), (torch.ones(2, 4, dtype=torch.int64), "floating-point"),
                       ([[1.0] * 4] * 2, "floating-point"), (torch.tensor([[1.0, -1e-9, 1.0, 1.0]] * 2), "finite and >= 0"),
                       (torch.tensor([[1.0, float("nan"), 1.0, 1.0]] * 2), "finite and >= 0"),
                       (torch.tensor([[1.0, float("inf"), 1.0, 1.0]] * 2), "finite and >= 0")):
        with pytest.raises(ValueError, match=match):
            target_weight_arg("predict", bad, 2, 4, "cpu", ValueError)


# ---- predict(attention_mass=True) and prune: the entry checks ----------------------------------------------------------------------
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


def _common_refusals(predict, prune, state, qx):
    with pytest.raises(ValueError, match="attention_mass=True with return_attention=True.*never"):
        predict(state, qx, attention_mass=True, return_attention=True)
    with pytest.raises(ValueError, match="attention_mass=True with context_mask=.*no reduced form"):
        predict(state, qx, attention_mass=True, context_mask=torch.ones(2, 4, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="target_weight= weighs the targets of attention_mass=True"):
        predict(state, qx, target_weight=torch.ones(2, 4))
    for chunk in (1, 8, 17, 24):
        with pytest.raises(ValueError, match="chunk must be a multiple of 16"):
            predict(state, qx, attention_mass=True, chunk=chunk)
    with pytest.raises(ValueError, match="chunk must be a positive"):
        predict(state, qx, attention_mass=True, chunk=0)
    for tw, match in ((torch.ones(2, 5), r"target_weight must be \[T=2, Nq=4\]"), (-torch.ones(2, 4), "finite and >= 0"),
                      (torch.full((2, 4), float("nan")), "finite and >= 0"), (torch.ones(2, 4, dtype=torch.int32), "floating-point")):
        with pytest.raises(ValueError, match=match):
            predict(state, qx, attention_mass=True, target_weight=tw)
        with pytest.raises(ValueError, match=match):
            prune(state, qx, 2, target_weight=tw)
    for keep in (0, (2, 0), (1,), 1.5):
        with pytest.raises(ValueError, match="prune: keep"):
            prune(state, qx, keep)
    with pytest.raises(ValueError, match="chunk must be a multiple of 16"):
        prune(state, qx, 2, chunk=8)
    with pytest.raises(ValueError, match="same tasks"):
        predict(state, qx[:1], attention_mass=True)
    with pytest.raises(ValueError, match="same tasks"):
        prune(state, qx[:1], 2)


def test_resnet_predict_and_prune_refuse_before_any_launch():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, 4, 3, 64, 64)
    cnp = _cpu_model("CondNeuralProcess", agg_mode="max", **CFG3D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 256), rs=torch.zeros(2, 3, 256))
    empty = ContextState(cnp, 2, 0, fingerprint(cnp), "empty")
    for state in (latent, empty):
        with pytest.raises(ValueError, match="attention_mass=True - .*has no attention"):
            cnp.predict(state, qx, attention_mass=True)
        with pytest.raises(ValueError, match="attention_mass=True - .*has no attention"):
            cached.predict(cnp, state, qx, attention_mass=True)
    with pytest.raises(ValueError, match="attention_mass=True - .*has no attention"):
        cached.prune(cnp, latent, qx, 2)
    with pytest.raises(ValueError, match="prune: the state holds no context shot"):
        cached.prune(cnp, empty, qx, 2)
    anp = _cpu_model("ANP", agg_mode="attention", **CFG3D)
    summary = _attention_state(anp, 8, 256, route="summary", form="summary")
    with pytest.raises(ValueError, match="attention_mass=True - a summary state keeps no per-shot rows"):
        anp.predict(summary, qx, attention_mass=True)
    with pytest.raises(ValueError, match="prune: a summary state keeps no per-shot rows"):
        cached.prune(anp, summary, qx, 2)
    with pytest.raises(ValueError, match="attention_mass=True needs the cached kernels' envelope"):
        anp.predict(_attention_state(anp, 8, 256, route="plain"), qx, attention_mass=True)
    with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
        cached.predict(anp, _attention_state(anp, 8, 256), qx, route="composed", attention_mass=True)
    with pytest.raises(ValueError, match="not made by this model"):
        anp.predict(latent, qx, attention_mass=True)
    state = _attention_state(anp, 8, 256)
    _common_refusals(anp.predict, lambda s, x, keep, **kw: cached.prune(anp, s, x, keep, **kw), state, qx)
    _common_refusals(lambda s, x, **kw: cached.predict(anp, s, x, **kw), lambda s, x, keep, **kw: cached.prune(anp, s, x, keep, **kw), state, qx)
    anp.train()
    with pytest.raises(ValueError, match="eval"):
        anp.predict(state, qx, attention_mass=True)
    with pytest.raises(ValueError, match="eval"):
        cached.prune(anp, state, qx, 2)


def test_vanilla_predict_and_prune_refuse_before_any_launch():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, 4, 1, 128, 128)
    anp = _cpu_model("ANPShapeNet1D", agg_mode="attention", dim_r=64, **CFG1D)
    state = _attention_state(anp, 8, 64)
    for route in ("fused", "fused_summary"):
        with pytest.raises(ValueError, match=f'attention_mass=True with route "{route}"'):
            cached.predict(anp, state, qx, route=route, attention_mass=True)
    with pytest.raises(ValueError, match="route must be one of"):
        cached.predict(anp, state, qx, route="both", attention_mass=True)
    summary = _attention_state(anp, 8, 64, route="summary", form="summary")
    with pytest.raises(ValueError, match="attention_mass=True - a summary state keeps no per-shot rows"):
        cached.predict(anp, summary, qx, attention_mass=True)
    with pytest.raises(ValueError, match="prune: a summary state keeps no per-shot rows"):
        cached.prune(anp, summary, qx, 2)
    cnp = _cpu_model("CNPShapeNet1D", agg_mode="mean", dim_r=100, **CFG1D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 64), rs=torch.zeros(2, 3, 100))
    with pytest.raises(ValueError, match="attention_mass=True - .*has no attention"):
        cached.predict(cnp, latent, qx, attention_mass=True)
    with pytest.raises(ValueError, match="attention_mass=True - .*has no attention"):
        cached.prune(cnp, latent, qx, 1)
    _common_refusals(lambda s, x, **kw: cached.predict(anp, s, x, **kw), lambda s, x, keep, **kw: cached.prune(anp, s, x, keep, **kw), state, qx)
    # the read-out's own refusals keep their words
    with pytest.raises(ValueError, match='return_attention=True with route "fused"'):
        cached.predict(anp, state, qx, route="fused", return_attention=True)
