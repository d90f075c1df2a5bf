"""Shared targets without a GPU: the case table covers every edge the kernels of csrc/favor_shared.h have, the float64
reference on the broadcast query is the per-task reference on the expanded one, the two entries are declared like the entries they
extend, and every refusal of favor_query(shared=True) and predict(shared_targets=True) is raised on the host before a tensor reaches a
kernel."""
import importlib
import types

import pytest
import torch

from tests import shared_query_cases as SC


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_edge():
    by_form = {f: [c for c in SC.CASES if c[0] == f] for f in ("cached", "long")}
    assert {c[1] for c in SC.CASES} == {1, 2, 5}                                       # T
    assert SC.NQS == [1, 15, 16, 17, 33] and SC.NQ == 33
    assert {c[2] for c in by_form["cached"] if (c[3], c[4]) != SC.DM_BIG} == {1, 31, 32}
    assert {c[2] for c in by_form["long"]} == {33, 64, 65, 256}
    for dm in SC.DM:
        for form, ncs in (("cached", {1, 31, 32}), ("long", {33, 64, 65, 256})):
            assert {c[2] for c in by_form[form] if (c[3], c[4]) == dm} == ncs, (form, dm)
        for form in by_form:
            mine = [c for c in by_form[form] if (c[3], c[4]) == dm]
            assert any(c[5] is None for c in mine) and any(c[5] is not None for c in mine), (form, dm)     # with and without lens
            assert any(c[5] is not None and 1 in c[5] for c in mine), (form, dm)                             # a task with a single shot
            assert {c[1] for c in mine} == {1, 2, 5}, (form, dm)
    assert set(SC.DM) == {(16, 16), (64, 266)}
    assert [c for c in SC.CASES if (c[3], c[4]) == (256, 1419)] == [("cached", 2, 15, 256, 1419, None, 17)]
    for form, T, Nc, d, m, lens, nq in SC.CASES:
        assert (Nc <= 32) == (form == "cached") and Nc <= 256 and nq <= SC.NQ
        assert lens is None or (len(lens) == T and all(1 <= n <= Nc for n in lens) and min(lens) < Nc)
    # a ragged long case whose tasks end in different 32-slot chunks, and one that crosses the last chunk edge
    assert any(c[0] == "long" and c[5] and len({(n - 1) // 32 for n in c[5]}) >= 3 for c in SC.CASES)
    assert any(c[0] == "long" and c[5] and max(c[5]) > 224 for c in SC.CASES)
    # task groups: one task each, a group that does not divide T = 5, all tasks, the library's choice
    assert SC.TASK_GROUPS == (1, 2, "T", 0)
    assert {c[0] for c in SC.POISON_CASES} == {"cached", "long"} and all(c[5] is not None for c in SC.POISON_CASES)
    assert all(torch.isfinite(torch.tensor(x)) and x != 0.0 for x in SC.POISON.values())
    assert len({SC.case_id(c) for c in SC.CASES}) == len(SC.CASES)


@pytest.mark.parametrize("case", [c for c in SC.CASES if (c[3], c[4]) == (16, 16)] + [SC.CASES[len(SC.SHAPES) + 2], SC.CASES[len(SC.SHAPES) + 7]],
                         ids=SC.case_id)
def test_the_reference_on_the_broadcast_query_is_the_per_task_reference_on_the_expanded_one(case):
    form, T, Nc, d, m, lens, _ = case
    q, k, v, p = SC.inputs(form, T, Nc, d, m)
    qb = SC.broadcast(q, T)
    assert qb.shape == (T, SC.H, SC.NQ, d) and (T == 1 or qb.stride(0) == 0) and qb.data_ptr() == q.data_ptr()      # a view of the one copy
    w, out = SC.want(form, T, Nc, d, m, lens)
    w2, out2 = SC.reference_for(qb.contiguous(), k, v, p, form, lens)
    assert w.dtype == torch.float64 and w.shape == (T, SC.H, SC.NQ, Nc) and out.shape == (T, SC.H, SC.NQ, d)
    assert torch.equal(w, w2) and torch.equal(out, out2)
    # every task alone, its own rows: the reference is row-wise in q and per task given the batch's stabiliser
    assert torch.allclose(w.sum(dim=-1), torch.ones(()).double(), atol=1e-12)
    if lens is not None:
        for t, L in enumerate(lens):
            assert not bool(w[t, :, :, L:].any()) and float(w[t, :, :, :L].min()) > 0.0
    # what stands behind lens[t] goes nowhere: the kernels' operands (NaN in k; zeros, NaN or the poison in v) give the same reference
    for poison in (None, SC.POISON[form]):
        _, kn, vp, _ = SC.operands(form, T, Nc, d, m, lens, poison)
        if lens is not None:
            assert bool(torch.isnan(kn).any())
            if form == "long":                                                          # the chunked reference never reads those rows
                w3, out3 = SC.reference_for(qb, kn, vp, p, form, lens)
                assert torch.equal(w3, w) and torch.equal(out3, out)


# ---- the ABI table -------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_like_the_entries_they_extend():
    from mlhot.binding import SIGNATURES
    keys, long_ = SIGNATURES["mlhot_favor_query_shared_fwd"], SIGNATURES["mlhot_favor_query_long_shared_fwd"]
    assert len(long_[1]) == len(keys[1]) + 1                                          # lens is the one argument more
    assert len(long_[1]) == len(SIGNATURES["mlhot_favor_query_long_fwd"][1]) + 1      # task_group
    assert len(keys[1]) == len(SIGNATURES["mlhot_favor_query_weights_fwd"][1]) + 1
    assert SIGNATURES["mlhot_favor_query_shared_ws_bytes"] == SIGNATURES["mlhot_favor_query_long_shared_ws_bytes"] == SIGNATURES["mlhot_favor_query_ws_bytes"]


def test_the_host_build_reports_the_shapes_as_unserved(hostsim):
    assert hostsim.c.mlhot_favor_query_shared_ws_bytes(2, 8, 17, 15, 64, 266) == 0      # GPU build only, like the entries they extend
    assert hostsim.c.mlhot_favor_query_long_shared_ws_bytes(2, 8, 17, 65, 64, 266) == 0


# ---- favor_query(shared=True) --------------------------------------------------------------------------------------------------------
def test_favor_query_shared_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_query
    qh, q4, kh, proj = torch.randn(5, 2, 16), torch.randn(2, 5, 2, 16), torch.randn(2, 3, 2, 16), torch.randn(32, 16)
    buf = torch.zeros(16, dtype=torch.uint8)
    cached = FavorKeyState("cached", (2, 3, 2, 16, 32), buf=buf)
    with pytest.raises(MlhotError, match="shared=True with mask="):
        favor_query(qh, cached, kh, proj, mask=torch.ones(2, 5, 3, dtype=torch.bool), shared=True)
    with pytest.raises(MlhotError, match="shared=True with mass="):
        favor_query(qh, cached, kh, proj, mass=True, shared=True)
    with pytest.raises(MlhotError, match="shared=True with mass="):
        favor_query(qh, cached, kh, proj, mass="tiles", shared=True)
    with pytest.raises(MlhotError, match="shared=True with target_weight="):
        favor_query(qh, cached, kh, proj, target_weight=torch.ones(2, 5), shared=True)
    with pytest.raises(MlhotError, match="shared=True with topk="):
        favor_query(qh, cached, kh, proj, topk=3, shared=True)
    for route, extra in (("summary", dict(lens=(3, 3))), ("paged", {}), ("plain", dict(kh=kh))):
        state = FavorKeyState(route, (2, 3, 2, 16, 32), buf=buf, **extra)
        with pytest.raises(MlhotError, match=f"shared=True serves .* this state's route is '{route}'"):
            favor_query(qh, state, kh, proj, shared=True)
        with pytest.raises(MlhotError, match=f"route is '{route}'"):
            favor_query(qh, state, kh, proj, weights=True, shared=True)
    with pytest.raises(MlhotError, match="state must come from favor_keys"):
        favor_query(qh, buf, kh, proj, shared=True)
    for bad in (-1, True, 1.0, "2"):
        with pytest.raises(MlhotError, match="task_group must be an integer >= 0"):
            favor_query(qh, cached, kh, proj, shared=True, task_group=bad)
    with pytest.raises(MlhotError, match="task_group= groups the tasks of shared=True"):
        favor_query(q4, cached, kh, proj, task_group=2)
    for state in (cached, FavorKeyState("long", (2, 3, 2, 16, 32), buf=buf)):
        with pytest.raises(MlhotError, match="ROCm device"):                       # a served state gets as far as asking for the device
            favor_query(qh, state, kh, proj, shared=True)
        with pytest.raises(MlhotError, match="ROCm device"):
            favor_query(qh, state, kh, proj, weights=True, shared=True, task_group=2)
    with pytest.raises(MlhotError, match="ROCm device"):                           # shared=False is the call it always was
        favor_query(q4, cached, kh, proj)


# ---- predict(shared_targets=True): the entry checks ------------------------------------------------------------------------------------
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


def _common_refusals(predict, state, qx, qx_tasks):
    """`predict(state, qx, **kw)` with shared_targets=True inside; qx [Nq, ...], qx_tasks the same images with a task axis"""
    with pytest.raises(ValueError, match="shared_targets=True with context_mask="):
        predict(state, qx, context_mask=torch.ones(2, 4, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="shared_targets=True with attention_mass=True"):
        predict(state, qx, attention_mass=True)
    with pytest.raises(ValueError, match="shared_targets=True with target_weight="):
        predict(state, qx, target_weight=torch.ones(2, 4))
    with pytest.raises(ValueError, match="shared_targets=True with top_k="):
        predict(state, qx, top_k=3)
    with pytest.raises(ValueError, match=r"shared_targets=True takes qry_x \[Nq, .*no task axis.*got \(2, 4, "):
        predict(state, qx_tasks)
    with pytest.raises(ValueError, match="no task axis"):
        predict(state, qx_tasks[:, :1])                                    # [T, 1, ...] is a task axis too, not T targets
    with pytest.raises(ValueError, match="chunk must be a positive"):
        predict(state, qx, chunk=0)
    with pytest.raises(ValueError, match="at least one target"):
        predict(state, qx[:0])


def test_resnet_predict_refuses_before_any_launch():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qt = torch.rand(2, 4, 3, 64, 64)
    qx = qt[0]
    cnp = _cpu_model("CondNeuralProcess", agg_mode="max", **CFG3D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 256), rs=torch.zeros(2, 3, 256))
    with pytest.raises(ValueError, match="has no attention"):
        cnp.predict(latent, qx, return_attention=True, shared_targets=True)
    anp = _cpu_model("ANP", agg_mode="attention", **CFG3D)
    for form, route in (("summary", "summary"), ("paged", "paged")):
        state = _attention_state(anp, 8, 256, route=route, form=form)
        for call in (lambda: anp.predict(state, qx, shared_targets=True), lambda: cached.predict(anp, state, qx, shared_targets=True),
                     lambda: anp.predict(state, qx, shared_targets=True, return_attention=True)):
            with pytest.raises(ValueError, match=f"shared_targets=True serves .*this state is a '{form}' state"):
                call()
    with pytest.raises(ValueError, match="shared_targets=True needs the cached kernels' envelope.*'plain'"):
        anp.predict(_attention_state(anp, 8, 256, route="plain"), qx, shared_targets=True)
    with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
        cached.predict(anp, _attention_state(anp, 8, 256), qx, route="composed", shared_targets=True)
    with pytest.raises(ValueError, match="not made by this model"):
        anp.predict(latent, qx, shared_targets=True)
    state = _attention_state(anp, 8, 256)
    _common_refusals(lambda s, x, **kw: anp.predict(s, x, shared_targets=True, **kw), state, qx, qt)
    _common_refusals(lambda s, x, **kw: cached.predict(anp, s, x, shared_targets=True, **kw), state, qx, qt)
    with torch.no_grad():
        next(anp.parameters()).add_(1.0)                                   # a weight update: the state is stale
    with pytest.raises(ValueError, match="stale"):
        anp.predict(state, qx, shared_targets=True)
    with pytest.raises(ValueError, match="stale"):                         # ... as for the plain call
        anp.predict(state, qt)
    state = _attention_state(anp, 8, 256)
    anp.train()
    with pytest.raises(ValueError, match="eval"):
        anp.predict(state, qx, shared_targets=True)


def test_vanilla_predict_refuses_before_any_launch():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qt = torch.rand(2, 4, 1, 128, 128)
    qx = qt[0]
    anp = _cpu_model("ANPShapeNet1D", agg_mode="attention", dim_r=64, **CFG1D)
    state = _attention_state(anp, 8, 64)
    for route in ("fused", "fused_summary"):
        with pytest.raises(ValueError, match=f'shared_targets=True with route "{route}"'):
            cached.predict(anp, state, qx, route=route, shared_targets=True)
    with pytest.raises(ValueError, match="route must be one of"):
        cached.predict(anp, state, qx, route="both", shared_targets=True)
    for form in ("summary", "paged"):
        with pytest.raises(ValueError, match=f"this state is a '{form}' state"):
            cached.predict(anp, _attention_state(anp, 8, 64, route=form, form=form), qx, shared_targets=True)
    cnp = _cpu_model("CNPShapeNet1D", agg_mode="mean", dim_r=100, **CFG1D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 64), rs=torch.zeros(2, 3, 100))
    with pytest.raises(ValueError, match="has no attention"):
        cached.predict(cnp, latent, qx, return_attention=True, shared_targets=True)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(anp, latent, qx, shared_targets=True)
    _common_refusals(lambda s, x, **kw: cached.predict(anp, s, x, shared_targets=True, **kw), state, qx, qt)
    assert cached.predict.__defaults__[-1] is False                       # the keyword is opt-in
    with pytest.raises(ValueError, match="same tasks"):                    # without it, a tensor without a task axis is refused as before
        cached.predict(anp, state, qx)
    cnp.train()
    with pytest.raises(ValueError, match="eval"):
        cached.predict(cnp, latent, qx, shared_targets=True)


@pytest.mark.parametrize("method,agg,cfg,shape", [("ANPMRShapeNet1D", "attention", dict(CFG1D, dim_r=64), (4, 1, 128, 128)),
                                                  ("CNPMRShapeNet1D", "mean", dict(CFG1D, dim_r=64), (4, 1, 128, 128)),
                                                  ("ANPMRShapeNet3D", "attention", CFG3D, (4, 3, 64, 64))])
def test_bayes_by_backprop_classes_refuse(method, agg, cfg, shape):
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    mr = _cpu_model(method, agg_mode=agg, **cfg)
    state = ContextState(mr, 2, 0, fingerprint(mr), "empty")
    with pytest.raises(ValueError, match=method + ".*fresh weights"):
        cached.predict(mr, state, torch.rand(*shape), shared_targets=True)
