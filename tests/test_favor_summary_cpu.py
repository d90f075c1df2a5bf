"""The fixed-size FAVOR+ summary state without a GPU: the float64 streaming restatement tests/favor_summary_ref.py
against tests/favor_cached_ref.py on every input the GPU tests use, the host build's six entries, and every host-side refusal of the
new arguments (all raised before anything touches a GPU)."""
import ctypes as C
import importlib
import math
import types

import pytest
import torch

from tests import favor_summary_ref as S

CFGV = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
            n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
             tasks_per_batch=2)
MODELS = {
    "resnet_anp": ("ANP", dict(CFG3D, agg_mode="attention"), (3, 64, 64), 4),
    "resnet_cnp_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max"), (3, 64, 64), 4),
    "vanilla_anp": ("ANPShapeNet1D", dict(CFGV, agg_mode="attention", dim_r=64), (1, 128, 128), 3),
    "vanilla_cnp_mean": ("CNPShapeNet1D", dict(CFGV, agg_mode="mean", dim_r=100), (1, 128, 128), 3),
}


# ---- the streaming state against the per-shot form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("chunking", list(S.CHUNKINGS))
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_streamed_state_equals_attention_on_the_concatenated_shots(d, m, chunking, kind):
    c = S.case(kind, d, m, chunking)
    want = S.reference(c)
    st = S.streamed(c)
    assert st.cnt == c["totals"]
    got = st.query(c["q"], c["proj"])
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"streamed state {kind} d={d} m={m} {chunking}: {err:.2e} of out's scale")
    assert bool(torch.isfinite(got).all()) and err <= 1e-12
    if c["peak"] is not None:                       # the case is what it says: one key ~50 above every other
        dd = torch.einsum("thnd,md->thnm", d ** -0.25 * c["k"].double(), c["proj"].double())
        top = dd[c["peak"]].max().item()
        dd[c["peak"]] = -1e30
        assert abs(top - 50) < 1e-3 and abs(st.M - top) < 1e-12 and 45 < top - dd.max().item() < 55


def test_a_fresh_state_is_minus_infinity_and_zeros_and_stays_finite():
    c = S.case("live", 16, 16, "ragged")
    st = S.State(2, S.H, 16, 16)
    assert st.M == -math.inf and not st.A.any() and not st.a.any() and st.cnt == [0, 0]
    kc, vc, _ = c["chunks"][0]
    st.absorb(kc, vc, c["proj"], [0, 0])            # no valid shot: nothing moves, nothing turns NaN
    assert st.M == -math.inf and not st.A.any() and st.cnt == [0, 0]
    st.absorb(kc, vc, c["proj"], [5, 0])
    assert math.isfinite(st.M) and bool(torch.isfinite(st.A).all()) and st.cnt == [5, 0] and not st.A[1].any()


def test_every_chunking_gives_the_same_state():
    c = S.case("live", 64, 266, "7_32_31")
    st = S.streamed(c)
    one = S.State(2, S.H, 64, 266).absorb(c["k"], c["v"], c["proj"])
    for x, y in ((st.A, one.A), (st.a, one.a), (st.vs, one.vs)):
        assert (x - y).abs().max().item() <= 1e-12 * y.abs().max().item()
    assert st.M == one.M and st.cnt == one.cnt == [70, 70]


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_six_entries_and_they_are_unsupported(hostsim):
    c = hostsim.c
    assert c.mlhot_favor_summary_bytes(2, 2, 64, 266) == 0
    assert c.mlhot_favor_summary_ws_bytes(2, 2, 8, 64, 266) == 0
    assert c.mlhot_favor_summary_query_ws_bytes(2, 2, 5, 64, 266) == 0
    buf = torch.full((1024,), 7.0)
    p = C.c_void_p(buf.data_ptr())
    calls = {
        "favor_summary_init": lambda: c.mlhot_favor_summary_init(2, 2, 64, 266, p, 4096, None),
        "favor_summary_absorb": lambda: c.mlhot_favor_summary_absorb(p, p, p, None, 2, 2, 8, 64, 266, p, p, 4096, p, 4096, None),
        "favor_summary_query_fwd": lambda: c.mlhot_favor_summary_query_fwd(p, p, p, 2, 2, 5, 64, 266, p, p, 4096, None),
    }
    for name, call in calls.items():
        assert call() == 4, name                                    # MLHOT_ERR_UNSUPPORTED
        assert name in c.mlhot_last_error().decode(), (name, c.mlhot_last_error().decode())
    assert bool((buf == 7.0).all())
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError, match="favor_summary_init serves"):              # the wrapper refuses before it allocates
        hostsim.favor_summary_init(2, 2, 64, 266, "cpu")


# ---- host-side refusals -------------------------------------------------------------------------------------------------------------
def _model(name):
    method, cfg, img, L = MODELS[name]
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval(), img, L


@pytest.mark.parametrize("name", list(MODELS))
def test_condition_refusals_of_the_form_argument(name):
    from mlhot import cached
    model, img, L = _model(name)
    cx, cy = torch.rand(2, 4, *img), torch.rand(2, 4, L)
    entries = [lambda **kw: cached.condition(model, cx, cy, **kw)] + ([lambda **kw: model.condition(cx, cy, **kw)] if hasattr(model, "extend") else [])
    for cond in entries:
        for bad in ("rows", None, "SUMMARY", 1):
            with pytest.raises(ValueError, match="form must be one of"):
                cond(form=bad)
        if not model.ATTENTION:
            with pytest.raises(ValueError, match='form="summary" serves the attention models'):
                cond(form="summary")
            continue
        with pytest.raises(ValueError, match='form="summary" takes no capacity'):
            cond(form="summary", capacity=64)
        with pytest.raises(ValueError, match=r"ctx_len must lie in 1\.\.4"):
            cond(form="summary", ctx_len=[0, 4])
        with pytest.raises(ValueError, match="capacity = 33 is outside"):          # the default form keeps its cap
            cond(ctx_len=[1, 2], capacity=33)
    if model.ATTENTION:
        with pytest.raises(ValueError, match="at least one context shot"):
            cached.condition(model, cx[:, :0], cy[:, :0], form="summary")
        model.train()
        with pytest.raises(ValueError, match="eval"):
            cached.condition(model, cx, cy, form="summary")


def _summary_state(model, lens=(40, 31)):
    from mlhot.cached import VanillaContextState, _fingerprint
    from mlhot.ops import FavorKeyState
    from networks._resnet_np import ContextState, ResNetNP
    d = 256 if isinstance(model, ResNetNP) else 64
    keys = FavorKeyState("summary", (2, max(lens), 8, d, model.attn.projection_matrix.shape[0]), buf=None, lens=tuple(lens))
    if isinstance(model, ResNetNP):
        return ContextState(model, 2, max(lens), model._fingerprint(), "attention", keys=keys, lens=lens, form="summary")
    return VanillaContextState(model, 2, max(lens), _fingerprint(model), "attention", keys=keys, lens=lens, form="summary")


@pytest.mark.parametrize("name", ["resnet_anp", "vanilla_anp"])
def test_extend_and_predict_refusals_on_a_summary_state(name):
    from mlhot import cached
    model, img, L = _model(name)
    state = _summary_state(model)
    assert state.capacity is None and state.vh is None and state.kh is None and state.form == "summary"
    nx, ny, qx = torch.rand(2, 40, 1, 1, 1).expand(2, 40, *img), torch.rand(2, 40, L), torch.rand(2, 3, *img)
    with pytest.raises(ValueError, match=r"new_len must lie in 0\.\.40"):             # 40 more shots are no capacity problem; 41 of 40 slots are
        cached.extend(model, state, nx, ny, new_len=[41, 0])
    with pytest.raises(ValueError, match="new_len has 3 entries"):
        cached.extend(model, state, nx, ny, new_len=[1, 2, 3])
    other, _, _ = _model(name)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.extend(other, state, nx, ny)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(other, state, qx)
    if name == "vanilla_anp":
        with pytest.raises(ValueError, match='route "fused"'):
            cached.predict(model, state, qx, route="fused")
    with torch.no_grad():
        next(model.parameters()).add_(1.0)
    with pytest.raises(ValueError, match="stale"):
        cached.predict(model, state, qx)
    with pytest.raises(ValueError, match="stale"):
        cached.extend(model, state, nx, ny)


def test_favor_query_refuses_a_task_without_a_shot_and_favor_absorb_its_bad_arguments():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_absorb, favor_keys, favor_query
    q, proj = torch.zeros(2, 3, 2, 16), torch.zeros(16, 16)
    empty = FavorKeyState("summary", (2, 5, 2, 16, 16), buf=None, lens=(5, 0))
    with pytest.raises(MlhotError, match=r"has absorbed no shot \(shots per task: \[5, 0\]\)"):
        favor_query(q, empty, None, proj)
    with pytest.raises(MlhotError, match="no summary"):
        FavorKeyState("plain", (2, 5, 2, 16, 16), kh=q).summary()
    with pytest.raises(MlhotError, match="holds no key features"):
        empty.features()
    k = torch.zeros(2, 5, 2, 16)
    with pytest.raises(MlhotError, match="needs tensors on a ROCm device"):
        favor_absorb(None, k, k, proj)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_absorb(None, k.clone().requires_grad_(True), k, proj)
    with pytest.raises(MlhotError, match="needs tensors on a ROCm device"):        # favor_keys is as it was
        favor_keys(k, proj)
