"""The attention read-out without a GPU: the float64 statement of w = S / D (tests/attention_readout_ref.py) on every
input of the GPU value tests - non-negative, rows summing to 1, sum_n w v equal to favor_cached_ref.attention's out, exact zeros in
the masked columns - and the refusals of favor_query(weights=True) and predict(return_attention=True), all raised on the host before
any tensor is touched."""
import importlib
import types

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import ragged_ref as RR
from tests import util as U


# ---- the reference itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_reference_weights_are_a_distribution_that_gives_out(d, m, Nc, kind):
    _, _, v, _ = AC.inputs(kind, d, m, Nc)
    w, out = AC.want(kind, d, m, Nc)
    assert w.dtype == torch.float64 and w.shape == (AC.T, AC.H, AC.NQ, Nc)
    assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0
    assert float((w.sum(dim=-1) - 1.0).abs().max()) <= 1e-12
    assert U.rel_err(AR.apply(w, v), out) <= 1e-12
    if kind == "equal":                  # equal keys share the weight: 1 / Nc each
        assert float((w - 1.0 / Nc).abs().max()) <= 1e-12


@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_reference_masked_columns_are_exact_zeros(d, m, Nc):
    for lens in AC.masked_lens(Nc):
        q, kn, vz, p, w, out = AC.masked("live", d, m, Nc, lens)
        valid = RR.valid_mask(lens, Nc)[:, None, None, :].expand_as(w)
        assert bool(torch.isfinite(w).all()) and bool((w[~valid] == 0.0).all()) and float(w[valid].min()) > 0.0
        assert float((w.sum(dim=-1) - 1.0).abs().max()) <= 1e-12
        assert U.rel_err(AR.apply(w, vz), out) <= 1e-12
        # a task's weights are those against its own shots alone (the stabiliser still the ragged batch's): nothing leaks from a masked slot
        for t, L in enumerate(lens):
            fk = RR.key_features(AC.inputs("live", d, m, Nc)[1], p, lens)[0]
            alone = AR.weights_from_features(q[t:t + 1], fk[t:t + 1, :, :L], p)
            assert U.rel_err(w[t:t + 1, :, :, :L], alone) <= 1e-12


# ---- favor_query(weights=True) on states that keep no cached key features -------------------------------------------------------
def test_favor_query_weights_refuses_summary_and_plain_states():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_query
    qh, kh, proj = torch.randn(1, 5, 2, 16), torch.randn(1, 3, 2, 16), torch.randn(32, 16)
    summary = FavorKeyState("summary", (1, 3, 2, 16, 32), buf=torch.zeros(16, dtype=torch.uint8), lens=(3,))
    with pytest.raises(MlhotError, match="summary state keeps no per-shot rows"):
        favor_query(qh, summary, None, proj, weights=True)
    plain = FavorKeyState("plain", (1, 40, 2, 16, 32), kh=torch.randn(1, 40, 2, 16))
    with pytest.raises(MlhotError, match=r"envelope \(Nc <= 32"):
        favor_query(qh, plain, torch.randn(1, 40, 2, 16), proj, weights=True)
    # without the keyword the calls are what they were: they get as far as asking for the device
    with pytest.raises(MlhotError, match="ROCm device"):
        favor_query(qh, plain, torch.randn(1, 40, 2, 16), proj)
    with pytest.raises(MlhotError, match="ROCm device"):
        favor_query(qh, FavorKeyState("plain", (1, 3, 2, 16, 32), kh=kh), kh, proj, weights=False)


# ---- predict(return_attention=True): the entry checks ----------------------------------------------------------------------------
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


def test_resnet_predict_refuses_the_read_out_where_there_is_nothing_to_read():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, 4, 3, 64, 64)
    cnp = _cpu_model("CondNeuralProcess", agg_mode="max", **CFG3D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 256))
    empty = ContextState(cnp, 2, 0, fingerprint(cnp), "empty")
    for state in (latent, empty):
        with pytest.raises(ValueError, match="has no attention"):
            cnp.predict(state, qx, return_attention=True)
        with pytest.raises(ValueError, match="has no attention"):
            cached.predict(cnp, state, qx, return_attention=True)
    anp = _cpu_model("ANP", agg_mode="attention", **CFG3D)
    with pytest.raises(ValueError, match="summary state keeps no per-shot rows"):
        anp.predict(_attention_state(anp, 8, 256, route="summary", form="summary"), qx, return_attention=True)
    with pytest.raises(ValueError, match="envelope"):
        anp.predict(_attention_state(anp, 8, 256, route="plain"), qx, return_attention=True)
    with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
        cached.predict(anp, _attention_state(anp, 8, 256), qx, route="fused", return_attention=True)
    # the existing refusals are unchanged and come first
    with pytest.raises(ValueError, match="same tasks"):
        cnp.predict(latent, qx[:1], return_attention=True)
    with pytest.raises(ValueError, match="not made by this model"):
        anp.predict(latent, qx, return_attention=True)
    with pytest.raises(ValueError, match="chunk"):
        cnp.predict(latent, qx, chunk=0, return_attention=True)
    cnp.train()
    with pytest.raises(ValueError, match="eval"):
        cnp.predict(latent, qx, return_attention=True)


def test_vanilla_predict_refuses_the_fused_route_and_models_without_attention():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, 4, 1, 128, 128)
    anp = _cpu_model("ANPShapeNet1D", agg_mode="attention", dim_r=64, **CFG1D)
    state = _attention_state(anp, 8, 64)
    with pytest.raises(ValueError, match='route "fused".*composed route'):
        cached.predict(anp, state, qx, route="fused", return_attention=True)
    with pytest.raises(ValueError, match="route must be one of"):
        cached.predict(anp, state, qx, route="both", return_attention=True)
    with pytest.raises(ValueError, match="summary state keeps no per-shot rows"):
        cached.predict(anp, _attention_state(anp, 8, 64, route="summary", form="summary"), qx, return_attention=True)
    cnp = _cpu_model("CNPShapeNet1D", agg_mode="mean", dim_r=100, **CFG1D)
    latent = ContextState(cnp, 2, 3, fingerprint(cnp), "latent", z=torch.zeros(2, 64))
    with pytest.raises(ValueError, match="has no attention"):
        cached.predict(cnp, latent, qx, return_attention=True)
    with pytest.raises(ValueError, match="has no attention"):
        cached.predict(cnp, latent, qx, route="composed", return_attention=True)
    with pytest.raises(ValueError, match="same tasks"):
        cached.predict(cnp, latent, qx[:1], return_attention=True)
    anp.train()
    with pytest.raises(ValueError, match="eval"):
        cached.predict(anp, state, qx, return_attention=True)
