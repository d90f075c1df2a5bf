"""Cached-context inference for the vanilla family without a GPU: the float64 restatement of the query tail (tests/np_query_ref.py)
against the model's own torch modules applied as in the reference forward, and every refusal of mlhot.cached (all raised before any
kernel)."""
import importlib
import types

import pytest
import torch

from oracle import ref_cpu as O
from tests import np_query_ref as NR

CFG = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
           n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape")
CASES = {"anp": ("ANPShapeNet1D", "attention", 64), "cnp_mean": ("CNPShapeNet1D", "mean", 100), "cnp_max": ("CNPShapeNet1D", "max", 100),
         "cnp_baco": ("CNPShapeNet1D", "baco", 256)}


def _model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c)


def _vanilla(case):
    method, agg, dim_r = CASES[case]
    return _model(method, agg_mode=agg, dim_r=dim_r, **CFG)


def _module_chain(model, cx, cy, qx):
    """The reference forward, layer by layer, from the model's own torch modules (ANPShapeNet1D.py:93-157, CNPShapeNet1D.py:96-140);
    the FAVOR+ attention is the oracle's unsplit one.  -> (mu, x_ctx, x_qry)"""
    T, Nc, Nq = cx.shape[0], cx.shape[1], qx.shape[1]
    x_qry = model.encoder_w0(qx.reshape(-1, 1, 128, 128)).reshape(T, Nq, -1)
    x_ctx = model.encoder_w0(cx.reshape(-1, 1, 128, 128)).reshape(T, Nc, -1) if Nc else torch.zeros(T, 0, model.dim_w, dtype=qx.dtype)
    if Nc == 0:
        z = torch.zeros(T, Nq, model.dim_z, dtype=qx.dtype)
    else:
        rs = model.encoder_r.layers(torch.cat([x_ctx, model.transform_y(cy)], dim=2))
        if model.ATTENTION:
            def heads(x, mods):
                return torch.stack([m.linear(x) for m in mods], dim=1)
            out = O.favor_attention(heads(x_qry, model._W_q), heads(x_ctx, model._W_k), heads(rs, model._W_v), model.attn.projection_matrix)
            z = model.r_to_z(model._W.linear(out.permute(0, 2, 3, 1).reshape(T, Nq, -1)))
        else:
            if model.agg_mode == "mean":
                r = rs.mean(dim=1)
            elif model.agg_mode == "max":
                r = rs.max(dim=1)[0]
            else:
                var = 1e-5 + torch.nn.functional.softplus(model.rs_to_var(rs))
                r = O.agg_baco(model.rs_to_mu(rs), var)[0]
            z = model.r_to_z(r)[:, None, :].expand(T, Nq, -1)
    return model.decoder0(torch.cat([x_qry, z], dim=-1)), x_ctx, x_qry


@pytest.mark.parametrize("Nc", [0, 5])
@pytest.mark.parametrize("case", list(CASES))
def test_restatement_equals_the_module_chain_in_float64(case, Nc):
    model = _vanilla(case).double().eval()
    g = torch.Generator().manual_seed(5)
    cx, qx = torch.rand(2, Nc, 1, 128, 128, generator=g).double(), torch.rand(2, 3, 1, 128, 128, generator=g).double()
    cy = torch.rand(2, Nc, 3, generator=g).double()
    with torch.no_grad():
        want, x_ctx, x_qry = _module_chain(model, cx, cy, qx)
        p = dict(model.state_dict())
        proj = p.get("attn.projection_matrix")
        state = NR.condition(p, x_ctx, cy, model.agg_mode, proj)
        assert state["kind"] == ("empty" if Nc == 0 else "attention" if model.ATTENTION else "latent")
        got = NR.query_tail(p, x_qry, state, model.OUT_TANH, proj)
        # row-wise in the targets: one row alone gives that row
        alone = NR.query_tail(p, x_qry[:, 1:2], state, model.OUT_TANH, proj)
    assert got.shape == want.shape == (2, 3, 2)
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    assert (alone - got[:, 1:2]).abs().max().item() <= 1e-14


def _state(model, T=2, kind="latent"):
    from mlhot.cached import VanillaContextState, _fingerprint
    return VanillaContextState(model, T, 3, _fingerprint(model), kind, z=torch.zeros(T, 64))


@pytest.mark.parametrize("case", ["anp", "cnp_max"])
def test_condition_and_predict_refusals(case):
    from mlhot import cached
    model = _vanilla(case)
    cx, cy, qx = torch.rand(2, 3, 1, 128, 128), torch.rand(2, 3, 3), torch.rand(2, 4, 1, 128, 128)
    model.train()
    with pytest.raises(ValueError, match="eval"):
        cached.condition(model, cx, cy)
    good = _state(model)
    with pytest.raises(ValueError, match="eval"):
        cached.predict(model, good, qx)
    model.eval()
    with pytest.raises(ValueError, match="tasks_per_batch"):
        cached.condition(model, cx[:1], cy[:1])
    other = _vanilla(case).eval()
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(other, good, qx)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(model, {"z": None}, qx)
    with pytest.raises(ValueError, match="same tasks"):
        cached.predict(model, good, qx[:1])
    with pytest.raises(ValueError, match="same tasks"):
        cached.predict(model, _state(model, T=1), qx[:1])
    with pytest.raises(ValueError, match="chunk"):
        cached.predict(model, good, qx, chunk=0)
    with pytest.raises(ValueError, match="at least one target"):
        cached.predict(model, good, qx[:, :0])
    with pytest.raises(ValueError, match="route"):
        cached.predict(model, good, qx, route="eager")
    with torch.no_grad():
        model.r_to_z.bias.add_(1.0)                   # a weight update in place, as an optimizer step does
    with pytest.raises(ValueError, match="stale"):
        cached.predict(model, good, qx)
    assert not hasattr(type(model), "condition") and not hasattr(type(model), "predict")        # the classes gain no attribute


def test_bridges_refuse_cpu_tensors():
    from mlhot import cached
    from mlhot.binding import MlhotError
    model = _vanilla("cnp_mean").eval()
    cx, cy, qx = torch.rand(2, 3, 1, 128, 128), torch.rand(2, 3, 3), torch.rand(2, 4, 1, 128, 128)
    with pytest.raises(MlhotError, match="ROCm device"):
        cached.condition(model, cx, cy)
    with pytest.raises(MlhotError, match="ROCm device"):
        cached.predict(model, _state(model), qx)
    with pytest.raises(MlhotError, match="ROCm device"):
        cached.predict(model, _state(model), qx, route="composed")


@pytest.mark.parametrize("method,agg", [("ANPMRShapeNet1D", "attention"), ("CNPMRShapeNet1D", "mean")])
def test_bayes_by_backprop_twins_refuse(method, agg):
    from mlhot import cached
    mr = _model(method, agg_mode=agg, dim_r=64, **CFG).eval()
    ok, reason = cached.supports(mr)
    assert not ok and "fresh weights in every forward" in reason
    with pytest.raises(ValueError, match=method + ".*fresh weights"):
        cached.condition(mr, torch.rand(2, 2, 1, 128, 128), torch.rand(2, 2, 3))
    with pytest.raises(ValueError, match=method + ".*fresh weights"):
        cached.predict(mr, None, torch.rand(2, 2, 1, 128, 128))


def test_other_classes_refuse_as_not_built():
    from mlhot import cached
    lin = torch.nn.Linear(4, 4).eval()
    assert cached.supports(lin) == (False, "cached-context inference is not built for this class")
    with pytest.raises(ValueError, match="Linear.*not built"):
        cached.condition(lin, torch.rand(1, 1, 4), torch.rand(1, 1, 4))
    with pytest.raises(ValueError, match="Linear.*not built"):
        cached.predict(lin, None, torch.rand(1, 1, 4))


def test_supports_answers_for_each_family():
    from mlhot import cached
    assert cached.supports(_vanilla("anp"))[0] and cached.supports(_vanilla("cnp_baco"))[0]
    assert "mlhot_np_query_fwd" in cached.supports(_vanilla("anp"))[1]
    resnet = _model("CondNeuralProcess", tasks_per_batch=2, agg_mode="max", **CFG3D)
    assert cached.supports(resnet) == (True, "ResNetNP.condition / predict")
    mr3d = _model("ANPMRShapeNet3D", tasks_per_batch=1, agg_mode="attention", **CFG3D)
    ok, reason = cached.supports(mr3d)
    assert not ok and "fresh weights" in reason


def test_resnet_instances_go_through_their_own_methods():
    from mlhot import cached
    model = _model("CondNeuralProcess", tasks_per_batch=2, agg_mode="max", **CFG3D).eval()
    calls = []
    model.condition = lambda cx, cy: calls.append(("condition", cx, cy)) or "the state"
    model.predict = lambda state, qx, chunk=None: calls.append(("predict", state, qx, chunk)) or "mu"
    assert cached.condition(model, "cx", "cy") == "the state"
    assert cached.predict(model, "the state", "qx", chunk=3) == "mu"
    assert calls == [("condition", "cx", "cy"), ("predict", "the state", "qx", 3)]
    with pytest.raises(ValueError, match="route"):
        cached.predict(model, "the state", "qx", route="composed")
