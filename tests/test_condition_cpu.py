"""Cached-context inference without a GPU: the float64 restatement of the split FAVOR+ against the oracle's unsplit one, and every
refusal of the new bridges and of ResNetNP.condition / predict (all raised before any kernel)."""
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import favor_cached_ref as R
from tests import util as U


def _fixture_cases():
    out = []
    fx = np.load(os.path.join(U.GOLDEN, "favor.npz"))
    for tag in json.loads(str(fx["meta"])):
        out.append((tag, tuple(torch.from_numpy(fx[f"{tag}/{n}"]) for n in ("q", "k", "v", "proj"))))
    fx = np.load(os.path.join(U.GOLDEN, "favor_c5.npz"))
    for tag in json.loads(str(fx["meta"])):
        out.append((tag, tuple(torch.from_numpy(fx[f"{tag}/{n}"]) for n in ("q", "k", "v")) + (torch.from_numpy(fx["proj"]),)))
    return out


@pytest.mark.parametrize("tag,case", _fixture_cases(), ids=[t for t, _ in _fixture_cases()])
def test_split_restatement_equals_the_unsplit_oracle_in_float64(tag, case):
    q, k, v, proj = (t.double() for t in case)
    want = O.favor_attention(q, k, v, proj)
    got = R.attention(q, k, v, proj)
    assert U.rel_err(got, want) <= 1e-12
    fk, M = R.key_features(k, proj)
    assert U.rel_err(fk, O.favor_features(k, proj, False)) <= 1e-13
    # row-wise in the queries: one row alone, and the rows in another order, give the same rows
    assert U.rel_err(R.query(q[:, :, 2:3], fk, v, proj), got[:, :, 2:3]) <= 1e-14
    assert U.rel_err(R.query(q.flip(2), fk, v, proj).flip(2), got) <= 1e-14


def test_large_norm_case_sits_on_the_floor():
    """favor.npz's d64_big: most key features are the 1e-4 floor - the regime the value tests must cover."""
    fx = np.load(os.path.join(U.GOLDEN, "favor.npz"))
    k, proj = torch.from_numpy(fx["d64_big/k"]), torch.from_numpy(fx["d64_big/proj"])
    fk, _ = R.key_features(k, proj)
    floor = proj.shape[0] ** -0.5 * 1e-4
    assert (fk < 2 * floor).double().mean().item() > 0.5


def test_bridges_refuse_cpu_tensors_and_gradients():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_keys, favor_query
    kh, proj = torch.randn(1, 3, 2, 16), torch.randn(32, 16)
    with pytest.raises(MlhotError, match="ROCm device"):
        favor_keys(kh, proj)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_keys(kh.clone().requires_grad_(True), proj)
    with torch.no_grad(), pytest.raises(MlhotError, match="ROCm device"):
        favor_keys(kh.clone().requires_grad_(True), proj)
    state = FavorKeyState("plain", (1, 3, 2, 16, 32), kh=kh)
    qh = torch.randn(1, 5, 2, 16)
    with pytest.raises(MlhotError, match="ROCm device"):
        favor_query(qh, state, kh, proj)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_query(qh.clone().requires_grad_(True), state, kh, proj)
    with pytest.raises(MlhotError, match="route 'plain'"):
        state.features()


CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape")


def _cpu_model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), seed=2578, temperature=0.07, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c)


@pytest.mark.parametrize("method,agg", [("ANP", "attention"), ("CondNeuralProcess", "max")])
def test_condition_and_predict_refusals(method, agg):
    from networks._resnet_np import ContextState
    model = _cpu_model(method, tasks_per_batch=2, agg_mode=agg, **CFG3D)
    cx, cy, qx = torch.rand(2, 3, 3, 64, 64), torch.rand(2, 3, 4), torch.rand(2, 4, 3, 64, 64)
    model.train()
    with pytest.raises(ValueError, match="eval"):
        model.condition(cx, cy)
    good = ContextState(model, 2, 3, model._fingerprint(), "latent", z=torch.zeros(2, 256))
    with pytest.raises(ValueError, match="eval"):
        model.predict(good, qx)
    model.eval()
    with pytest.raises(ValueError, match="tasks_per_batch"):
        model.condition(cx[:1], cy[:1])
    other = _cpu_model(method, tasks_per_batch=2, agg_mode=agg, **CFG3D).eval()
    with pytest.raises(ValueError, match="not made by this model"):
        other.predict(good, qx)
    with pytest.raises(ValueError, match="not made by this model"):
        model.predict({"z": None}, qx)
    with pytest.raises(ValueError, match="same tasks"):
        model.predict(good, qx[:1])
    with pytest.raises(ValueError, match="same tasks"):
        model.predict(ContextState(model, 1, 3, model._fingerprint(), "latent", z=torch.zeros(1, 256)), qx[:1])
    with pytest.raises(ValueError, match="chunk"):
        model.predict(good, qx, chunk=0)
    with torch.no_grad():
        model.mu.bias.add_(1.0)                       # a weight update in place, as an optimizer step does
    with pytest.raises(ValueError, match="stale"):
        model.predict(good, qx)


def test_bayes_by_backprop_models_refuse():
    mr = _cpu_model("ANPMRShapeNet3D", tasks_per_batch=1, agg_mode="attention", **CFG3D).eval()
    with pytest.raises(ValueError, match="fresh weights"):
        mr.condition(torch.rand(1, 2, 3, 64, 64), torch.rand(1, 2, 4))
    with pytest.raises(ValueError, match="fresh weights"):
        mr.predict(None, torch.rand(1, 2, 3, 64, 64))


@pytest.mark.parametrize("method", ["ANPShapeNet1D", "CNPShapeNet1D", "ANPVanillaPascal1D", "CNPVanillaPascal1D", "FCLCNPShapeNet1D",
                                    "ANPMRShapeNet1D", "CNPMRShapeNet1D", "ANPMR", "CNPMR"])
def test_vanilla_classes_have_no_condition(method):
    cls = getattr(importlib.import_module("networks." + method), method)
    assert not hasattr(cls, "condition") and not hasattr(cls, "predict")


@pytest.mark.parametrize("method", ["ANP", "CondNeuralProcess", "ANPDistractor", "CNPDistractor", "FCLANP", "FCLCNPDistractor"])
def test_resnet_family_has_condition(method):
    cls = getattr(importlib.import_module("networks." + method), method)
    assert callable(cls.condition) and callable(cls.predict)
