"""Whole models above 32 context shots with the option "favor_linear" on against the same model with it off (favor.h's chain, the
route these shapes take without the option and which the oracle tests cover up to 25 + 30 shots): loss, mu and every parameter gradient
within U.RTOL of the tensor's own scale.  The _W_q / _W_k gradients are floored at the _W_v gradients' scale: at initialisation they
are rounding residue, as in the existing whole-model parity tests.  Run on the MI355X box:  pytest tests -m gpu"""
import importlib
import types

import pytest
import torch
import torch.nn.functional as F

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _anp1d():
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2,
                                agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d")
    g = torch.Generator().manual_seed(7)
    cx, qx = torch.rand(2, 40, 1, 128, 128, generator=g), torch.rand(2, 35, 1, 128, 128, generator=g)
    cy, qy = torch.rand(2, 40, 3, generator=g), torch.rand(2, 35, 3, generator=g)
    return "ANPShapeNet1D", cfg, (cx, cy, qx, qy), None


def _anp3d():
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                agg_mode="attention", img_agg="reshape", task="shapenet_3d", temperature=0.07)
    g = torch.Generator().manual_seed(4321)
    cx, qx = torch.rand(2, 34, 3, 64, 64, generator=g), torch.rand(2, 5, 3, 64, 64, generator=g)
    cy = F.normalize(torch.randn(2, 34, 4, generator=g), dim=-1)
    qy = F.normalize(torch.randn(2, 5, 4, generator=g), dim=-1)
    return "ANP", cfg, (cx, cy, qx, qy), None


def _step(model, cfg, batch):
    from trainer.losses import LossFunc
    cx, cy, qx, qy = (t.to(DEV) for t in batch)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(99)
    mu, var, kl = model(cx, cy, qx)
    loss = LossFunc("mse", cfg.task).calc_loss(mu, var, qy)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), mu.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("make", [_anp1d, _anp3d], ids=["anp_shapenet1d_40+35", "anp_shapenet3d_34+5"])
def test_model_step_linear_route_equals_the_chain(gpulib, make):
    from mlhot.ops import favor_route
    method, cfg, batch, dims = make()
    torch.manual_seed(cfg.seed)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
    gpulib.prof_begin(8192)
    try:
        gpulib.set_option("favor_linear", 1)
        if dims:
            assert favor_route(*dims) == "linear"
        loss1, mu1, g1 = _step(model, cfg, batch)
    finally:
        gpulib.set_option("favor_linear", 0)
        labels = {label for label, _ in gpulib.prof_end()}
    assert "favor.lin.ctx" in labels and "favor.lin.bwd.Gk" in labels and "favor.S" not in labels, "the model did not take the linear route"
    loss0, mu0, g0 = _step(model, cfg, batch)
    assert set(g0) == set(g1)
    print(f"favor_linear model {method}: loss {loss1.item():.6f} / {loss0.item():.6f}, mu {U.rel_err(mu1, mu0):.2e}")
    assert abs(loss1.item() - loss0.item()) <= U.RTOL * abs(loss0.item())
    assert U.rel_err(mu1, mu0) <= U.RTOL
    v_scale = max(g0[k].abs().max().item() for k in g0 if k.startswith("_W_v"))
    worst = (0.0, None)
    for k in g0:
        floor = v_scale if k.startswith("_W_q") or k.startswith("_W_k") else 0.0
        e = U.rel_err(g1[k], g0[k], floor)
        worst = max(worst, (e, k))
    print(f"favor_linear model {method}: worst gradient {worst[0]:.2e} ({worst[1]}) over {len(g0)} tensors")
    for k in g0:
        floor = v_scale if k.startswith("_W_q") or k.startswith("_W_k") else 0.0
        assert U.rel_err(g1[k], g0[k], floor) <= U.RTOL, k
