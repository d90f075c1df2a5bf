"""Prefix sweep without a GPU: the numpy statement of the prefix operators against the oracle on sliced inputs, the oracle helper
against the reference's own per-k outputs, the evaluator's protocol with a stub model, and the refusals."""
import importlib
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import prefix_ref as P
from tests import util as U


# ---- the numpy statement of the operators against the oracle on sliced inputs -----------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max", "baco"])
def test_numpy_agg_prefixes_against_the_oracle_on_every_prefix(mode):
    g = torch.Generator().manual_seed(3)
    rs, lv = torch.randn(3, 7, 16, generator=g, dtype=torch.float64), torch.randn(3, 7, 16, generator=g, dtype=torch.float64) * 3
    got = P.agg_prefixes_np(mode, rs, lv)
    assert got.shape == (7, 3, 16)
    for k in range(1, 8):
        want = (O.agg_mean(rs[:, :k]) if mode == "mean" else O.agg_max(rs[:, :k]) if mode == "max"
                else O.agg_baco(rs[:, :k], 1e-5 + F.softplus(lv[:, :k]))[0])
        assert U.rel_err(got[k - 1], want) <= 1e-12, (mode, k)


@pytest.mark.parametrize("scales", [(0.5, 0.5), (0.3, "climb"), (0.3, "first")])
def test_numpy_favor_prefixes_against_the_oracle_on_every_prefix(scales):
    """FAVOR+ with the key stabiliser per prefix (max over the FIRST k shots of every task): float64, against oracle.ref_cpu's
    favor_attention on k[:, :, :kk], v[:, :, :kk] - incl. keys whose maximum climbs from shot to shot and keys whose maximum sits
    in the first shot (M_k constant)."""
    g = torch.Generator().manual_seed(9)
    T, H, Nq, Nc, d, m = 2, 3, 4, 6, 16, 40
    q = torch.randn(T, H, Nq, d, generator=g, dtype=torch.float64) * scales[0]
    k = torch.randn(T, H, Nc, d, generator=g, dtype=torch.float64) * 0.5
    if scales[1] == "climb":
        k = k * (1.6 ** torch.arange(Nc, dtype=torch.float64))[None, None, :, None]
    elif scales[1] == "first":
        k[:, :, 0] *= 6.0
    v = torch.randn(T, H, Nc, d, generator=g, dtype=torch.float64)
    proj = torch.randn(m, d, generator=g, dtype=torch.float64)
    M = P.favor_stabilisers_np(k, proj)
    assert np.all(np.diff(M) >= 0)
    if scales[1] == "climb":
        assert np.all(np.diff(M) > 0)
    if scales[1] == "first":
        assert np.all(M == M[0])
    got = P.favor_prefixes_np(q, k, v, proj)
    for kk in range(1, Nc + 1):
        want = O.favor_attention(q, k[:, :, :kk], v[:, :, :kk], proj)
        assert U.rel_err(got[kk - 1], want) <= 1e-10, kk
        dd = torch.einsum("thnd,md->thnm", d ** -0.25 * k[:, :, :kk], proj)
        assert abs(M[kk - 1] - dd.max().item()) <= 1e-12 * max(1.0, abs(M[kk - 1]))


# ---- the oracle helper against the reference's own outputs per context size ---------------------------------------------------------
@pytest.mark.parametrize("name", ["p_anp_shapenet3d", "p_cnp_shapenet3d_max"])
def test_oracle_prefix_helper_against_the_reference_fixtures(name):
    fx, meta = U.load_case(name)
    assert os.path.getsize(os.path.join(U.GOLDEN, name + ".npz")) < 1 << 20
    model = U.build_model(meta, "cpu", fx)
    p = {k: v.detach() for k, v in model.state_dict().items()}
    views = torch.from_numpy(fx["views_u8"]).float().div(255.0).permute(0, 1, 4, 2, 3).contiguous()
    labels = torch.from_numpy(fx["labels"])
    K = meta["K"]
    assert fx["mu"].shape == (K, meta["T"], meta["V"], meta["cfg"]["output_dim"])
    mu = P.forward_prefixes_ref(p, views[:, :K], labels[:, :K], views, meta["cfg"]["agg_mode"], meta["cfg"]["img_agg"])
    for k in range(K):
        assert U.rel_err(mu[k], fx["mu"][k]) <= U.RTOL, (name, k + 1)
    assert U.rel_err(mu[0], fx["mu"][K - 1]) > U.RTOL, "the context size must matter for this check to mean something"


# ---- the evaluator's protocol, with a stub model --------------------------------------------------------------------------------
class StubModel(torch.nn.Module):
    """A model whose output depends on every context shot and target, with forward_prefixes = one plain forward per k."""

    def __init__(self, out_dim):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.0, out_dim))
        self.calls = []

    def forward(self, cx, cy, qx, test=False):
        self.calls.append(("forward", cx.shape[1]))
        s = cx.mean(dim=(1, 2, 3, 4)) + cy.mean(dim=(1, 2))
        return torch.tanh(qx.mean(dim=(2, 3, 4))[..., None] + s[:, None, None]) * self.w, None, 0

    def forward_prefixes(self, cx, cy, qx, ks=None):
        self.calls.append(("forward_prefixes", cx.shape[1]))
        ks = range(1, cx.shape[1] + 1) if ks is None else ks
        with torch.no_grad():
            s = [cx[:, :k].mean(dim=(1, 2, 3, 4)) + cy[:, :k].mean(dim=(1, 2)) for k in ks]
            return torch.stack([torch.tanh(qx.mean(dim=(2, 3, 4))[..., None] + sk[:, None, None]) * self.w for sk in s])


class NoPrefixModel(torch.nn.Module):
    def forward(self, cx, cy, qx, test=False):
        return qx.mean(dim=(2, 3, 4))[..., None].expand(-1, -1, 4), None, 0


class Recorder:
    """Passes a loader through and records every call made on it."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []
        self.val_rng, self.test_rng = inner.val_rng, inner.test_rng

    @property
    def test_counter(self):
        return self.inner.test_counter

    @test_counter.setter
    def test_counter(self, v):
        self.inner.test_counter = v

    def get_batch(self, source, tasks_per_batch, shot):
        self.calls.append(("get_batch", source, tasks_per_batch, shot))
        return self.inner.get_batch(source, tasks_per_batch, shot)


def _evaluate(tmp_path, tag, data, model=None, task="shapenet_3d", **extra):
    from evaluator.model_evaluator import ModelEvaluator
    log = []
    cfg = types.SimpleNamespace(device=torch.device("cpu"), tasks_per_batch=2, val_iters=3, max_ctx_num=4, task=task, contrastive=False,
                                logger=types.SimpleNamespace(info=log.append), save_path=str(tmp_path / tag), **extra)
    loss = types.SimpleNamespace(calc_loss=lambda mu, var, gt, test=False: O.calc_loss(task, mu, gt, test=test))
    model = StubModel(4 if task == "shapenet_3d" else 2) if model is None else model
    ev = ModelEvaluator(model=model, loss=loss, config=cfg, data=data)
    assert ev.ingest is None
    return ev, ev.evaluate(), log, model


def _views(**kw):
    from mlhot.synth import SyntheticViews
    return SyntheticViews("shapenet_3d", objects=4, views=8, **kw)


def test_prefix_sweep_writes_the_plain_sweeps_files_and_numbers(tmp_path):
    _, plain, _, m0 = _evaluate(tmp_path, "plain", _views())
    _, swept, log, m1 = _evaluate(tmp_path, "swept", _views(), prefix_sweep=True)
    assert swept == plain                                   # (means, stds) of validation and test, every context size: the same floats
    for f in ("val_losses.txt", "test_losses.txt"):
        a, b = (tmp_path / "plain" / f).read_text(), (tmp_path / "swept" / f).read_text()
        assert a == b and np.loadtxt(tmp_path / "swept" / f).shape == (4, 3)
    assert os.path.exists(tmp_path / "swept" / "models" / "model.pt")
    assert sum("reproduces the reference's draws" in m for m in log) == 2
    assert m0.calls == [("forward", k) for k in range(1, 5) for _ in range(2 * 3)]
    assert m1.calls == [("forward_prefixes", 4)] * (2 * 3)           # val_iters forwards per source instead of K * val_iters


def test_prefix_sweep_absent_or_false_leaves_the_loader_calls_as_they_are(tmp_path):
    today = [("get_batch", src, 2, k) for k in range(1, 5) for src in ("validation", "test") for _ in range(3)]
    rec = Recorder(_views())
    _evaluate(tmp_path, "absent", rec)
    assert rec.calls == today
    rec = Recorder(_views())
    _evaluate(tmp_path, "false", rec, prefix_sweep=False)
    assert rec.calls == today
    rec = Recorder(_views())
    _evaluate(tmp_path, "on", rec, prefix_sweep=True)
    per_source = lambda src: [("get_batch", src, 2, 1), ("get_batch", src, 2, 4)] + [("get_batch", src, 2, 4)] * 3
    assert rec.calls == per_source("validation") + per_source("test")


def test_prefix_sweep_refuses_loaders_without_the_prefix_property(tmp_path):
    from mlhot.synth import SyntheticData
    with pytest.raises(ValueError, match="not a prefix"):
        _evaluate(tmp_path, "train_mode", _views(mode="train"), prefix_sweep=True)
    with pytest.raises(ValueError, match="not a prefix"):
        _evaluate(tmp_path, "synthetic_1d", SyntheticData("shapenet_1d"), task="shapenet_1d", prefix_sweep=True)
    _, res, log, model = _evaluate(tmp_path, "paired", SyntheticData("shapenet_1d"), task="shapenet_1d", prefix_sweep="paired")
    assert sum("same tasks at every context size, not the reference's draws" in m for m in log) == 2
    assert len(res[0][0]) == 4 and all(np.isfinite(res[0][0])) and model.calls == [("forward_prefixes", 4)] * 6
    with pytest.raises(ValueError, match="prefix_sweep must be"):
        _evaluate(tmp_path, "bad_mode", _views(), prefix_sweep="yes")


def test_prefix_sweep_refuses_models_without_forward_prefixes(tmp_path):
    with pytest.raises(ValueError, match="no forward_prefixes"):
        _evaluate(tmp_path, "no_prefix", _views(), model=NoPrefixModel(), prefix_sweep=True)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _cpu_model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), seed=2578, temperature=0.07, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c)


def test_bayes_by_backprop_and_vanilla_models_refuse_the_prefix_sweep():
    x = torch.zeros(1, 2, 3, 64, 64)
    mr = _cpu_model("ANPMRShapeNet3D", task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=1, input_dim=4, output_dim=4,
                    agg_mode="attention", img_agg="reshape").eval()
    with pytest.raises(ValueError, match="fresh weights"):
        mr.forward_prefixes(x, torch.zeros(1, 2, 4), x)
    vanilla = dict(task="shapenet_1d", img_size=[128, 128, 1], tasks_per_batch=1, input_dim=3, output_dim=2, img_agg="", dim_w=64,
                   n_hidden_units_r=[100, 100], dim_z=64)
    x1 = torch.zeros(1, 2, 1, 128, 128)
    for method, agg, dim_r in (("ANPShapeNet1D", "attention", 64), ("CNPShapeNet1D", "mean", 100)):
        with pytest.raises(ValueError, match="vanilla 128x128x1 family"):
            _cpu_model(method, agg_mode=agg, dim_r=dim_r, **vanilla).eval().forward_prefixes(x1, torch.zeros(1, 2, 3), x1)
    with pytest.raises(ValueError, match="fresh weights"):
        _cpu_model("CNPMRShapeNet1D", agg_mode="mean", dim_r=100, **vanilla).eval().forward_prefixes(x1, torch.zeros(1, 2, 3), x1)


def test_prefix_operators_refuse_gradients_and_cpu_tensors():
    from mlhot.binding import MlhotError
    from mlhot.ops import agg_prefixes, favor_prefixes
    rs = torch.randn(2, 3, 8, requires_grad=True)
    with pytest.raises(MlhotError, match="forward-only"):
        agg_prefixes("mean", rs)
    with pytest.raises(MlhotError, match="ROCm device"):
        agg_prefixes("mean", rs.detach())
    q, kv, proj = torch.randn(1, 2, 2, 16, requires_grad=True), torch.randn(1, 3, 2, 16), torch.randn(32, 16)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_prefixes(q, kv, kv, proj)
    with torch.no_grad(), pytest.raises(MlhotError, match="ROCm device"):
        favor_prefixes(q, kv, kv, proj)


def test_resnet_family_forward_prefixes_checks_its_arguments_before_any_kernel():
    cnp = _cpu_model("CondNeuralProcess", task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=1, input_dim=4, output_dim=4,
                     agg_mode="max", img_agg="reshape")
    x = torch.zeros(1, 2, 3, 64, 64)
    with pytest.raises(ValueError, match="eval"):
        cnp.train().forward_prefixes(x, torch.zeros(1, 2, 4), x)
    with pytest.raises(ValueError, match="ks"):
        cnp.eval().forward_prefixes(x, torch.zeros(1, 2, 4), x, ks=[3])
    with pytest.raises(ValueError, match="at least one context shot"):
        cnp.eval().forward_prefixes(x[:, :0], torch.zeros(1, 0, 4), x)
