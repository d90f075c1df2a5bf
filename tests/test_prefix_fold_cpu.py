"""The folded prefix sweep without a GPU: argument checks in front of any kernel, the forward-only bridges' refusals, the
evaluator's config.prefix_sweep_fold switch with stub models, mlhot_loss_prefix_fwd in the host build, the row map's statement."""
import importlib
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import linear_rows_ref as R


# ---- forward_prefixes(fold=True): the existing refusals come first ------------------------------------------------------------------
def _cpu_model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), seed=2578, temperature=0.07, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c)


def test_folded_forward_prefixes_checks_its_arguments_before_any_kernel():
    cnp = _cpu_model("CondNeuralProcess", task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=1, input_dim=4, output_dim=4,
                     agg_mode="max", img_agg="reshape")
    x = torch.zeros(1, 2, 3, 64, 64)
    with pytest.raises(ValueError, match="eval"):
        cnp.train().forward_prefixes(x, torch.zeros(1, 2, 4), x, fold=True)
    with pytest.raises(ValueError, match="ks"):
        cnp.eval().forward_prefixes(x, torch.zeros(1, 2, 4), x, ks=[3], fold=True)
    with pytest.raises(ValueError, match="at least one context shot"):
        cnp.eval().forward_prefixes(x[:, :0], torch.zeros(1, 0, 4), x, fold=True)


def test_bayes_by_backprop_and_vanilla_models_refuse_the_folded_sweep_too():
    x = torch.zeros(1, 2, 3, 64, 64)
    mr = _cpu_model("ANPMRShapeNet3D", task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=1, input_dim=4, output_dim=4,
                    agg_mode="attention", img_agg="reshape").eval()
    with pytest.raises(ValueError, match="fresh weights"):
        mr.forward_prefixes(x, torch.zeros(1, 2, 4), x, fold=True)
    vanilla = dict(task="shapenet_1d", img_size=[128, 128, 1], tasks_per_batch=1, input_dim=3, output_dim=2, img_agg="", dim_w=64,
                   n_hidden_units_r=[100, 100], dim_z=64)
    x1 = torch.zeros(1, 2, 1, 128, 128)
    with pytest.raises(ValueError, match="vanilla 128x128x1 family"):
        _cpu_model("CNPShapeNet1D", agg_mode="mean", dim_r=100, **vanilla).eval().forward_prefixes(x1, torch.zeros(1, 2, 3), x1, fold=True)


# ---- the bridges --------------------------------------------------------------------------------------------------------------------
def test_linear_rows_and_loss_prefixes_refuse_gradients_and_cpu_tensors():
    from mlhot.binding import MlhotError
    from mlhot.ops import linear_rows, loss_prefixes
    x, w, b = torch.randn(6, 8, requires_grad=True), torch.randn(4, 8), torch.randn(4)
    with pytest.raises(MlhotError, match="forward-only"):
        linear_rows([(x, 1, 0)], w, b, "relu")
    with pytest.raises(MlhotError, match="forward-only"):
        linear_rows([(x.detach(), 1, 0)], w.requires_grad_(), b, "relu")
    with pytest.raises(MlhotError, match="ROCm device"):
        linear_rows([(x.detach(), 1, 0), (x.detach(), 1, 0)], torch.randn(4, 16), b, "none")
    with torch.no_grad(), pytest.raises(MlhotError, match="ROCm device"):
        linear_rows([(x, 1, 0)], w, b, "relu")
    mu, gt = torch.randn(3, 5, 4, requires_grad=True), torch.randn(5, 4)
    with pytest.raises(MlhotError, match="forward-only"):
        loss_prefixes("quaternion", mu, gt)
    with pytest.raises(MlhotError, match="ROCm device"):
        loss_prefixes("quaternion", mu.detach(), gt)


def test_calc_loss_prefixes_uses_calc_loss_kind_table():
    from mlhot.binding import MlhotError
    from trainer.losses import LossFunc
    mu, gt = torch.randn(3, 5, 2), torch.randn(5, 2)
    assert LossFunc("nll", "shapenet_3d").calc_loss_prefixes(mu, gt) is None and LossFunc("nll", "shapenet_3d").calc_loss(mu[0], None, gt) is None
    assert LossFunc("mse", "no_such_task").calc_loss_prefixes(mu, gt, test=True) is None and LossFunc("mse", "no_such_task").calc_loss(mu[0], None, gt) is None
    for task in ("shapenet_3d", "shapenet_1d", "pascal_1d", "distractor"):      # a kind is chosen: the bridge is reached and refuses the CPU tensors
        with pytest.raises(MlhotError, match="ROCm device"):
            LossFunc("mse", task).calc_loss_prefixes(mu, gt, test=True)


# ---- the evaluator's switch, with stub models -------------------------------------------------------------------------------------------
class StubModel(torch.nn.Module):
    """Output depends on every context shot and target; forward_prefixes = one plain forward per k; every call recorded with its keywords."""

    def __init__(self, out_dim):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.0, out_dim))
        self.calls = []

    def forward(self, cx, cy, qx, test=False):
        self.calls.append(("forward", cx.shape[1]))
        s = cx.mean(dim=(1, 2, 3, 4)) + cy.mean(dim=(1, 2))
        return torch.tanh(qx.mean(dim=(2, 3, 4))[..., None] + s[:, None, None]) * self.w, None, 0

    def forward_prefixes(self, cx, cy, qx, **kw):
        self.calls.append(("forward_prefixes", cx.shape[1], tuple(sorted(kw.items()))))
        with torch.no_grad():
            s = [cx[:, :k].mean(dim=(1, 2, 3, 4)) + cy[:, :k].mean(dim=(1, 2)) for k in range(1, cx.shape[1] + 1)]
            return torch.stack([torch.tanh(qx.mean(dim=(2, 3, 4))[..., None] + sk[:, None, None]) * self.w for sk in s])


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


class StubLoss:
    def __init__(self, task):
        self.task, self.calls = task, []

    def calc_loss(self, mu, var, gt, test=False):
        self.calls.append("calc_loss")
        return O.calc_loss(self.task, mu, gt, test=test)

    def calc_loss_prefixes(self, mu, gt, test=False):
        self.calls.append("calc_loss_prefixes")
        return torch.stack([O.calc_loss(self.task, mu[k], gt, test=test).view(()) for k in range(mu.shape[0])])


def _evaluate(tmp_path, tag, **extra):
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot.synth import SyntheticViews
    log, task = [], "shapenet_3d"
    cfg = types.SimpleNamespace(device=torch.device("cpu"), tasks_per_batch=2, val_iters=3, max_ctx_num=4, task=task, contrastive=False,
                                logger=types.SimpleNamespace(info=log.append), save_path=str(tmp_path / tag), **extra)
    data, model, loss = Recorder(SyntheticViews(task, objects=4, views=8)), StubModel(4), StubLoss(task)
    res = ModelEvaluator(model=model, loss=loss, config=cfg, data=data).evaluate()
    return res, data.calls, model.calls, loss.calls, [m for m in log if "have been saved to" not in m]      # that line names the run's folder


def test_prefix_sweep_fold_config_errors(tmp_path):
    with pytest.raises(ValueError, match="prefix_sweep_fold needs prefix_sweep"):
        _evaluate(tmp_path, "alone", prefix_sweep_fold=True)
    with pytest.raises(ValueError, match="prefix_sweep_fold needs prefix_sweep"):
        _evaluate(tmp_path, "alone_false", prefix_sweep=False, prefix_sweep_fold=True)
    with pytest.raises(ValueError, match="prefix_sweep_fold must be"):
        _evaluate(tmp_path, "yes", prefix_sweep=True, prefix_sweep_fold="yes")
    with pytest.raises(ValueError, match="prefix_sweep_fold must be"):
        _evaluate(tmp_path, "one", prefix_sweep=True, prefix_sweep_fold=1)


def test_prefix_sweep_fold_absent_or_false_leaves_every_call_as_it_is(tmp_path):
    base = _evaluate(tmp_path, "sweep", prefix_sweep=True)
    assert base[2] == [("forward_prefixes", 4, ())] * 6 and set(base[3]) == {"calc_loss"}
    off = _evaluate(tmp_path, "off", prefix_sweep=True, prefix_sweep_fold=False)
    assert off[:4] == base[:4] and off[4] == base[4]
    plain = _evaluate(tmp_path, "plain")
    plain_off = _evaluate(tmp_path, "plain_off", prefix_sweep_fold=False)
    assert plain_off[:4] == plain[:4] and all(c[0] == "forward" for c in plain[2])
    for f in ("val_losses.txt", "test_losses.txt"):
        assert (tmp_path / "off" / f).read_text() == (tmp_path / "sweep" / f).read_text()


def test_prefix_sweep_fold_on_calls_the_folded_forward_and_one_loss_per_batch(tmp_path):
    base = _evaluate(tmp_path, "sweep", prefix_sweep=True)
    on = _evaluate(tmp_path, "fold", prefix_sweep=True, prefix_sweep_fold=True)
    assert on[1] == base[1]                                                       # the loader sees the prefix sweep's calls
    assert on[2] == [("forward_prefixes", 4, (("fold", True),))] * 6
    assert on[3] == ["calc_loss_prefixes"] * 6
    assert on[0] == base[0] and on[4] == base[4]                                  # the stub computes the same floats: same results, same log lines
    for f in ("val_losses.txt", "test_losses.txt"):
        assert (tmp_path / "fold" / f).read_text() == (tmp_path / "sweep" / f).read_text()


# ---- the host build --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["azimuth", "mse", "quaternion", "degree", "distractor"])
def test_host_build_loss_prefix_fwd_equals_loss_fwd_per_slice(hostsim, kind):
    g = torch.Generator().manual_seed(4)
    y_dim, gt_dim = {"azimuth": (2, 3), "degree": (2, 3), "mse": (2, 2), "quaternion": (4, 4), "distractor": (2, 2)}[kind]
    for P, rows in ((1, 1), (3, 7), (2, 600)):
        mu = torch.randn(P, rows, y_dim, generator=g)
        if kind == "degree":
            ang = torch.rand(P, rows, generator=g) * 6.28
            mu = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1) * 0.999
        gt = torch.randn(rows, gt_dim, generator=g)
        got = hostsim.loss_prefix_fwd(kind, mu, gt)
        want = torch.stack([hostsim.loss_fwd(kind, mu[p].contiguous(), gt) for p in range(P)])
        assert got.shape == (P,) and torch.equal(got, want), (kind, P, rows)


def test_host_build_reports_linear_rows_as_gpu_only(hostsim):
    from mlhot.binding import MlhotError
    assert not hostsim.linear_rows_supported(256, 256, 4)
    with pytest.raises(MlhotError, match="GPU build only"):
        hostsim.linear_rows_fwd([(torch.randn(4, 8), 1, 0)], torch.randn(2, 8), None, "none")


# ---- the row map -------------------------------------------------------------------------------------------------------------------------
def test_row_map_statement_against_repeat_and_tile():
    x = np.arange(12 * 3, dtype=np.float32).reshape(12, 3)
    assert np.array_equal(R.gather(x, 60, 5, 0), np.repeat(x, 5, axis=0))                    # one source row serves `rep` output rows
    assert np.array_equal(R.gather(x, 48, 1, 12), np.tile(x, (4, 1)))                        # the source wraps every `period` rows
    assert np.array_equal(R.gather(x, 72, 2, 12), np.tile(np.repeat(x, 2, axis=0), (3, 1)))
    assert np.array_equal(R.gather(x, 7, 1, 0), x[:7]) and np.array_equal(R.gather(x, 31, 5, 0), np.repeat(x, 5, axis=0)[:31])
    assert np.array_equal(R.source_rows(7, 3, 2), [0, 0, 0, 1, 1, 1, 0])
    t = torch.from_numpy(x)
    assert torch.equal(R.gather(t, 60, 5, 0), t.repeat_interleave(5, dim=0))
    w, b = np.ones((2, 6), dtype=np.float32), np.zeros(2, dtype=np.float32)
    y = R.linear_rows_np([(x, 1, 12), (x[:4], 6, 0)], w, b, "relu", 24)
    assert y.shape == (24, 2) and y[13, 0] == x[1].sum() + x[2].sum()
