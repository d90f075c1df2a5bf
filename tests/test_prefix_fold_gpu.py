"""The folded prefix sweep on the MI355X: `forward_prefixes(fold=True)` against the plain forwards, against fold=False and against
the reference fixtures, its chunking contract, its launch count, and the evaluator with config.prefix_sweep_fold.  Run with -m gpu."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

from tests import util as U
from tests.test_prefix_sweep_gpu import CFG3D, CFGDIS, MODEL_CASES, _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["anp_3d", "cnp_3d_mean", "cnp_3d_baco", "cnp_distractor", "fclanp_3d"]


@pytest.mark.parametrize("case", CASES)
def test_folded_forward_prefixes_against_the_plain_forward_and_its_chunks(gpulib, case):
    method, cfg, T, Nc, Nq = MODEL_CASES[case]
    model = _model(method, cfg, T)
    cx, cy, qx = _batch(cfg, T, Nc, Nq)
    mu = model.forward_prefixes(cx, cy, qx, fold=True)
    assert mu.shape == (Nc, T, Nq, cfg["output_dim"])
    unfolded = model.forward_prefixes(cx, cy, qx)
    worst = 0.0
    with torch.no_grad():
        for k in range(1, Nc + 1):
            args = (cx[:, :k].contiguous(), cy[:, :k].contiguous(), qx)
            ref = model(*args, cy[:, :1].expand(-1, Nq, -1), test=True)[0] if model.CONTRASTIVE else model(*args, test=True)[0]
            worst = max(worst, U.rel_err(mu[k - 1], ref))
    against_unfolded = max(U.rel_err(mu[k], unfolded[k]) for k in range(Nc))
    print(f"forward_prefixes(fold=True) {case}: worst error over {Nc} context sizes {worst:.2e} of mu's scale against the plain forward, "
          f"{against_unfolded:.2e} against fold=False")
    assert worst <= U.RTOL and against_unfolded <= U.RTOL
    # chunked = unchunked, bit for bit
    half = Nc // 2
    chunks = torch.cat([model.forward_prefixes(cx, cy, qx, ks=range(1, half + 1), fold=True),
                        model.forward_prefixes(cx, cy, qx, ks=range(half + 1, Nc + 1), fold=True)])
    assert torch.equal(chunks, mu)
    assert torch.equal(model.forward_prefixes(cx, cy, qx, ks=[Nc, 1], fold=True), mu[[Nc - 1, 0]])


@pytest.mark.parametrize("name", ["p_anp_shapenet3d", "p_cnp_shapenet3d_max"])
def test_folded_forward_prefixes_against_the_reference_fixtures(gpulib, name):
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx).to(DEV).eval()
    views = torch.from_numpy(fx["views_u8"]).float().div(255.0).permute(0, 1, 4, 2, 3).contiguous().to(DEV)
    labels = torch.from_numpy(fx["labels"]).to(DEV)
    K = meta["K"]
    mu = model.forward_prefixes(views[:, :K].contiguous(), labels[:, :K].contiguous(), views, fold=True)
    worst = max(U.rel_err(mu[k], fx["mu"][k]) for k in range(K))
    print(f"forward_prefixes(fold=True) vs the reference ({name}): worst error {worst:.2e} of mu's scale")
    assert worst <= U.RTOL


@pytest.mark.parametrize("case", ["anp_3d", "cnp_3d_mean"])
def test_folded_launch_count_does_not_depend_on_the_number_of_prefixes(gpulib, case):
    method, cfg, T, Nc, Nq = MODEL_CASES[case]
    model = _model(method, cfg, T)
    cx, cy, qx = _batch(cfg, T, Nc, Nq)

    def launches(ks, fold):
        model.forward_prefixes(cx, cy, qx, ks=ks, fold=fold)          # warm: head stacks built, allocator sized
        gpulib.prof_begin(4096)
        model.forward_prefixes(cx, cy, qx, ks=ks, fold=fold)
        return [label for label, _ in gpulib.prof_end()]
    few, all_ = launches([1, 2], True), launches(list(range(1, Nc + 1)), True)
    assert len(few) == len(all_) and "linear_rows" in few, (len(few), len(all_))
    assert len(launches([1, 2], False)) != len(launches(list(range(1, Nc + 1)), False))


@pytest.mark.parametrize("method,task", [("ANP", "shapenet_3d"), ("CNPDistractor", "distractor")])
def test_evaluator_folded_prefix_sweep_against_its_plain_sweep(gpulib, tmp_path, method, task):
    """ModelEvaluator.evaluate() with prefix_sweep + prefix_sweep_fold: every row of both loss files within
    tests/util.py::test_loss_allowance of the plain sweep's, the same files, ONE loss launch per batch."""
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot.synth import SyntheticViews, host_convert
    from trainer.losses import LossFunc
    T, K, n_iter, views = 3, 5, 2, 8
    base = dict(CFG3D, agg_mode="attention") if task == "shapenet_3d" else dict(CFGDIS, agg_mode="max")
    results, loss_launches, logs = {}, {}, {}
    for fold in (False, True):                  # the plain sweep and the folded prefix sweep: two models from the same seed
        logs[fold] = []
        cfg = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, iterations=0, val_iters=n_iter, max_ctx_num=K, contrastive=False,
                                    logger=types.SimpleNamespace(info=logs[fold].append), save_path=str(tmp_path / f"fold{int(fold)}"), **base)
        if fold:
            cfg.prefix_sweep, cfg.prefix_sweep_fold = True, True
        model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
        ev = ModelEvaluator(model=model, loss=LossFunc("mse", task), config=cfg, data=SyntheticViews(task, objects=6, views=views))
        assert ev.ingest is not None
        gpulib.prof_begin(16384)
        results[fold] = ev.evaluate()
        labels = [label for label, _ in gpulib.prof_end()]
        loss_launches[fold] = (labels.count("loss_prefix_fwd"), labels.count("loss_fwd"))
    assert loss_launches[True] == (2 * n_iter, 0) and loss_launches[False][0] == 0, loss_launches      # 2 sources x n_iter batches
    assert [m for m in logs[True] if "loss:" in m or "std:" in m][0].startswith("validation loss: ")
    assert sum("loss:" in m for m in logs[True]) == sum("loss:" in m for m in logs[False]) == 2 * K
    assert sorted(os.listdir(tmp_path / "fold1")) == sorted(os.listdir(tmp_path / "fold0"))
    assert os.path.exists(tmp_path / "fold1" / "models" / "model.pt")
    plain = {f: np.loadtxt(tmp_path / "fold0" / f) for f in ("val_losses.txt", "test_losses.txt")}
    swept = {f: np.loadtxt(tmp_path / "fold1" / f) for f in ("val_losses.txt", "test_losses.txt")}
    for si, (source, f) in enumerate((("validation", "val_losses.txt"), ("test", "test_losses.txt"))):
        assert plain[f].shape == swept[f].shape == (K, 3) and list(swept[f][:, 0]) == list(range(1, K + 1))
        for k in range(1, K + 1):
            data = SyntheticViews(task, objects=6, views=views)
            getattr(data, "test_rng" if source == "test" else "val_rng").seed(42)
            bounds = []
            with torch.no_grad():
                for _ in range(n_iter):
                    xs, xq, ys, yq = data.get_batch_u8(source, T, k)
                    mu = model.eval()(host_convert(xs).to(DEV), ys.to(DEV), host_convert(xq).to(DEV), test=True)[0]
                    bounds.append(U.test_loss_allowance(task, mu, yq))
            (pm, ps), (sm, ss) = (results[False][si][0][k - 1], results[False][si][1][k - 1]), (results[True][si][0][k - 1], results[True][si][1][k - 1])
            tol_mean = sum(bounds) / n_iter + 1e-5 * max(1.0, abs(pm))
            tol_std = 2 ** 0.5 * max(bounds) + 1e-5 * max(1.0, abs(ps))           # std of two values = |a - b| / sqrt(2)
            print(f"[folded prefix sweep {method}] {source} k={k}: mean {pm:.6f} vs {sm:.6f} (allowed {tol_mean:.2e}), std {ps:.6f} vs {ss:.6f} (allowed {tol_std:.2e})")
            assert abs(pm - sm) <= tol_mean and abs(ps - ss) <= tol_std, (source, k)
            assert abs(plain[f][k - 1, 1] - swept[f][k - 1, 1]) <= tol_mean + 1e-4 and abs(plain[f][k - 1, 2] - swept[f][k - 1, 2]) <= tol_std + 1e-4
