"""Prefix sweep on the MI355X: the prefix kernels against the plain kernels on sliced inputs, `forward_prefixes` against K plain
forwards, the evaluator's prefix sweep against its plain sweep.  Run with -m gpu."""
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "max", "baco"])
def test_agg_prefixes_equal_agg_fwd_on_every_prefix(gpulib, mode):
    """Row k-1 of agg_prefixes against mlhot_agg_fwd on rs[:, :k], k = 1..25: bit-equal in all three modes (csrc/prefix.h's header)."""
    from mlhot.ops import agg_prefixes
    g = torch.Generator().manual_seed(11)
    T, Nc, R = 20, 25, 256
    rs = torch.randn(T, Nc, R, generator=g).to(DEV)
    lv = (torch.randn(T, Nc, R, generator=g) * 2).to(DEV) if mode == "baco" else None
    out = agg_prefixes(mode, rs, lv)
    assert out.shape == (Nc, T, R)
    worst = 0.0
    for k in range(1, Nc + 1):
        ref = gpulib.agg_fwd(mode, rs[:, :k].contiguous(), lv[:, :k].contiguous() if lv is not None else None)[0]
        worst = max(worst, U.rel_err(out[k - 1], ref))
        assert torch.equal(out[k - 1].view(torch.int32), ref.view(torch.int32)), (k, worst)
    print(f"agg_prefixes {mode}: worst error over the 25 prefixes {worst:.2e} of the tensor's scale")
    assert worst == 0.0


def _favor_cases():
    """name -> (q, k, v, proj) in the oracle's layout [T, H, N, d]."""
    cases = {}
    fx = np.load(os.path.join(U.GOLDEN, "favor_c5.npz"))
    proj = torch.from_numpy(fx["proj"])
    for tag in json.loads(str(fx["meta"])):                      # 15 + 15 and 7 + 23 shots at d = 256, m = 1419, 8 heads
        cases[tag] = tuple(torch.from_numpy(fx[f"{tag}/{n}"]) for n in ("q", "k", "v")) + (proj,)
    g = torch.Generator().manual_seed(5)
    T, H, Nc, Nq, d = 2, 8, 25, 30, 256
    cases["25_30"] = (torch.randn(T, H, Nq, d, generator=g) * 0.3, torch.randn(T, H, Nc, d, generator=g) * 0.3,
                      torch.randn(T, H, Nc, d, generator=g), proj)
    fx2 = np.load(os.path.join(U.GOLDEN, "favor.npz"))          # the large-norm case: inputs x 4, features mostly at the 1e-4 floor
    cases["d64_big"] = tuple(torch.from_numpy(fx2[f"d64_big/{n}"]) for n in ("q", "k", "v", "proj"))
    # the stabiliser's arg-max in the LAST shot, far above the first shots' (dd ~ N(0, (4 s)^2) for keys ~ N(0, s^2): the maxima
    # of the early shots are ~ 2, the last shot's is ~ 60): exp(. - M_Nc) of the early keys underflows where exp(. - M_k) does not
    T, H, Nc, Nq = 2, 8, 12, 9
    k = torch.randn(T, H, Nc, d, generator=g) * 0.12
    k[:, :, -1] *= 30.0
    cases["argmax_last"] = (torch.randn(T, H, Nq, d, generator=g) * 0.3, k, torch.randn(T, H, Nc, d, generator=g), proj)
    # ... climbing from shot to shot (one feature pass per step of more than e^32)
    k = torch.randn(T, H, Nc, d, generator=g) * 0.12 * (1.5 ** torch.arange(Nc, dtype=torch.float32))[None, None, :, None]
    cases["argmax_climbs"] = (torch.randn(T, H, Nq, d, generator=g) * 0.3, k, torch.randn(T, H, Nc, d, generator=g), proj)
    # M_k constant: the batch's largest key is in the first shot
    k = torch.randn(T, H, Nc, d, generator=g) * 0.12
    k[:, :, 0] *= 4.0
    cases["argmax_first"] = (torch.randn(T, H, Nq, d, generator=g) * 0.3, k, torch.randn(T, H, Nc, d, generator=g), proj)
    return cases


@pytest.mark.parametrize("case", ["c5_15_15", "c5_7_23", "25_30", "d64_big", "argmax_last", "argmax_climbs", "argmax_first"])
def test_favor_prefixes_equal_favor_fwd_on_every_prefix(gpulib, case):
    """out[k-1] of favor_prefixes against mlhot_favor_fwd on the first k keys / values, each at 1e-4 of ITS OWN scale, no floor."""
    from mlhot.ops import favor_prefixes
    from tests.prefix_ref import favor_stabilisers_np
    q, k, v, proj = _favor_cases()[case]
    M = favor_stabilisers_np(k, proj)
    if case == "argmax_last":
        assert M[-1] - M[0] > 40 and M[-1] > M[-2] + 40, M
    if case == "argmax_climbs":
        assert M[-1] - M[0] > 100, M
    if case == "argmax_first":
        assert np.all(M == M[0]), M
    qn, kn, vn = (t.permute(0, 2, 1, 3).contiguous().to(DEV) for t in (q, k, v))
    pd = proj.to(DEV)
    assert gpulib.favor_prefix_supported(qn.shape[0], qn.shape[2], qn.shape[1], kn.shape[1], qn.shape[3], pd.shape[0]), "the prefix kernels must serve this shape"
    out = favor_prefixes(qn, kn, vn, pd)
    Nc = kn.shape[1]
    assert out.shape == (Nc,) + tuple(qn.shape[:2]) + (qn.shape[2] * qn.shape[3],)
    assert bool(torch.isfinite(out).all())
    worst = (0.0, 0)
    for kk in range(1, Nc + 1):
        ref, _ = gpulib.favor_fwd(qn, kn[:, :kk].contiguous(), vn[:, :kk].contiguous(), pd)
        e = U.rel_err(out[kk - 1], ref)
        worst = max(worst, (e, kk))
    print(f"favor_prefixes {case}: M_1 = {M[0]:.2f}, M_Nc = {M[-1]:.2f}; worst error {worst[0]:.2e} of out[k]'s own scale (k = {worst[1]})")
    assert worst[0] <= U.RTOL, worst


def test_prefix_operators_are_forward_only(gpulib):
    from mlhot.binding import MlhotError
    from mlhot.ops import agg_prefixes, favor_prefixes
    rs = torch.randn(2, 3, 8, device=DEV, requires_grad=True)
    with pytest.raises(MlhotError, match="forward-only"):
        agg_prefixes("mean", rs)
    with torch.no_grad():
        agg_prefixes("mean", rs)
    q = torch.randn(1, 2, 2, 16, device=DEV, requires_grad=True)
    kv = torch.randn(1, 3, 2, 16, device=DEV)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_prefixes(q, kv, kv, torch.randn(32, 16, device=DEV))
    with pytest.raises(MlhotError, match="ROCm device"):
        agg_prefixes("mean", torch.randn(2, 3, 8))


# ---- the model ------------------------------------------------------------------------------------------------------------------
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFGDIS = dict(task="distractor", img_size=[128, 128, 1], input_dim=2, output_dim=2, img_agg="max", dim_w=16, seed=2578, temperature=0.07)
MODEL_CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention"), 2, 5, 6),
    "cnp_3d_mean": ("CondNeuralProcess", dict(CFG3D, agg_mode="mean"), 2, 5, 6),
    "cnp_3d_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max"), 2, 5, 6),
    "cnp_3d_baco": ("CondNeuralProcess", dict(CFG3D, agg_mode="baco"), 2, 5, 6),
    "anp_distractor": ("ANPDistractor", dict(CFGDIS, agg_mode="attention"), 2, 4, 5),
    "cnp_distractor": ("CNPDistractor", dict(CFGDIS, agg_mode="max"), 2, 4, 5),
    "fclanp_3d": ("FCLANP", dict(CFG3D, agg_mode="attention"), 2, 4, 5),
    "fclcnp_distractor_baco": ("FCLCNPDistractor", dict(CFGDIS, agg_mode="baco"), 2, 4, 5),
    "anp_3d_shipped_eval_shape": ("ANP", dict(CFG3D, agg_mode="attention"), 20, 25, 30),
}


def _model(method, cfg, T):
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _batch(cfg, T, Nc, Nq, seed=3):
    g = torch.Generator().manual_seed(seed)
    H, W, C = cfg["img_size"]
    C = C - 1 if cfg["task"] == "shapenet_3d" else C
    views = torch.rand(T, max(Nc, Nq), C, H, W, generator=g)                  # eval mode: the context is a prefix of the targets' views
    ys = torch.rand(T, max(Nc, Nq), cfg["input_dim"], generator=g)
    return views[:, :Nc].contiguous().to(DEV), ys[:, :Nc].contiguous().to(DEV), views[:, :Nq].contiguous().to(DEV)


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_forward_prefixes_equals_one_plain_forward_per_context_size(gpulib, case):
    method, cfg, T, Nc, Nq = MODEL_CASES[case]
    model = _model(method, cfg, T)
    cx, cy, qx = _batch(cfg, T, Nc, Nq)
    mu = model.forward_prefixes(cx, cy, qx)
    assert mu.shape == (Nc, T, Nq, cfg["output_dim"])
    worst = 0.0
    with torch.no_grad():
        for k in range(1, Nc + 1):
            args = (cx[:, :k].contiguous(), cy[:, :k].contiguous(), qx)
            ref = model(*args, cy[:, :1].expand(-1, Nq, -1), test=True)[0] if model.CONTRASTIVE else model(*args, test=True)[0]
            worst = max(worst, U.rel_err(mu[k - 1], ref))
    print(f"forward_prefixes {case}: worst error over {Nc} context sizes {worst:.2e} of mu's scale")
    assert worst <= U.RTOL
    # chunked = unchunked, bit for bit
    half = Nc // 2
    chunks = torch.cat([model.forward_prefixes(cx, cy, qx, ks=range(1, half + 1)), model.forward_prefixes(cx, cy, qx, ks=range(half + 1, Nc + 1))])
    assert torch.equal(chunks, mu)
    assert torch.equal(model.forward_prefixes(cx, cy, qx, ks=[Nc, 1]), mu[[Nc - 1, 0]])


@pytest.mark.parametrize("name", ["p_anp_shapenet3d", "p_cnp_shapenet3d_max"])
def test_forward_prefixes_against_the_reference_fixtures(gpulib, name):
    """The reference's own ANP / CondNeuralProcess run at k = 1..K on prefix contexts (tests/golden/make_prefix_fixtures.py)."""
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx).to(DEV).eval()
    views = torch.from_numpy(fx["views_u8"]).float().div(255.0).permute(0, 1, 4, 2, 3).contiguous().to(DEV)
    labels = torch.from_numpy(fx["labels"]).to(DEV)
    K = meta["K"]
    mu = model.forward_prefixes(views[:, :K].contiguous(), labels[:, :K].contiguous(), views)
    worst = max(U.rel_err(mu[k], fx["mu"][k]) for k in range(K))
    print(f"forward_prefixes vs the reference ({name}): worst error {worst:.2e} of mu's scale")
    assert worst <= U.RTOL


def test_forward_prefixes_refusals_on_the_device(gpulib):
    method, cfg, T, Nc, Nq = MODEL_CASES["anp_3d"]
    model = _model(method, cfg, T)
    cx, cy, qx = _batch(cfg, T, Nc, Nq)
    model.train()
    with pytest.raises(ValueError, match="eval"):
        model.forward_prefixes(cx, cy, qx)
    model.eval()
    with pytest.raises(ValueError, match="ks"):
        model.forward_prefixes(cx, cy, qx, ks=[0])
    with pytest.raises(ValueError, match="ks"):
        model.forward_prefixes(cx, cy, qx, ks=[Nc + 1])


# ---- the evaluator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,task", [("ANP", "shapenet_3d"), ("CNPDistractor", "distractor")])
def test_evaluator_prefix_sweep_against_its_plain_sweep(gpulib, tmp_path, method, task):
    """ModelEvaluator.evaluate() with config.prefix_sweep on the synthetic eval-mode loader through the u8 ingest: every row of both
    loss files within tests/util.py::test_loss_allowance of the plain sweep's, and ONE trunk call per batch instead of one per
    batch and context size (counted through mlhot_prof_begin / _end)."""
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot.synth import SyntheticViews, host_convert
    from trainer.losses import LossFunc
    T, K, n_iter, views = 3, 5, 2, 8
    base = dict(CFG3D, agg_mode="attention") if task == "shapenet_3d" else dict(CFGDIS, agg_mode="max")
    results, trunk_calls, logs = {}, {}, {}
    for sweep in (False, True):                 # two evaluators, two models - from the same seed, so with the same weights
        logs[sweep] = []
        logger = types.SimpleNamespace(info=logs[sweep].append)
        cfg = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, iterations=0, val_iters=n_iter, max_ctx_num=K, contrastive=False,
                                    logger=logger, save_path=str(tmp_path / f"sweep{int(sweep)}"), **base)
        if sweep:
            cfg.prefix_sweep = True
        model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
        ev = ModelEvaluator(model=model, loss=LossFunc("mse", task), config=cfg, data=SyntheticViews(task, objects=6, views=views))
        assert ev.ingest is not None
        gpulib.prof_begin(16384)
        results[sweep] = ev.evaluate()
        trunk_calls[sweep] = sum(1 for label, _ in gpulib.prof_end() if label == "trunk.stem")      # one stem launch per trunk call, every pass in it
    assert trunk_calls[False] == 2 * K * n_iter and trunk_calls[True] == 2 * n_iter, trunk_calls
    assert any("reproduces the reference's draws" in m for m in logs[True])
    plain = {f: np.loadtxt(tmp_path / "sweep0" / f) for f in ("val_losses.txt", "test_losses.txt")}
    swept = {f: np.loadtxt(tmp_path / "sweep1" / f) for f in ("val_losses.txt", "test_losses.txt")}
    for si, (source, f) in enumerate((("validation", "val_losses.txt"), ("test", "test_losses.txt"))):
        assert plain[f].shape == swept[f].shape == (K, 3) and list(swept[f][:, 0]) == list(range(1, K + 1))
        for k in range(1, K + 1):
            # the allowance from the plain forward's own mu on the same draws (`model`: the second evaluator's, the first one's weights)
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
            print(f"[prefix sweep {method}] {source} k={k}: mean {pm:.6f} vs {sm:.6f} (allowed {tol_mean:.2e}), std {ps:.6f} vs {ss:.6f} (allowed {tol_std:.2e})")
            assert abs(pm - sm) <= tol_mean and abs(ps - ss) <= tol_std, (source, k)
            # the files hold the numbers at 4 decimals
            assert abs(plain[f][k - 1, 1] - swept[f][k - 1, 1]) <= tol_mean + 1e-4 and abs(plain[f][k - 1, 2] - swept[f][k - 1, 2]) <= tol_std + 1e-4
    assert os.path.exists(tmp_path / "sweep1" / "models" / "model.pt")
