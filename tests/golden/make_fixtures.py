#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (needs /root/reference, which never travels to the
GPU box).  It imports the reference's own ``networks/*`` and ``trainer/losses.py``
on torch-CPU with import stubs for the third-party packages the image lacks
(SURVEY.md Appendix C - none of the stubs touches hot-path arithmetic), feeds them
seeded inputs and stores inputs' hashes, forward taps, outputs, loss and gradients.

    python tests/golden/make_fixtures.py            # rewrites tests/golden/*.npz

The fixtures are data only: no reference source text is stored.  Weights are NOT
stored; each fixture keeps the sha256 of every state_dict tensor so the tests can
prove that the identically-seeded modules of this repo regenerate the same weights.
"""
import hashlib
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
FULL_GRAD_BYTES = 64 * 1024

warnings.filterwarnings("ignore")


def install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            raise RuntimeError("stub called")

    tv = mod("torchvision")
    tv.models = mod("torchvision.models")
    tv.models.utils = mod("torchvision.models.utils", load_state_dict_from_url=_Any())
    tv.transforms = mod("torchvision.transforms")

    class MetaModule(torch.nn.Module):
        pass

    tm = mod("torchmeta")
    tm.modules = mod(
        "torchmeta.modules", MetaModule=MetaModule,
        MetaSequential=type("MetaSequential", (torch.nn.Sequential, MetaModule), {}),
        MetaConv2d=type("MetaConv2d", (torch.nn.Conv2d, MetaModule), {}),
        MetaLinear=type("MetaLinear", (torch.nn.Linear, MetaModule), {}),
        MetaBatchNorm2d=type("MetaBatchNorm2d", (torch.nn.BatchNorm2d, MetaModule), {}))
    tm.utils = mod("torchmeta.utils", gradient_update_parameters=None)
    ia = mod("imgaug", seed=lambda *a, **k: None, ALL="ALL")
    ia.augmenters = mod("imgaug.augmenters")
    for n in ["Sometimes", "Sequential", "CropAndPad", "GammaContrast", "AddToBrightness",
              "AverageBlur", "Affine", "OneOf", "Dropout", "CoarseDropout"]:
        setattr(ia.augmenters, n, _Any)
    class NTXentLoss:                                    # stand-in for the absent package: the restated algorithm (see FCL_CASES)
        def __init__(self, temperature=0.07):
            self.temperature = temperature

        def __call__(self, embeddings, labels):
            sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
            from oracle.ref_cpu import nt_xent
            return nt_xent(embeddings, labels.tolist(), self.temperature)

    pml = mod("pytorch_metric_learning")
    pml.losses = mod("pytorch_metric_learning.losses", NTXentLoss=NTXentLoss)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))


BASE = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64,
            n_hidden_units_r=[100, 100], dim_z=64)

# name -> (method, cfg overrides, Nc, Nq)
MODEL_CASES = {
    # BASELINE.json configs[0..2]
    "c1_cnp_pascal1d": ("CNPVanillaPascal1D", dict(task="pascal_1d", tasks_per_batch=4, input_dim=1, output_dim=1,
                                                    agg_mode="mean", dim_r=100), 5, 5),
    "c2_cnp_shapenet1d_mean": ("CNPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=16, input_dim=3, output_dim=2,
                                                      agg_mode="mean", dim_r=100), 15, 15),
    "c3_anp_shapenet1d": ("ANPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=16, input_dim=3, output_dim=2,
                                                 agg_mode="attention", dim_r=64), 15, 15),
    # ragged / edge cases (Nc != Nq, Nc = 0, T = 1, other aggregators, Pascal ANP)
    "s_anp_shapenet1d_ragged": ("ANPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                       agg_mode="attention", dim_r=64), 3, 5),
    # mid-size: enough images for the band / unit loops of every kernel, few enough decisions (9.6 M) that no ReLU / pool tie
    # routes differently on the GPU - the test asserts flips == 0, so the reference's own gradients are compared directly
    "s_anp_shapenet1d_t2_full": ("ANPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                        agg_mode="attention", dim_r=64), 15, 15),
    "s_anp_shapenet1d_t1": ("ANPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=1, input_dim=3, output_dim=2,
                                                   agg_mode="attention", dim_r=64), 25, 30),
    "s_anp_shapenet1d_nc0": ("ANPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                    agg_mode="attention", dim_r=64), 0, 4),
    "s_anp_pascal1d": ("ANPVanillaPascal1D", dict(task="pascal_1d", tasks_per_batch=3, input_dim=1, output_dim=1,
                                                   agg_mode="attention", dim_r=64), 4, 6),
    "s_cnp_shapenet1d_max": ("CNPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=3, input_dim=3, output_dim=2,
                                                    agg_mode="max", dim_r=100), 7, 2),
    "s_cnp_shapenet1d_baco": ("CNPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                     agg_mode="baco", dim_r=256), 5, 3),
    "s_cnp_shapenet1d_nc0": ("CNPShapeNet1D", dict(task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                    agg_mode="mean", dim_r=100), 0, 3),
    "s_cnp_pascal1d_max": ("CNPVanillaPascal1D", dict(task="pascal_1d", tasks_per_batch=2, input_dim=1, output_dim=1,
                                                       agg_mode="max", dim_r=100), 1, 2),
}


# ResNet-encoder family: name -> (method, cfg, Nc, Nq, image channels fed to forward)
RESNET_CASES = {
    "r_anp_shapenet3d": ("ANP", dict(task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                     agg_mode="attention", img_agg="reshape", seed=2578, temperature=0.07), 3, 4, 3),
    "r_cnp_shapenet3d_max": ("CondNeuralProcess", dict(task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4,
                                                       output_dim=4, agg_mode="max", img_agg="reshape", seed=2578), 4, 3, 3),
    "r_cnp_distractor_baco": ("CondNeuralProcess", dict(task="distractor", img_size=[128, 128, 1], tasks_per_batch=1, input_dim=2,
                                                        output_dim=2, agg_mode="baco", img_agg="max", seed=2578), 3, 2, 1),
    # BASELINE config c5: Bayes-by-backprop encoder; torch.manual_seed(99) right before the forward fixes the eps draws,
    # backward on loss + 1e-7 * kl (beta of cfg/train/ANPMR_ShapeNet3D.yaml)
    "r_anpmr_shapenet3d": ("ANPMRShapeNet3D", dict(task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                                   agg_mode="attention", img_agg="reshape", seed=2578, temperature=0.07), 3, 4, 3),
    # Distractor plugins: labels pass through transform_y = Linear(2 -> dim_w=16) (cfg/train/ANP_Distractor.yaml)
    "r_anp_distractor": ("ANPDistractor", dict(task="distractor", img_size=[128, 128, 1], tasks_per_batch=1, input_dim=2, output_dim=2,
                                               agg_mode="attention", img_agg="max", dim_w=16, seed=2578), 3, 2, 1),
    "r_cnp_distractor_mean": ("CNPDistractor", dict(task="distractor", img_size=[128, 128, 1], tasks_per_batch=2, input_dim=2, output_dim=2,
                                                    agg_mode="mean", img_agg="max", dim_w=16, seed=2578), 2, 2, 1),
    "r_cnp_shapenet3d_nc0": ("CondNeuralProcess", dict(task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=1, input_dim=4,
                                                       output_dim=4, agg_mode="mean", img_agg="reshape", seed=2578), 0, 2, 3),
}


# Functional-contrastive variants: forward(ctx_x, ctx_y, qry_x, qry_y) -> (mu, var, kl, contrastive term).
# pytorch_metric_learning is not in this image: its NTXentLoss is stubbed with oracle.ref_cpu.nt_xent (the published algorithm
# restated), so the contrastive VALUE in these fixtures is restatement-vs-restatement ("parity unpinned" for that term);
# mu, the regression loss and the rest of the graph are the reference's own arithmetic.
FCL_CASES = {
    "f_fclcnp_shapenet1d_max": ("FCLCNPShapeNet1D", dict(BASE, task="shapenet_1d", tasks_per_batch=3, input_dim=3, output_dim=2,
                                                         agg_mode="max", dim_r=100), 4, 5, 1),
    "f_fclcnp_shapenet1d_mean": ("FCLCNPShapeNet1D", dict(BASE, task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                          agg_mode="mean", dim_r=100), 3, 3, 1),
    "f_fclanp_shapenet3d": ("FCLANP", dict(task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                           agg_mode="attention", img_agg="reshape", seed=2578, temperature=0.07), 3, 4, 3),
    "f_fclcnp_distractor_max": ("FCLCNPDistractor", dict(task="distractor", img_size=[128, 128, 1], tasks_per_batch=2, input_dim=2,
                                                         output_dim=2, agg_mode="max", img_agg="max", dim_w=16, seed=2578), 2, 3, 1),
    "f_fclcnp_distractor_baco": ("FCLCNPDistractor", dict(task="distractor", img_size=[128, 128, 1], tasks_per_batch=2, input_dim=2,
                                                          output_dim=2, agg_mode="baco", img_agg="max", dim_w=16, seed=2578), 3, 2, 1),
}


# Meta-regularised twins of the vanilla models (SURVEY.md §8a E1 "MR twin" / B1): Bayes-by-backprop vanilla encoder.
# Same runner as the ResNet family: torch.manual_seed(99) right before the forward, backward on loss + 1e-7 * kl.
MR1D = dict(img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, seed=2578, temperature=0.07)
MR_CASES = {
    "m_anpmr_shapenet1d": ("ANPMRShapeNet1D", dict(MR1D, task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                    agg_mode="attention"), 3, 4, 1),
    "m_anpmr_pascal1d": ("ANPMR", dict(MR1D, task="pascal_1d", tasks_per_batch=1, input_dim=1, output_dim=1,
                                       agg_mode="attention"), 4, 2, 1),
    "m_cnpmr_pascal1d_max": ("CNPMR", dict(MR1D, task="pascal_1d", tasks_per_batch=2, input_dim=1, output_dim=1,
                                           agg_mode="max"), 3, 2, 1),
    "m_cnpmr_shapenet1d_mean": ("CNPMRShapeNet1D", dict(MR1D, task="shapenet_1d", tasks_per_batch=2, input_dim=3, output_dim=2,
                                                         agg_mode="mean"), 2, 3, 1),
}


def run_resnet_case(name, method, cfgd, Nc, Nq, C, LossFunc):
    cfg = types.SimpleNamespace(device=torch.device("cpu"), **cfgd)
    model = getattr(importlib.import_module(f"networks.{method}"), method)(cfg)
    T = cfg.tasks_per_batch
    H, W, _ = cfg.img_size
    # With 2-5 images a single ReLU whose pre-activation is a rounding-level tie (|v| ~ 1e-7 of scale)
    # moves the upstream gradients by ~1e-2 between ANY two fp32 evaluation orders; the
    # seed-1234 draw of the distractor case contains such a tie in layer3.conv1, so that case uses 4321.
    input_seed = 4321 if name == "r_cnp_distractor_baco" else 1234
    cx, qx, cy, qy = make_inputs(T, Nc, Nq, C, H, W, cfg.input_dim, seed=input_seed)
    if cfg.task == "shapenet_3d":                       # unit quaternions with q[1] >= 0 (shapenet_3d.py:226-227)
        qy = torch.nn.functional.normalize(qy - 0.5, dim=-1)
        qy = torch.where(qy[..., 1:2] < 0, -qy, qy)
    model.train()
    torch.manual_seed(99)
    mu, var, kl = model(cx, cy, qx)
    assert var is None
    loss = LossFunc("mse", cfg.task).calc_loss(mu, var, qy)
    (loss + 1e-7 * kl if torch.is_tensor(kl) else loss).backward()
    out = {"mu": np32(mu), "loss": np.float64(loss.item()), "qy": np32(qy), "kl": np.float64(float(kl))}
    state_sha, grad_norm = {k: sha(v) for k, v in model.state_dict().items()}, {}
    if hasattr(model, "attn"):
        out["projection_matrix"] = np32(model.attn.projection_matrix)
    for k, prm in model.named_parameters():
        if prm.grad is None:
            grad_norm[k] = None
            continue
        gnp = np32(prm.grad)
        grad_norm[k] = float(np.linalg.norm(gnp.astype(np.float64)))
        if gnp.nbytes <= 16 * 1024:
            out["grad/" + k] = gnp
        else:
            flat = gnp.reshape(-1)
            out["gradhead/" + k] = flat[:1024].copy()
            out["gradstride/" + k] = flat[1::61][:4096].copy()
    meta = dict(name=name, method=method, cfg=cfgd, Nc=Nc, Nq=Nq, C=C, input_seed=input_seed, state_sha=state_sha, grad_norm=grad_norm,
                input_sha=dict(cx=sha(cx), qx=sha(qx), cy=sha(cy)), n_params=sum(p.numel() for p in model.parameters()))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: loss={loss.item():.8f} sum(mu)={mu.sum().item():.8f} params={meta['n_params']}")


# BASELINE configs[4]'s per-GPU share at its REAL size: ANPMRShapeNet3D, 8 tasks x (15 + 15) resp. the training
# draw's (7 + 23) 3x64x64 views, torch.manual_seed(99) right before the forward, backward on loss + 1e-7 * kl.  Inputs follow
# tests/test_gpu_parity.py::test_c5_full_size_forward_backward_vs_oracle (one generator seeded 1234: images U[0, 1), labels =
# normalised N(0, 1)^4 quaternions).  Weights by sha, gradients as norms + heads + strided samples: ~2 MB per case.
# `labels`: "quat" as described; "rand" = SURVEY.md section 8c's recipe (cx, qx, cy, qy all torch.rand from the one generator), whose
# answers the survey recorded: loss 2.26335859, kl 1383162.5, |grad| 2.12012622.  The FAVOR+ projection buffer (1.45 MB, the same
# for every fixture of this model and seed) is NOT repeated: tests load it from r_anpmr_shapenet3d.npz (sha-checked).
C5_FULL_CASES = {"c5_anpmr_shapenet3d_t8": (15, 15, "quat"), "c5_anpmr_shapenet3d_t8_7_23": (7, 23, "quat"),
                 "c5_anpmr_shapenet3d_t8_survey": (15, 15, "rand")}


def run_c5_full_case(name, Nc, Nq, labels, LossFunc):
    cfgd = dict(task="shapenet_3d", img_size=[64, 64, 4], tasks_per_batch=8, input_dim=4, output_dim=4, agg_mode="attention",
                img_agg="reshape", seed=2578, temperature=0.07)
    cfg = types.SimpleNamespace(device=torch.device("cpu"), **cfgd)
    model = importlib.import_module("networks.ANPMRShapeNet3D").ANPMRShapeNet3D(cfg)
    T = 8
    g = torch.Generator().manual_seed(1234)
    cx, qx = torch.rand(T, Nc, 3, 64, 64, generator=g), torch.rand(T, Nq, 3, 64, 64, generator=g)
    if labels == "quat":
        cy = torch.nn.functional.normalize(torch.randn(T, Nc, 4, generator=g), dim=-1)
        qy = torch.nn.functional.normalize(torch.randn(T, Nq, 4, generator=g), dim=-1)
    else:
        cy, qy = torch.rand(T, Nc, 4, generator=g), torch.rand(T, Nq, 4, generator=g)
    model.train()
    torch.manual_seed(99)
    mu, var, kl = model(cx, cy, qx)
    assert var is None
    loss = LossFunc("mse", cfg.task).calc_loss(mu, var, qy)
    (loss + 1e-7 * kl).backward()
    out = {"mu": np32(mu), "loss": np.float64(loss.item()), "kl": np.float64(float(kl))}
    state_sha, grad_norm, total = {k: sha(v) for k, v in model.state_dict().items()}, {}, 0.0
    for k, prm in model.named_parameters():
        if prm.grad is None:
            grad_norm[k] = None
            continue
        gnp = np32(prm.grad)
        grad_norm[k] = float(np.linalg.norm(gnp.astype(np.float64)))
        total += grad_norm[k] ** 2
        if gnp.nbytes <= 16 * 1024:
            out["grad/" + k] = gnp
        else:
            flat = gnp.reshape(-1)
            out["gradhead/" + k] = flat[:1024].copy()
            out["gradstride/" + k] = flat[1::61][:4096].copy()
    meta = dict(name=name, method="ANPMRShapeNet3D", cfg=cfgd, Nc=Nc, Nq=Nq, C=3, input_seed=1234, eps_seed=99, labels=labels,
                projection_from="r_anpmr_shapenet3d", state_sha=state_sha,
                grad_norm=grad_norm, grad_norm_total=total ** 0.5,
                input_sha=dict(cx=sha(cx), qx=sha(qx), cy=sha(cy), qy=sha(qy)), n_params=sum(p.numel() for p in model.parameters()))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: loss={loss.item():.8f} kl={float(kl):.1f} |grad|={total ** 0.5:.8f} mu[0,0]={mu[0, 0].tolist()} params={meta['n_params']}")


def run_fcl_case(name, method, cfgd, Nc, Nq, C, LossFunc):
    cfg = types.SimpleNamespace(device=torch.device("cpu"), **cfgd)
    model = getattr(importlib.import_module(f"networks.{method}"), method)(cfg)
    T = cfg.tasks_per_batch
    H, W, _ = cfg.img_size
    cx, qx, cy, qy = make_inputs(T, Nc, Nq, C, H, W, cfg.input_dim, seed=1234)
    if cfg.task == "shapenet_3d":
        qy = torch.nn.functional.normalize(qy - 0.5, dim=-1)
        qy = torch.where(qy[..., 1:2] < 0, -qy, qy)
    model.train()
    mu, var, kl, contra = model(cx, cy, qx, qy)
    assert var is None and kl == 0
    loss = LossFunc("mse", cfg.task).calc_loss(mu, var, qy)
    (loss + contra).backward()                           # contrastive_rate 1 (model_trainer.py:80-81 scales it by the config's rate)
    model.eval()
    with torch.no_grad():
        mu_t, _, _, contra_t = model(cx, cy, qx, qy, test=True)
    assert contra_t == 0 and torch.equal(mu_t, mu.detach())
    out = {"mu": np32(mu), "loss": np.float64(loss.item()), "contra": np.float64(contra.item()), "qy": np32(qy)}
    state_sha, grad_norm = {k: sha(v) for k, v in model.state_dict().items()}, {}
    if hasattr(model, "attn"):
        out["projection_matrix"] = np32(model.attn.projection_matrix)
    for k, prm in model.named_parameters():
        if prm.grad is None:
            grad_norm[k] = None
            continue
        gnp = np32(prm.grad)
        grad_norm[k] = float(np.linalg.norm(gnp.astype(np.float64)))
        if gnp.nbytes <= 16 * 1024:
            out["grad/" + k] = gnp
        else:
            flat = gnp.reshape(-1)
            out["gradhead/" + k] = flat[:1024].copy()
            out["gradstride/" + k] = flat[1::61][:4096].copy()
    meta = dict(name=name, method=method, cfg=cfgd, Nc=Nc, Nq=Nq, C=C, input_seed=1234, state_sha=state_sha, grad_norm=grad_norm,
                input_sha=dict(cx=sha(cx), qx=sha(qx), cy=sha(cy)), n_params=sum(p.numel() for p in model.parameters()))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: loss={loss.item():.8f} contra={contra.item():.8f} sum(mu)={mu.sum().item():.8f} params={meta['n_params']}")


def make_inputs(T, Nc, Nq, C, H, W, L, seed=1234):
    g = torch.Generator().manual_seed(seed)
    cx = torch.rand(T, Nc, C, H, W, generator=g)
    qx = torch.rand(T, Nq, C, H, W, generator=g)
    cy = torch.rand(T, Nc, L, generator=g)
    qy = torch.rand(T, Nq, L, generator=g)
    return cx, qx, cy, qy


def run_model_case(name, method, over, Nc, Nq, LossFunc):
    cfgd = dict(BASE, **over)
    cfg = types.SimpleNamespace(device=torch.device("cpu"), **cfgd)
    model = getattr(importlib.import_module(f"networks.{method}"), method)(cfg)
    T = cfg.tasks_per_batch
    H, W, C = cfg.img_size
    cx, qx, cy, qy = make_inputs(T, Nc, Nq, C, H, W, cfg.input_dim)

    calls = {}

    def hook(tag):
        def fn(_m, _inp, out):
            calls.setdefault(tag, []).append(out.detach().clone())
        return fn

    for tag in ["encoder_w0", "encoder_r", "attn", "_W", "r_to_z", "transform_y"]:
        if hasattr(model, tag):
            getattr(model, tag).register_forward_hook(hook(tag))

    model.train()
    mu, var, kl = model(cx, cy, qx)
    assert var is None
    loss = LossFunc("mse", cfg.task).calc_loss(mu, var, qy)
    (loss + 1e-7 * kl if torch.is_tensor(kl) else loss).backward()
    with torch.no_grad():
        model.eval()
        mu_test, _, _ = model(cx, cy, qx, test=True)
        loss_test = LossFunc("mse", cfg.task).calc_loss(mu_test, None, qy, test=True)

    out = {"meta": None, "mu": np32(mu), "loss": np.float64(loss.item()),
           "loss_test": np.float64(loss_test.item()), "kl": np.float64(float(kl))}
    enc = calls.get("encoder_w0", [])
    is_anp = method.startswith("ANP")
    if Nc:
        # ANP encodes qry first (ANPShapeNet1D.py:129-134), CNP ctx first (CNPShapeNet1D.py:108-134)
        out["x_qry"], out["x_ctx"] = (np32(enc[0]), np32(enc[1])) if is_anp else (np32(enc[1]), np32(enc[0]))
        out["rs"] = np32(calls["encoder_r"][0])
        out["z_lin"] = np32(calls["r_to_z"][0])
        if is_anp:
            out["attn_out"] = np32(calls["attn"][0])
            out["r"] = np32(calls["_W"][0])
    else:
        out["x_qry"] = np32(enc[0])

    state_sha, grad_norm = {}, {}
    for k, v in model.state_dict().items():
        state_sha[k] = sha(v)
    if is_anp:
        # the QR inside gaussian_orthogonal_random_matrix is LAPACK/CPU dependent (MKL picks other
        # code paths on other hosts), so this one buffer travels with the fixture
        out["projection_matrix"] = np32(model.attn.projection_matrix)
    for k, prm in model.named_parameters():
        if prm.grad is None:
            grad_norm[k] = None
            continue
        gnp = np32(prm.grad)
        grad_norm[k] = float(np.linalg.norm(gnp.astype(np.float64)))
        if gnp.nbytes <= FULL_GRAD_BYTES:
            out["grad/" + k] = gnp
        else:
            flat = gnp.reshape(-1)
            out["gradhead/" + k] = flat[:4096].copy()
            out["gradstride/" + k] = flat[1::61].copy()
    meta = dict(name=name, method=method, cfg=cfgd, Nc=Nc, Nq=Nq, input_seed=1234,
                input_sha=dict(cx=sha(cx), qx=sha(qx), cy=sha(cy), qy=sha(qy)),
                state_sha=state_sha, grad_norm=grad_norm,
                n_params=sum(p.numel() for p in model.parameters()),
                torch=torch.__version__, threads=torch.get_num_threads())
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: loss={loss.item():.8f} sum(mu)={mu.sum().item():.8f} "
          f"gradnorm={np.sqrt(sum(v * v for v in grad_norm.values() if v is not None)):.8f}")


def run_favor_cases():
    """FastAttention / softmax_kernel / linear_attention in isolation (fast_attention.py)."""
    fa = importlib.import_module("networks.fast_attention")
    out = {}
    meta = {}
    for tag, (T, H, Nc, Nq, d, scale, nb) in {"d64": (3, 8, 5, 7, 64, 1.0, None), "d64_big": (2, 8, 15, 15, 64, 4.0, None),
                                              "d256": (1, 2, 3, 4, 256, 0.5, 320)}.items():
        torch.manual_seed(77)
        attn = fa.FastAttention(dim_heads=d, nb_features=nb, causal=False)
        g = torch.Generator().manual_seed(4321)
        q = (torch.randn(T, H, Nq, d, generator=g) * scale).requires_grad_()
        k = (torch.randn(T, H, Nc, d, generator=g) * scale).requires_grad_()
        v = torch.randn(T, H, Nc, d, generator=g).requires_grad_()
        wout = torch.randn(T, H, Nq, d, generator=g)
        proj = attn.projection_matrix
        qp = fa.softmax_kernel(q, projection_matrix=proj, is_query=True)
        kp = fa.softmax_kernel(k, projection_matrix=proj, is_query=False)
        o = attn(q, k, v)
        (o * wout).sum().backward()
        out[f"{tag}/proj"] = np32(proj)   # QR is host-LAPACK dependent: the matrix travels
        out.update({f"{tag}/q": np32(q), f"{tag}/k": np32(k), f"{tag}/v": np32(v),
                    f"{tag}/wout": np32(wout), f"{tag}/qp": np32(qp), f"{tag}/kp": np32(kp), f"{tag}/out": np32(o),
                    f"{tag}/dq": np32(q.grad), f"{tag}/dk": np32(k.grad), f"{tag}/dv": np32(v.grad)})
        meta[tag] = dict(T=T, H=H, Nc=Nc, Nq=Nq, d=d, m=int(proj.shape[0]), proj_seed=77, proj_sha=sha(proj))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "favor.npz"), **out)
    print("favor:", {k: v["m"] for k, v in meta.items()})


def run_favor_c5_cases():
    """FastAttention at the SHIPPED ANPMRShapeNet3D shape (ANPMRShapeNet3D.py:160-183: 8 heads, d = 256, nb_features = None ->
    m = int(256 ln 256) = 1419), 15 + 15 shots and the ragged 7 + 23 training draw, with inputs scaled (0.25 randn: dd has unit
    spread, diag = 0.5) so that exp(dd - diag - max) sits far above the 1e-4 floor: query and key gradients are first-class, not
    the fp32 residue the whole-model fixtures see at the seeded weights.  One projection matrix (seed 77) serves both tags."""
    fa = importlib.import_module("networks.fast_attention")
    out, meta = {}, {}
    for tag, (T, H, Nc, Nq, d, scale) in {"c5_15_15": (2, 8, 15, 15, 256, 0.25), "c5_7_23": (2, 8, 7, 23, 256, 0.25)}.items():
        torch.manual_seed(77)
        attn = fa.FastAttention(dim_heads=d, nb_features=None, causal=False)
        g = torch.Generator().manual_seed(8642 + Nc)
        q = (torch.randn(T, H, Nq, d, generator=g) * scale).requires_grad_()
        k = (torch.randn(T, H, Nc, d, generator=g) * scale).requires_grad_()
        v = torch.randn(T, H, Nc, d, generator=g).requires_grad_()
        wout = torch.randn(T, H, Nq, d, generator=g)
        proj = attn.projection_matrix
        qp = fa.softmax_kernel(q, projection_matrix=proj, is_query=True)
        kp = fa.softmax_kernel(k, projection_matrix=proj, is_query=False)
        o = attn(q, k, v)
        (o * wout).sum().backward()
        if "proj" in out:
            assert sha(proj) == sha(torch.from_numpy(out["proj"]))
        out["proj"] = np32(proj)
        out.update({f"{tag}/q": np32(q), f"{tag}/k": np32(k), f"{tag}/v": np32(v), f"{tag}/wout": np32(wout),
                    f"{tag}/qp00": np32(qp[0, 0]), f"{tag}/kp00": np32(kp[0, 0]), f"{tag}/out": np32(o),
                    f"{tag}/dq": np32(q.grad), f"{tag}/dk": np32(k.grad), f"{tag}/dv": np32(v.grad)})
        # how far the features sit above the +1e-4 floor, and how live the query / key gradients are
        meta[tag] = dict(T=T, H=H, Nc=Nc, Nq=Nq, d=d, m=int(proj.shape[0]), proj_seed=77, proj_sha=sha(proj),
                         kp_median_over_floor=float((kp.detach() * proj.shape[0] ** 0.5).median() / 1e-4),
                         dq_over_dv=float(q.grad.abs().max() / v.grad.abs().max()),
                         dk_over_dv=float(k.grad.abs().max() / v.grad.abs().max()))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "favor_c5.npz"), **out)
    print("favor_c5:", meta)


def run_loss_cases(LossFunc):
    g = torch.Generator().manual_seed(99)
    out = {}
    pr2 = torch.tanh(torch.randn(4, 6, 2, generator=g))
    ang = torch.rand(4, 6, 1, generator=g) * 2 * np.pi
    gt3 = torch.cat([torch.cos(ang), torch.sin(ang), ang], dim=-1)
    out["az/pr"], out["az/gt"] = np32(pr2), np32(gt3)
    out["az/train"] = np.float64(LossFunc("mse", "shapenet_1d").calc_loss(pr2, None, gt3).item())
    out["az/test"] = np.float64(LossFunc("mse", "shapenet_1d").calc_loss(pr2.clone(), None, gt3, test=True).item())
    pr1, gt1 = torch.randn(3, 5, 1, generator=g), torch.rand(3, 5, 1, generator=g)
    out["pas/pr"], out["pas/gt"] = np32(pr1), np32(gt1)
    out["pas/train"] = np.float64(LossFunc("mse", "pascal_1d").calc_loss(pr1, None, gt1).item())
    pr4 = torch.randn(2, 7, 4, generator=g)
    gt4 = torch.nn.functional.normalize(torch.randn(2, 7, 4, generator=g), dim=-1)
    out["quat/pr"], out["quat/gt"] = np32(pr4), np32(gt4)
    out["quat/train"] = np.float64(LossFunc("mse", "shapenet_3d").calc_loss(pr4, None, gt4).item())
    prd, gtd = torch.randn(2, 3, 2, generator=g), torch.rand(2, 3, 2, generator=g)
    out["dis/pr"], out["dis/gt"] = np32(prd), np32(gtd)
    out["dis/train"] = np.float64(LossFunc("mse", "distractor").calc_loss(prd, None, gtd).item())
    np.savez_compressed(os.path.join(OUT, "losses.npz"), **out)
    print("losses: ok")


def run_conv_embedding_case():
    """ConvEmbeddingModel with the MMAMLShapeNet1D settings (MMAMLShapeNet1D.py:63-81)."""
    cem = importlib.import_module("networks.conv_embedding_model")
    torch.manual_seed(2578)
    model = cem.ConvEmbeddingModel(
        input_size=np.prod((1, 128, 128)), output_size=2, embedding_dims=[64, 128, 256, 512], hidden_size=128,
        num_layers=2, convolutional=True, num_conv=4, num_channels=32, rnn_aggregation=False,
        linear_before_rnn=False, embedding_pooling="avg", batch_norm=True, avgpool_after_conv=True,
        img_size=(1, 128, 128))
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(6, 1, 128, 128, generator=g)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    embs = model(x)
    sum(((e * (i + 1)).sum() for i, e in enumerate(embs))).backward()
    out = {}
    for i, e in enumerate(embs):
        out[f"emb{i}"] = np32(e)
    meta = dict(state_sha={k: sha(v) for k, v in sd0.items()}, seed=2578, input_seed=1234, x_sha=sha(x),
                grad_norm={k: float(p.grad.norm()) for k, p in model.named_parameters() if p.grad is not None})
    for k, p in model.named_parameters():
        if p.grad is not None and p.grad.numel() * 4 <= FULL_GRAD_BYTES:
            out["grad/" + k] = np32(p.grad)
    for k, v in model.state_dict().items():
        if "running" in k:
            out["after/" + k] = np32(v)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(OUT, "conv_embedding.npz"), **out)
    print("conv_embedding: ok", [tuple(e.shape) for e in embs])


def run_ingest_case():
    """Host-side image conversion of the loaders: the divide restates dataset/shapenet_1d.py:189-190 (that method needs the
    LFS data files to run), the layout change is the reference's own utils.utils.convert_channel_last_np_to_tensor."""
    conv = importlib.import_module("utils.utils").convert_channel_last_np_to_tensor
    rng = np.random.RandomState(5)
    out = {}
    for C, (H, W) in ((1, (8, 12)), (3, (8, 8)), (4, (6, 10)), (2, (5, 3))):
        u8 = rng.randint(0, 256, size=(2, 3, H, W, C)).astype(np.uint8)
        n = min(256, u8.size)
        u8.reshape(-1)[:n] = np.arange(n, dtype=np.uint8)      # every byte value appears (where the case is large enough)
        out[f"c{C}/u8"] = u8
        out[f"c{C}/f32"] = np32(conv(u8.astype(np.float32) / 255.0))
    np.savez_compressed(os.path.join(OUT, "ingest.npz"), **out)
    print("ingest", {k: v.shape for k, v in out.items()})


def run_cfg_case():
    """Every YAML under the reference's cfg/, parsed as its train.py parses it (yaml.safe_load): relative path -> key/value dict,
    the data test_boundary.py::test_every_reference_yaml_parses feeds to configs.config.Config."""
    import glob
    import yaml
    root = os.path.join(REF, "cfg")
    out = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*.yaml"), recursive=True)):
        with open(path, "rb") as fh:
            out[os.path.relpath(path, root)] = yaml.safe_load(fh)
    with open(os.path.join(OUT, "reference_cfgs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("cfg", len(out))


def main():
    assert os.path.isdir(REF), "the reference is only available in the build container"
    install_stubs()
    sys.path.insert(0, REF)
    os.chdir(REF)
    torch.set_num_threads(8)
    LossFunc = importlib.import_module("trainer.losses").LossFunc
    only = set(sys.argv[1:])
    for name, (method, over, Nc, Nq) in MODEL_CASES.items():
        if only and name not in only:
            continue
        run_model_case(name, method, over, Nc, Nq, LossFunc)
    for name, (method, cfgd, Nc, Nq, C) in RESNET_CASES.items():
        if only and name not in only:
            continue
        run_resnet_case(name, method, cfgd, Nc, Nq, C, LossFunc)
    for name, (method, cfgd, Nc, Nq, C) in MR_CASES.items():
        if only and name not in only:
            continue
        run_resnet_case(name, method, cfgd, Nc, Nq, C, LossFunc)
    for name, (method, cfgd, Nc, Nq, C) in FCL_CASES.items():
        if only and name not in only:
            continue
        run_fcl_case(name, method, cfgd, Nc, Nq, C, LossFunc)
    for name, (Nc, Nq, labels) in C5_FULL_CASES.items():
        if only and name not in only:
            continue
        run_c5_full_case(name, Nc, Nq, labels, LossFunc)
    if not only or "favor" in only:
        run_favor_cases()
    if not only or "favor_c5" in only:
        run_favor_c5_cases()
    if not only or "losses" in only:
        run_loss_cases(LossFunc)
    if not only or "conv_embedding" in only:
        run_conv_embedding_case()
    if not only or "ingest" in only:
        run_ingest_case()
    if not only or "cfg" in only:
        run_cfg_case()


if __name__ == "__main__":
    main()
