"""Per-task context sizes and growing states without a GPU: every refusal of condition / extend (all raised before
any kernel), the operator's refusals, and the float64 restatement tests/ragged_ref.py against tests/favor_cached_ref.py."""
import importlib
import types

import pytest
import torch

from tests import favor_cached_ref as R
from tests import ragged_ref as RR

CFGV = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
            n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
             tasks_per_batch=2)
# family, class, agg_mode, extra configuration, image shape, label width
CASES = {
    "resnet_anp": ("ANP", dict(CFG3D, agg_mode="attention"), (3, 64, 64), 4),
    "resnet_cnp_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max"), (3, 64, 64), 4),
    "vanilla_anp": ("ANPShapeNet1D", dict(CFGV, agg_mode="attention", dim_r=64), (1, 128, 128), 3),
    "vanilla_cnp_mean": ("CNPShapeNet1D", dict(CFGV, agg_mode="mean", dim_r=100), (1, 128, 128), 3),
}


def _model(method, cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c)


def _state(model, T=2, Nc=4, lens=None):
    """A state as condition would leave it (contents never read: every refusal comes first)."""
    from mlhot.cached import VanillaContextState, _fingerprint
    from networks._resnet_np import ContextState, ResNetNP
    rows = torch.zeros(T, Nc, 8)
    if isinstance(model, ResNetNP):
        return ContextState(model, T, Nc, model._fingerprint(), "latent", z=torch.zeros(T, 256), lens=lens, kh=rows, vh=rows, rs=rows)
    return VanillaContextState(model, T, Nc, _fingerprint(model), "latent", z=torch.zeros(T, 64), lens=lens, kh=rows, vh=rows, rs=rows)


@pytest.mark.parametrize("case", list(CASES))
def test_condition_refusals(case):
    from mlhot import cached
    method, cfg, img, L = CASES[case]
    model = _model(method, cfg)
    cx, cy = torch.rand(2, 4, *img), torch.rand(2, 4, L)
    model.train()
    with pytest.raises(ValueError, match="eval"):
        cached.condition(model, cx, cy, ctx_len=[1, 2])
    model.eval()
    with pytest.raises(ValueError, match="tasks_per_batch"):
        cached.condition(model, cx[:1], cy[:1], ctx_len=[1])
    with pytest.raises(ValueError, match="ctx_len has 3 entries for 2 tasks"):
        cached.condition(model, cx, cy, ctx_len=[1, 2, 3])
    with pytest.raises(ValueError, match="ctx_len has 1 entries for 2 tasks"):
        cached.condition(model, cx, cy, ctx_len=torch.tensor([2]))
    for bad in ([1.0, 2], [1, 2.5], torch.tensor([1.0, 2.0]), [True, 2], ["1", 2]):
        with pytest.raises(ValueError, match="ctx_len must hold integers"):
            cached.condition(model, cx, cy, ctx_len=bad)
    for bad in ([0, 2], [1, 5], [-1, 4], torch.tensor([4, 5])):
        with pytest.raises(ValueError, match=r"ctx_len must lie in 1\.\.4"):
            cached.condition(model, cx, cy, ctx_len=bad)
    with pytest.raises(ValueError, match="capacity = 3 is smaller than the 4 context slots"):
        cached.condition(model, cx, cy, ctx_len=[1, 2], capacity=3)
    with pytest.raises(ValueError, match="capacity = 3 is smaller"):
        cached.condition(model, cx, cy, capacity=3)
    with pytest.raises(ValueError, match="capacity must be an integer"):
        cached.condition(model, cx, cy, ctx_len=[1, 2], capacity=6.0)
    if model.ATTENTION:
        with pytest.raises(ValueError, match="capacity = 33 is outside the cached attention kernels' envelope"):
            cached.condition(model, cx, cy, ctx_len=[1, 2], capacity=33)
        wide = torch.rand(2, 33, 1, 1, 1).expand(2, 33, *img)
        with pytest.raises(ValueError, match="capacity = 33 is outside"):
            cached.condition(model, wide, torch.rand(2, 33, L), ctx_len=[1, 2])
    with pytest.raises(ValueError, match="at least one context shot"):
        cached.condition(model, cx[:, :0], cy[:, :0], capacity=4)
    if hasattr(model, "extend"):                                  # the ResNet family's methods take the same arguments
        with pytest.raises(ValueError, match=r"ctx_len must lie in 1\.\.4"):
            model.condition(cx, cy, ctx_len=[0, 1])


@pytest.mark.parametrize("case", list(CASES))
def test_extend_refusals(case):
    from mlhot import cached
    method, cfg, img, L = CASES[case]
    model = _model(method, cfg)
    nx, ny = torch.rand(2, 2, *img), torch.rand(2, 2, L)
    good = _state(model, lens=(1, 3))
    model.train()
    with pytest.raises(ValueError, match="eval"):
        cached.extend(model, good, nx, ny)
    model.eval()
    other = _model(method, cfg).eval()
    with pytest.raises(ValueError, match="not made by this model"):
        cached.extend(other, good, nx, ny)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.extend(model, {"lens": (1, 3)}, nx, ny)
    with pytest.raises(ValueError, match="same tasks"):
        cached.extend(model, good, nx[:1], ny[:1])
    with pytest.raises(ValueError, match="same tasks"):
        cached.extend(model, _state(model, T=1, lens=(1,)), nx[:1], ny[:1])
    with pytest.raises(ValueError, match="new_len has 1 entries for 2 tasks"):
        cached.extend(model, good, nx, ny, new_len=[1])
    with pytest.raises(ValueError, match="new_len must hold integers"):
        cached.extend(model, good, nx, ny, new_len=[1.0, 0])
    for bad in ([3, 0], [-1, 1]):
        with pytest.raises(ValueError, match=r"new_len must lie in 0\.\.2"):
            cached.extend(model, good, nx, ny, new_len=bad)
    with pytest.raises(ValueError, match=r"task 1 would hold 5 context shots, the state's capacity is 4.*capacity="):
        cached.extend(model, good, nx, ny)                       # past capacity: 3 + 2 > 4
    with pytest.raises(ValueError, match=r"task 1 would hold 5 .*capacity="):
        cached.extend(model, good, nx, ny, new_len=[0, 2])
    full = _state(model)                                         # as made without ctx_len: lens all Nc, no spare slot
    assert full.lens == (4, 4) and full.capacity == 4
    with pytest.raises(ValueError, match=r"task 0 would hold 5 context shots, the state's capacity is 4 - condition with capacity="):
        cached.extend(model, full, nx, ny, new_len=[1, 0])
    assert good.lens == (1, 3) and good.capacity == 4            # nothing of the old state changed
    bias = model.mu.bias if hasattr(model, "mu") else model.r_to_z.bias
    with torch.no_grad():
        bias.add_(1.0)                                           # a weight update in place, as an optimizer step does
    with pytest.raises(ValueError, match="stale"):
        cached.extend(model, good, nx, ny, new_len=[1, 0])
    if hasattr(model, "extend"):
        with pytest.raises(ValueError, match="stale"):
            model.extend(good, nx, ny, new_len=[1, 0])


def test_bayes_by_backprop_and_other_classes_refuse():
    from mlhot import cached
    mr = _model("ANPMRShapeNet1D", dict(CFGV, agg_mode="attention", dim_r=64)).eval()
    with pytest.raises(ValueError, match="ANPMRShapeNet1D.*fresh weights"):
        cached.condition(mr, torch.rand(2, 2, 1, 128, 128), torch.rand(2, 2, 3), ctx_len=[1, 2])
    with pytest.raises(ValueError, match="ANPMRShapeNet1D.*fresh weights"):
        cached.extend(mr, None, torch.rand(2, 2, 1, 128, 128), torch.rand(2, 2, 3))
    mr3 = _model("ANPMRShapeNet3D", dict(CFG3D, tasks_per_batch=1, agg_mode="attention")).eval()
    with pytest.raises(ValueError, match="fresh weights"):
        mr3.condition(torch.rand(1, 2, 3, 64, 64), torch.rand(1, 2, 4), ctx_len=[1])
    with pytest.raises(ValueError, match="fresh weights"):
        mr3.extend(None, torch.rand(1, 2, 3, 64, 64), torch.rand(1, 2, 4))
    lin = torch.nn.Linear(4, 4).eval()
    with pytest.raises(ValueError, match="Linear.*not built"):
        cached.condition(lin, torch.rand(1, 1, 4), torch.rand(1, 1, 4), ctx_len=[1])
    with pytest.raises(ValueError, match="Linear.*not built"):
        cached.extend(lin, None, torch.rand(1, 1, 4), torch.rand(1, 1, 4))


@pytest.mark.parametrize("method", ["ANPShapeNet1D", "CNPShapeNet1D", "ANPVanillaPascal1D", "CNPVanillaPascal1D"])
def test_vanilla_classes_still_gain_no_attribute(method):
    cls = getattr(importlib.import_module("networks." + method), method)
    assert not any(hasattr(cls, name) for name in ("condition", "extend", "predict"))


@pytest.mark.parametrize("method", ["ANP", "CondNeuralProcess", "ANPDistractor", "CNPDistractor"])
def test_resnet_family_has_extend(method):
    cls = getattr(importlib.import_module("networks." + method), method)
    assert callable(cls.extend)


def test_favor_keys_with_lens_refuses_cpu_tensors_and_gradients():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_keys
    kh, proj = torch.randn(2, 3, 2, 16), torch.randn(32, 16)
    with pytest.raises(MlhotError, match="ROCm device"):
        favor_keys(kh, proj, lens=[1, 3])
    with pytest.raises(MlhotError, match="ROCm device"):
        favor_keys(kh, proj, lens=torch.tensor([1, 3]))
    with pytest.raises(MlhotError, match="forward-only"):
        favor_keys(kh.clone().requires_grad_(True), proj, lens=[1, 3])
    state = FavorKeyState("cached", (2, 3, 2, 16, 32), buf=None, lens=(1, 3))
    assert state.lens == (1, 3) and FavorKeyState("plain", (2, 3, 2, 16, 32), kh=kh).lens is None


def test_host_lens_checks():
    from mlhot.binding import MlhotError
    from mlhot.ops import host_lens
    assert host_lens([1, 3], 2, 1, 3, "lens") == (1, 3)
    assert host_lens(torch.tensor([2, 1], dtype=torch.int32), 2, 1, 3, "lens") == (2, 1)
    import numpy as np
    assert host_lens(np.array([2, 3]), 2, 1, 3, "lens") == (2, 3)
    for bad, msg in (([1], "1 entries for 2 tasks"), ([1, 4], r"lie in 1\.\.3"), ([0, 1], r"lie in 1\.\.3"), ([1.5, 2], "integers"),
                     (torch.tensor([1.0, 2.0]), "integers"), (torch.tensor([[1, 2]]), "one-dimensional"), (3, "sequence")):
        with pytest.raises(MlhotError, match=msg):
            host_lens(bad, 2, 1, 3, "lens")
    with pytest.raises(ValueError, match="integers"):
        host_lens([1.5, 2], 2, 1, 3, "lens", ValueError)


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
def _kqv(T, H, Nc, Nq, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.25 * torch.randn(T, H, Nq, d, generator=g, dtype=torch.float64), 0.25 * torch.randn(T, H, Nc, d, generator=g, dtype=torch.float64),
            torch.randn(T, H, Nc, d, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("L", [1, 5, 9])
def test_uniform_lens_equal_the_sliced_keys(L):
    T, H, Nc, d, m = 3, 2, 9, 16, 24
    q, k, v = _kqv(T, H, Nc, 4, d, 5)
    proj = torch.randn(m, d, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    k[:, :, L:] = float("nan")                                   # what lies behind lens is never read
    v[:, :, L:] = float("inf")
    fk, M = RR.key_features(k, proj, [L] * T)
    want, wantM = R.key_features(k[:, :, :L], proj)
    assert torch.equal(fk[:, :, :L], want) and torch.equal(M, wantM)
    assert bool((fk[:, :, L:] == 0).all()) and bool(torch.isfinite(fk).all())
    out = RR.attention(q, k, v, proj, [L] * T)
    assert (out - R.attention(q, k[:, :, :L], v[:, :, :L], proj)).abs().max().item() <= 1e-13
    assert (out - RR.attention_sliced(q, k, v, proj, [L] * T)).abs().max().item() <= 1e-13


def test_mixed_lens_take_the_stabiliser_of_the_valid_rows_only():
    T, H, Nc, d, m = 3, 2, 6, 16, 24
    q, k, v = _kqv(T, H, Nc, 4, d, 7)
    proj = torch.randn(m, d, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    lens = [2, 6, 1]
    clean, M = RR.key_features(k, proj, lens)
    loud = k.clone()
    loud[0, :, 2:] *= 100.0                                      # invalid rows whose dd would lead the batch by far
    loud[2, :, 1:] = float("nan")
    fk, M2 = RR.key_features(loud, proj, lens)
    assert torch.equal(fk, clean) and torch.equal(M, M2)
    dd = torch.einsum("thnd,md->thnm", d ** -0.25 * k, proj)
    assert M.item() == max(dd[t, :, :L].max().item() for t, L in enumerate(lens))
    assert M.item() < R.key_features(loud[:2], proj)[1].item()   # unmasked, the loud rows would have set it
    sliced, zero_rows = RR.attention_sliced(q, k, v, proj, lens), RR.attention(q, loud, v, proj, lens)
    assert (sliced - zero_rows).abs().max().item() <= 1e-13      # a zero row of F_k adds nothing to D or to out
