"""The prefix sweep of the attention models beyond 32 context shots on the MI355X: `mlhot.cached.sweep` on an
ANPShapeNet1D-shaped model and `ResNetNP.forward_prefixes` on an ANP (ResNet, 64x64x3)-shaped one at Nc = 40 against one plain
test-mode forward per context size, and the paths up to 32 shots left as they were.

What the parent commit does at Nc > 32 (recorded when this file was written): `mlhot.cached.sweep` on a vanilla attention model picks
the composed route and RAISES MlhotError in mlhot.ops.favor_keys ("lens needs the cached kernels' envelope (Nc <= 32, ...)"), and
route="fused" raises ValueError; `ResNetNP.forward_prefixes` FALLS BACK to a loop of mlhot_favor_fwd over all Nc prefixes whatever `ks`
asks for.  Neither reaches mlhot.ops.favor_prefixes_long, which these tests require.  Run with -m gpu."""
import importlib
import types

import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, NC, NQ, KS = 2, 40, 5, [1, 32, 33, 40]

CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
             task="shapenet_1d", input_dim=3, output_dim=2, agg_mode="attention", dim_r=64)
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07,
             agg_mode="attention")


def _model(method, cfg):
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _batch(cfg, Nc, Nq, seed=3):
    g = torch.Generator().manual_seed(seed)
    H, W, C = cfg["img_size"]
    C = C - 1 if cfg["task"] == "shapenet_3d" else C
    n = max(Nc, Nq)
    views, ys = torch.rand(T, n, C, H, W, generator=g), torch.rand(T, n, cfg["input_dim"], generator=g)
    return views[:, :Nc].contiguous().to(DEV), ys[:, :Nc].contiguous().to(DEV), views[:, :Nq].contiguous().to(DEV)


def _plain(model, cx, cy, qx, ks):
    with torch.no_grad():
        return torch.stack([model(cx[:, :k].contiguous(), cy[:, :k].contiguous(), qx, test=True)[0] for k in ks])


@pytest.fixture
def long_calls(monkeypatch):
    """Counts the calls of mlhot_favor_prefix_long_fwd's wrapper."""
    import mlhot
    lib, calls = mlhot.lib(), []
    real = lib.favor_prefix_long_fwd
    monkeypatch.setattr(lib, "favor_prefix_long_fwd", lambda *a, **kw: (calls.append(len(a[4])), real(*a, **kw))[1])
    return calls


def test_vanilla_attention_sweep_at_40_shots(gpulib, long_calls):
    from mlhot import cached
    model = _model("ANPShapeNet1D", CFG1D)
    cx, cy, qx = _batch(CFG1D, NC, NQ)
    want = _plain(model, cx, cy, qx, KS)
    got = cached.sweep(model, cx, cy, qx, ks=KS)
    errs = [U.rel_err(got[i], want[i]) for i in range(len(KS))]
    print(f"sweep ANPShapeNet1D Nc={NC}: sizes {KS}: {' '.join(f'{e:.2e}' for e in errs)} of mu's scale")
    assert got.shape == want.shape == (len(KS), T, NQ, 2) and max(errs) <= U.RTOL
    assert cached.sweep.last_route == "composed" and cached.sweep.last_attention == "prefix_long" and long_calls == [len(KS)]
    # ks=None is 1..Nc; the same bits whether the sizes go out together or split
    every = cached.sweep(model, cx, cy, qx)
    assert every.shape[0] == NC and torch.equal(every[[k - 1 for k in KS]], got)
    assert torch.equal(torch.cat([cached.sweep(model, cx, cy, qx, ks=range(1, 21)), cached.sweep(model, cx, cy, qx, ks=range(21, NC + 1))]), every)
    with pytest.raises(ValueError, match="route 'fused'"):
        cached.sweep(model, cx, cy, qx, ks=KS, route="fused")


def test_resnet_attention_forward_prefixes_at_40_shots(gpulib, long_calls):
    model = _model("ANP", CFG3D)
    cx, cy, qx = _batch(CFG3D, NC, NQ)
    want = _plain(model, cx, cy, qx, KS)
    for fold in (False, True):
        got = model.forward_prefixes(cx, cy, qx, ks=KS, fold=fold)
        errs = [U.rel_err(got[i], want[i]) for i in range(len(KS))]
        print(f"forward_prefixes ANP Nc={NC} fold={fold}: sizes {KS}: {' '.join(f'{e:.2e}' for e in errs)} of mu's scale")
        assert got.shape == want.shape and max(errs) <= U.RTOL
        assert model.last_prefix_attention == "prefix_long"
    assert long_calls == [len(KS), len(KS)]                      # the asked-for sizes only, one call each
    a = model.forward_prefixes(cx, cy, qx, ks=[40, 1, 33])       # any order, as below 32 shots
    b = model.forward_prefixes(cx, cy, qx, ks=KS)
    assert torch.equal(a, b[[3, 0, 2]])


def test_up_to_32_shots_every_call_takes_the_path_it_took(gpulib, long_calls):
    from mlhot import cached
    model = _model("ANPShapeNet1D", CFG1D)
    cx, cy, qx = _batch(CFG1D, 15, NQ)
    labels, mu = U.launch_labels(gpulib, lambda: cached.sweep(model, cx, cy, qx))
    assert cached.sweep.last_route == "fused" and cached.sweep.last_attention == "np_prefix" and mu.shape[0] == 15
    assert not any(x.startswith("favor.plong") for x in labels), labels
    cx, cy, qx = _batch(CFG1D, 32, NQ)
    cached.sweep(model, cx, cy, qx, ks=[1, 32])
    assert cached.sweep.last_route == "fused"
    cached.sweep(model, cx, cy, qx, ks=[1, 32], route="composed")
    assert cached.sweep.last_attention == "favor_keys"
    res = _model("ANP", CFG3D)
    cx, cy, qx = _batch(CFG3D, 15, NQ)
    labels, _ = U.launch_labels(gpulib, lambda: res.forward_prefixes(cx, cy, qx))
    assert res.last_prefix_attention == "prefix" and not any(x.startswith("favor.plong") for x in labels), labels
    assert long_calls == []
