"""Prefix sweep for the vanilla family without a GPU: every refusal of mlhot.cached.sweep is host work and comes
before any kernel; supports_sweep answers for every class in scope; the classes keep their refusing forward_prefixes; the host
flavour of the library does not serve the sweep launch; and the float64 restatement's prefixes are what its name says."""
import importlib
import types

import pytest
import torch

from tests import np_prefix_ref as PR
from tests import np_query_ref as NR

CFG = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
           n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape")
CASES = {"anp": ("ANPShapeNet1D", "attention", 64), "cnp_mean": ("CNPShapeNet1D", "mean", 100), "cnp_max": ("CNPShapeNet1D", "max", 100),
         "cnp_baco": ("CNPShapeNet1D", "baco", 256), "anp_pascal": ("ANPVanillaPascal1D", "attention", 64),
         "cnp_pascal": ("CNPVanillaPascal1D", "mean", 100)}


def _model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c)


def _vanilla(case):
    method, agg, dim_r = CASES[case]
    cfg = dict(CFG, task="pascal_1d", input_dim=1, output_dim=1) if "pascal" in case else CFG
    return _model(method, agg_mode=agg, dim_r=dim_r, **cfg)


def _batch(Nc=3, Nq=4, T=2):
    return torch.rand(T, Nc, 1, 128, 128), torch.rand(T, Nc, 3), torch.rand(T, Nq, 1, 128, 128)


@pytest.mark.parametrize("case", ["anp", "cnp_mean"])
def test_sweep_refuses_on_the_host(case):
    from mlhot import cached
    from mlhot.binding import MlhotError
    model = _vanilla(case)
    cx, cy, qx = _batch()
    model.train()
    with pytest.raises(ValueError, match="eval"):
        cached.sweep(model, cx, cy, qx)
    model.eval()
    with pytest.raises(ValueError, match="tasks_per_batch"):
        cached.sweep(model, *_batch(T=3))
    with pytest.raises(ValueError, match="tasks_per_batch"):
        cached.sweep(model, cx, cy, qx[:1])
    with pytest.raises(ValueError, match="at least one context shot"):
        cached.sweep(model, cx[:, :0], cy[:, :0], qx)
    for bad in ([], [2, 1], [1, 1], [0, 1], [1, 4], [1.5], [True], torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError, match="ks"):
            cached.sweep(model, cx, cy, qx, ks=bad)
    with pytest.raises(ValueError, match="route"):
        cached.sweep(model, cx, cy, qx, route="eager")
    with pytest.raises(MlhotError, match="ROCm device"):              # everything above came first; this is _need_gpu's own error
        cached.sweep(model, cx, cy, qx, ks=[1, 3])
    with pytest.raises(MlhotError, match="ROCm device"):
        cached.sweep(model, cx, cy, qx, route="composed")
    assert not hasattr(type(model), "sweep")                          # the classes gain no attribute


@pytest.mark.parametrize("method,agg", [("ANPMRShapeNet1D", "attention"), ("CNPMRShapeNet1D", "mean")])
def test_bayes_by_backprop_twins_refuse(method, agg):
    from mlhot import cached
    mr = _model(method, agg_mode=agg, dim_r=64, **CFG).eval()
    ok, reason = cached.supports_sweep(mr)
    assert not ok and "fresh weights in every forward" in reason
    with pytest.raises(ValueError, match=method + ".*fresh weights"):
        cached.sweep(mr, *_batch())


def test_supports_sweep_answers_for_every_class_in_scope():
    from mlhot import cached
    for case in CASES:
        ok, reason = cached.supports_sweep(_vanilla(case))
        assert ok and "mlhot_np_prefix_fwd" in reason, case
    resnet = _model("CondNeuralProcess", tasks_per_batch=2, agg_mode="max", **CFG3D)
    assert cached.supports_sweep(resnet) == (True, "ResNetNP.forward_prefixes")
    mr3d = _model("ANPMRShapeNet3D", tasks_per_batch=1, agg_mode="attention", **CFG3D)
    assert not cached.supports_sweep(mr3d)[0] and "fresh weights" in cached.supports_sweep(mr3d)[1]
    lin = torch.nn.Linear(4, 4)
    assert cached.supports_sweep(lin) == (False, "the prefix sweep is not built for this class")
    with pytest.raises(ValueError, match="Linear.*not built"):
        cached.sweep(lin, *_batch())


def test_resnet_instances_go_to_their_forward_prefixes():
    from mlhot import cached
    model = _model("CondNeuralProcess", tasks_per_batch=2, agg_mode="max", **CFG3D).eval()
    model.forward_prefixes = lambda cx, cy, qx, ks=None: ("mu", cx, cy, qx, ks)
    assert cached.sweep(model, "cx", "cy", "qx", ks=[1, 2]) == ("mu", "cx", "cy", "qx", [1, 2])
    with pytest.raises(ValueError, match="route"):
        cached.sweep(model, "cx", "cy", "qx", route="fused")


@pytest.mark.parametrize("case", list(CASES))
def test_the_classes_keep_their_refusing_forward_prefixes(case):
    model = _vanilla(case).eval()
    with pytest.raises(ValueError, match="outside the prefix sweep - its forward is one fused call"):
        model.forward_prefixes(*_batch())


def test_hostsim_does_not_serve_the_sweep_launch(hostsim):
    import ctypes as C
    from mlhot.binding import NpParams
    dims = hostsim.np_dims(2, 15, 1, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 266)
    assert hostsim.c.mlhot_np_prefix_supported(C.byref(dims), 15) == 0 and not hostsim.np_prefix_supported(dims, 15)
    assert hostsim.c.mlhot_np_prefix_ws_bytes(C.byref(dims), 15) == 0
    x, mu = torch.zeros(2, 1, 64), torch.zeros(1, 2, 1, 2)
    ks = (C.c_int32 * 1)(1)
    rc = hostsim.c.mlhot_np_prefix_fwd(C.byref(dims), C.byref(NpParams()), C.c_void_p(x.data_ptr()), 1, ks, 1, None, None, None,
                                      C.c_void_p(mu.data_ptr()), None, 0, None)
    assert rc == 4 and "np_prefix_fwd" in hostsim.c.mlhot_last_error().decode()       # MLHOT_ERR_UNSUPPORTED


def test_restatement_prefix_is_the_tail_on_the_sliced_context():
    """want()[k - 1] is np_query_ref's tail on the first k shots; the last prefix of a base kind is np_query_ref's own result; the
    key placements move M_k as their names say."""
    d, m, Nc, Nq = 16, 16, 15, 3
    for attend in (True, False):
        got = PR.want("live", d, m, Nc, Nq, attend, False)
        assert got.shape == (Nc, NR.T, Nq, NR.Y_DIM)
        if attend:
            assert torch.equal(got[-1], NR.want("live", d, m, Nc, Nq, True, False))
    groups = {kind: len(set(PR.running_max(kind, 64, 266, Nc).tolist())) for kind in ("peak_first", "peak_last", "climb", "equal")}
    assert groups["peak_first"] == 1 and groups["climb"] == Nc and groups["equal"] == 1 and groups["peak_last"] >= 2
    M = PR.running_max("peak_last", 64, 266, Nc)
    assert M[-1] > M[-2] + 30 and PR.group_boundary("peak_last", 64, 266, Nc) == Nc and PR.group_boundary("peak_first", 64, 266, Nc) == 1
