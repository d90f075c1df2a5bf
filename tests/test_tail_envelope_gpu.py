"""tests/tail_cases.py on the MI355X: every case under the default options (the family np_route() picks: the run-time-shaped fused
attention tail, the fused CNP tail or the operator chain) and with tail_fused = 0 (the chain), each run held on its own to the float64
oracle under that run's routing; the family that ran is read from the profiler's launch labels and must be the same in forward and
backward.  Tolerances are the suite's: util.RTOL on mu and every saved activation, util.RTOL with the util.GRAD_FLOOR floor on every
gradient, 2e-4 of their own scale and no floor on W_q / W_k.  Worst values on record: profiles/INDEX_tail_envelope.md.
Run with -m gpu."""
import types

import pytest
import torch

from tests import tail_cases as TC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

NAMES = [c.name for c in TC.CASES]
_REF = {}          # case name -> (routes, oracle): the two runs of a case share the oracle when their routing is identical


def _same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _oracle(c, routes):
    if c.name not in _REF or not _same(_REF[c.name][0], routes):
        _REF[c.name] = (routes, TC.oracle(c, routes))
    return _REF[c.name][1]


def _run(gpulib, c, tail_fused, **kw):
    gpulib.set_option("tail_fused", tail_fused)
    try:
        return TC.run(gpulib, c, DEV, **kw)
    finally:
        gpulib.set_option("tail_fused", 1)


@pytest.mark.parametrize("impl", ["default", "chain"])
@pytest.mark.parametrize("name", NAMES)
def test_case_vs_float64_oracle(gpulib, name, impl):
    c = TC.BY_NAME[name]
    got = _run(gpulib, c, 1 if impl == "default" else 0)
    want = c.family if impl == "default" else "generic"
    fwd, bwd = TC.family_of(got["fwd_labels"]), TC.family_of(got["bwd_labels"])
    assert (fwd, bwd) == (want, want), f"{name} [{impl}]: forward ran {fwd}, backward {bwd}, expected {want}: {got['fwd_labels']} {got['bwd_labels']}"
    worst = TC.compare(c, got, _oracle(c, got["routes"]), f"{impl} ({fwd})")
    U.parity_log(f"tail envelope {name} [{impl}] family {fwd}: activations {worst['act']:.2e}, gradients {worst['grad']:.2e}, W_q / W_k {worst['qk']:.2e}, "
                 f"{worst['flips']} of {worst['decisions']} decisions flipped, LDS {TC.lds_bytes(c) if fwd != 'generic' else {}}")


@pytest.mark.parametrize("name", ["attn_distinct", "cnp_distinct_mean"])
def test_gradient_arena_and_loss_inside_the_backward_are_bit_equal(gpulib, name):
    """One forward's gradients three ways: every gradient a tensor of its own (the slabs reduce segment by segment), one flat buffer in
    mlhot_np_grads_flat_layout's order (one contiguous sum), and the loss's gradient taken inside mlhot_np_vanilla_bwd_loss - the same
    bits.  A slab entry or a flat offset computed from the wrong width would move or overlap a gradient.
    conv1's two gradients are the exception between the first two: the encoder folds its conv1 rows with c2::conv1_grads_kernel when
    weight and bias are tensors of their own and inside the one deferred sum when they are adjacent (csrc/encoder.h enc_backward_ws) -
    two fixed summation orders over the same rows, so those two are held to each other at the suite's gradient tolerance instead."""
    c = TC.BY_NAME[name]
    own = _run(gpulib, c, 1, flat=False)["grads"]
    flat = _run(gpulib, c, 1, flat=True)["grads"]
    for k in own:
        if k.startswith("encoder_w0.0."):
            assert U.rel_err(own[k], flat[k]) <= U.RTOL, f"{name}: {k}: {U.rel_err(own[k], flat[k]):.2e}"
        else:
            assert torch.equal(own[k], flat[k]), f"{name}: {k} differs between separate gradient tensors and the flat arena"
    plain = _run(gpulib, c, 1, loss="loss_then_bwd")
    inside = _run(gpulib, c, 1, loss="bwd_loss")
    assert TC.family_of(inside["bwd_labels"]) == c.family
    for k in own:
        assert torch.equal(plain["grads"][k], inside["grads"][k]), f"{name}: {k} differs when the backward takes the loss itself"


def test_anp_model_at_dim_w_128_trains_a_step(gpulib):
    """ANPShapeNet1D with cfg.dim_w = 128 (m = int(128 ln 128) = 621 random features): phase B' of the fused tail would need 264,576
    bytes of LDS, so the model takes the operator chain; loss.backward() succeeds and its gradients are the raw entry's bits."""
    from networks.ANPShapeNet1D import ANPShapeNet1D
    c = TC.BY_NAME["attn_dw128"]
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=c.T, input_dim=c.label_dim,
                                output_dim=c.y_dim, agg_mode="attention", img_agg="", dim_w=c.dim_w, n_hidden_units_r=list(c.hidden),
                                dim_r=c.dim_r, dim_z=c.dim_z, task="shapenet_1d")
    model = ANPShapeNet1D(cfg).to(DEV)
    assert tuple(model.attn.projection_matrix.shape) == (c.m_feat, c.dim_w)
    model.load_state_dict({k: v.to(DEV) for k, v in TC.params(c.name).items()}, strict=True)
    model.train()
    cx, cy, qx, dmu = (t.to(DEV) for t in TC.inputs(c.name))
    labels, mu = U.launch_labels(gpulib, lambda: model(cx, cy, qx)[0])
    assert TC.family_of(labels) == "generic", labels
    labels, _ = U.launch_labels(gpulib, lambda: (mu * dmu).sum().backward())
    torch.cuda.synchronize()
    assert TC.family_of(labels) == "generic", labels
    raw = TC.run(gpulib, c, DEV)
    assert torch.equal(mu.detach().cpu(), raw["mu"])
    for k, prm in model.named_parameters():
        assert prm.grad is not None and torch.equal(prm.grad.cpu(), raw["grads"][k]), k
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.step()
    assert all(torch.isfinite(prm).all() for prm in model.parameters())
