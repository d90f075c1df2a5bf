"""The aggregators and the losses on the MI355X, called directly (tests/agg_loss_cases.py has the cases, the inputs and the
references): agg_fwd / agg_bwd / agg_prefix_fwd past run_foreach's grid clamp, on ties and over BACO's softplus regimes; loss_fwd /
_bwd / _prefix_fwd / _plus_fwd / _plus_bwd through the three regimes of reduce1_block; and the loss VALUE taken by one extra workgroup of
the model's backward (loss_value_block) past its first iteration.  Run with -m gpu.  Worst errors on record: profiles/INDEX_agg_loss.md."""
import importlib
import types

import pytest
import torch

from tests import agg_loss_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- aggregators ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=G.ids)
def test_mean_bitwise(gpulib, shape):
    G.check_mean(gpulib, shape, DEV)


@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=G.ids)
def test_max_ties_bitwise(gpulib, shape):
    G.check_max(gpulib, shape, DEV)


@pytest.mark.parametrize("regime", G.BACO_REGIMES)
@pytest.mark.parametrize("shape", G.BACO_SHAPES, ids=G.ids)
def test_baco_vs_float64_per_column(gpulib, shape, regime):
    G.check_baco(gpulib, shape, regime, DEV)


@pytest.mark.parametrize("regime", G.BACO_REGIMES)
@pytest.mark.parametrize("shape", G.BACO_SHAPES, ids=G.ids)
def test_baco_prefix_rows_have_the_bits_of_agg_fwd(gpulib, shape, regime):
    G.check_prefix_rows_equal_agg_fwd(gpulib, "baco", shape, regime, DEV)


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_prefix_rows_have_the_bits_of_agg_fwd(gpulib, mode):
    G.check_prefix_rows_equal_agg_fwd(gpulib, mode, G.PREFIX_SHAPE, "-", DEV)


def test_agg_refusals(gpulib):
    G.check_agg_refusals(gpulib, DEV)


# ---- losses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", G.LOSS_ROWS)
@pytest.mark.parametrize("case", G.LOSS_KINDS, ids=G.ids)
def test_loss_value_and_gradient_vs_float64(gpulib, case, rows):
    G.check_loss(gpulib, case, rows, DEV)


@pytest.mark.parametrize("P", G.PREFIX_P)
@pytest.mark.parametrize("rows", G.PREFIX_ROWS)
@pytest.mark.parametrize("case", G.LOSS_KINDS, ids=G.ids)
def test_loss_prefix_vs_float64_and_loss_fwd(gpulib, case, rows, P):
    G.check_loss_prefix(gpulib, case, rows, P, DEV)


def test_distractor_row_with_mu_equal_gt(gpulib):
    G.check_distractor_equal_row(gpulib, DEV)


@pytest.mark.parametrize("rows", G.PLUS_ROWS)
@pytest.mark.parametrize("case", G.TRAIN_KINDS, ids=G.ids)
def test_loss_plus_has_the_bits_of_loss_and_axpy(gpulib, case, rows):
    G.check_loss_plus(gpulib, case, rows, DEV)


def test_loss_refusals(gpulib):
    G.check_loss_refusals(gpulib, DEV)


# ---- the loss value from inside the model's backward ------------------------------------------------------------------------
@pytest.mark.parametrize("T", [69, 274], ids=["1035_rows", "4110_rows"])
def test_loss_value_inside_the_models_backward_past_1024_rows(gpulib, T):
    """loss_value_block (csrc/ops_direct.h) repeats reduce1_block's arithmetic for one extra workgroup of the CNP tail's backward; at
    <= 40 rows (test_loss_gradient_taken_inside_the_models_backward) each of its virtual threads sums at most one row.  CNPShapeNet1D
    with mean aggregation at (T, 1, 15): 1035 rows run its `i += 1024` loop, 4110 rows its four-accumulator loop plus a tail.  The
    value left to the backward (ops.loss_value_aside) equals the plain two-node form's and gpulib.loss_fwd on the same mu as floats,
    and all parameter gradients are torch.equal.  (One forward per form: the node's backward releases its scratch, so a second
    backward through the same graph is not possible; the two forwards' mu are asserted equal.)"""
    from mlhot import ops
    from trainer.losses import LossFunc
    Nc, Nq = 1, 15
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=T, input_dim=3, output_dim=2,
                                agg_mode="mean", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=100, dim_z=64, task="shapenet_1d")
    model = getattr(importlib.import_module("networks.CNPShapeNet1D"), "CNPShapeNet1D")(cfg).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    cx, qx = torch.rand(T, Nc, 1, 128, 128, generator=g, device=DEV), torch.rand(T, Nq, 1, 128, 128, generator=g, device=DEV)
    cy, qy = torch.rand(T, Nc, 3, generator=g, device=DEV), torch.rand(T, Nq, 3, generator=g, device=DEV)
    loss_fn = LossFunc("mse", "shapenet_1d")

    def run(aside):
        model.zero_grad(set_to_none=True)
        mu = model(cx, cy, qx)[0]
        if aside:
            with ops.loss_value_aside(enabled=True):
                loss = loss_fn.calc_loss(mu, None, qy)
                loss.backward()
        else:
            loss = loss_fn.calc_loss(mu, None, qy)
            loss.backward()
        torch.cuda.synchronize()
        return loss.item(), mu.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    ref_loss, ref_mu, ref = run(False)
    got_loss, got_mu, got = run(True)
    assert ref_mu.numel() == T * Nq * 2 and T * Nq > 1024 and torch.equal(got_mu, ref_mu)
    direct = gpulib.loss_fwd("azimuth", ref_mu.contiguous(), qy).item()
    print(f"loss value inside the backward, {T * Nq} rows: aside {got_loss!r} two-node {ref_loss!r} loss_fwd {direct!r}")
    assert got_loss == ref_loss == direct
    assert got.keys() == ref.keys() and len(ref) > 0
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
