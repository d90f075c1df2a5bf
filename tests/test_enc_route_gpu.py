"""The vanilla encoder's route on the MI355X (csrc/encoder.h enc_route): which launches run, in which order, for a given
(n, dim_w, options) - counted through mlhot_prof_begin / _end - and the parity of the one mixed route (weight-stationary
convolutions with the generic Linear).  The expected launch lists were recorded with these test bodies on the commit BEFORE
enc_route() existed (two implementations interleaved layer by layer): they pin that the straight-line functions launch what the
interleaving launched.  Run with -m gpu."""
import types

import pytest
import torch

from oracle import ref_cpu as O
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DEFAULTS = U.ENC_OPTION_DEFAULTS
_enc_params, _with_options, _labels = U.enc_params, U.with_options, U.launch_labels     # shared with tests/enc_cases.py


def encoder_labels(gpulib, n, dim_w, opts):
    """(forward labels, backward labels) of one enc_vanilla_fwd + one enc_vanilla_bwd over n random images in two segments."""
    g = torch.Generator().manual_seed(n)
    n0 = (n + 1) // 2
    x0, x1 = torch.rand(n0, 1, 128, 128, generator=g).to(DEV), torch.rand(n - n0, 1, 128, 128, generator=g).to(DEV)
    df = torch.randn(n, dim_w, generator=g).to(DEV)
    plist = [t.to(DEV) for t in _enc_params(dim_w).values()]

    def run():
        fwd, (_, _, saved) = _labels(gpulib, lambda: gpulib.enc_vanilla_fwd(x0, x1 if n > n0 else None, plist, dim_w))
        bwd, _ = _labels(gpulib, lambda: gpulib.enc_vanilla_bwd(x0, x1 if n > n0 else None, plist, dim_w, df[:n0].contiguous(),
                                                                df[n0:].contiguous(), saved))
        torch.cuda.synchronize()
        return fwd, bwd
    return _with_options(gpulib, opts, run)


def model_labels(gpulib, opts):
    """The same for one ANP np_vanilla_fwd / _bwd at T = 2, Nc = Nq = 3, dim_w = 64 (gradients in the library's flat layout)."""
    from networks.ANPShapeNet1D import ANPShapeNet1D
    T, Nc, Nq = 2, 3, 3
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=T, input_dim=3,
                                output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                dim_z=64, task="shapenet_1d")
    model = ANPShapeNet1D(cfg).to(DEV)
    params = {k: p.detach().contiguous() for k, p in model.named_parameters()}
    proj = model.attn.projection_matrix
    dims = gpulib.np_dims(T, Nc, Nq, 3, 2, 64, 64, 64, [100, 100], 100, "attention", model.OUT_TANH, proj.shape[0])
    g = torch.Generator().manual_seed(7)
    cx, qx = torch.rand(T * Nc, 1, 128, 128, generator=g).to(DEV), torch.rand(T * Nq, 1, 128, 128, generator=g).to(DEV)
    cy, dmu = torch.rand(T, Nc, 3, generator=g).to(DEV), torch.randn(T, Nq, 2, generator=g).to(DEV)

    def run():
        fwd, (mu, saved, scratch) = _labels(gpulib, lambda: gpulib.np_vanilla_fwd(dims, params, cx, cy, qx, proj))
        bwd, _ = _labels(gpulib, lambda: gpulib.np_vanilla_bwd(dims, params, cx, cy, qx, mu, dmu, saved, scratch, proj))
        torch.cuda.synchronize()
        return fwd, bwd
    return _with_options(gpulib, opts, run)


# (n, dim_w, options): id -> case.  33: the conv12 grid clamps, the conv3 grids do not; 256: the first n of the merged conv3 backward
ENC_CASES = {
    "n3": (3, 64, {}),
    "n33": (33, 64, {}),
    "n256": (256, 64, {}),
    "n256_conv3_two_launches": (256, 64, {"conv3_bwd_merged": 0}),
    "n256_conv3_nw64": (256, 64, {"conv3_bwd_merged": 64}),
    "n3_dw32": (3, 32, {}),
    "n3_generic": (3, 64, {"conv2_tc": 0}),
    "n3_split": (3, 64, {"conv2_split": 7}),
    "n3_keep_a1": (3, 64, {"materialize_a1": 1}),
}
MODEL_CASES = {"default": {}, "tail_spec_0": {"tail_spec": 0}}

# Recorded on the parent commit by encoder_labels / model_labels above (see the module's docstring).
FWD_WS, BWD_WS_TAIL, BWD_WS, BWD_WS_MERGED = U.ENC_FWD_WS, U.ENC_BWD_WS_TAIL, U.ENC_BWD_WS, U.ENC_BWD_WS_MERGED
ENC_EXPECTED = {
    "n3": (FWD_WS, BWD_WS),
    "n33": (FWD_WS, BWD_WS),
    "n256": (FWD_WS, BWD_WS_MERGED),
    "n256_conv3_two_launches": (FWD_WS, BWD_WS),
    "n256_conv3_nw64": (FWD_WS, BWD_WS_MERGED),
    "n3_dw32": (FWD_WS, ["enc.bwd.linear.dgrad", "enc.bwd.linear.wgrad", "enc.bwd.conv3.wgrad", "enc.bwd.conv3.dgrad"] + BWD_WS_TAIL),
    "n3_generic": (["enc.conv1", "enc.conv2", "enc.pool", "enc.conv3", "enc.linear", "slab_reduce"],
                   ["enc.bwd.linear.dgrad", "enc.bwd.linear.wgrad", "enc.bwd.conv3.wgrad"] + ["enc.bwd.conv3.dgrad"] * 4 +
                   ["enc.bwd.conv2.wgrad"] + ["enc.bwd.conv2.dgrad"] * 4 + ["enc.bwd.conv1.wgrad", "slab_reduce"]),
    "n3_split": (["enc.conv12.split", "enc.conv3", "enc.linear", "slab_reduce"],
                 ["enc.bwd.linear", "enc.bwd.conv3.wgrad", "enc.bwd.conv3.dgrad", "enc.bwd.conv12.wgrad.split", "enc.bwd.conv12.dgrad.split",
                  "slab_reduce", "slab_reduce"]),
    "n3_keep_a1": (["enc.conv1.debug"] + FWD_WS, BWD_WS),
}
MODEL_BWD = ["tail.bwd.C", "tail.bwd.B", "tail.bwd.A", "enc.bwd.linear", "enc.bwd.conv3.wgrad", "enc.bwd.conv3.dgrad", "enc.bwd.conv12.wgrad",
             "enc.bwd.conv12.dgrad", "slab_reduce"]              # flat gradients: conv1's rows and the tail's slabs in the one deferred launch
MODEL_EXPECTED = {
    "default": (["enc.conv12", "enc.conv3", "enc.linear", "tail.A", "tail.B", "tail.C"], MODEL_BWD),         # phase A folds the Linear's partial results
    "tail_spec_0": (["enc.conv12", "enc.conv3", "enc.linear", "slab_reduce", "tail.A", "tail.B", "tail.C"], MODEL_BWD),
}


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_encoder_launch_sequence(gpulib, case):
    n, dim_w, opts = ENC_CASES[case]
    fwd, bwd = encoder_labels(gpulib, n, dim_w, opts)
    print(f"[enc route {case}] forward {fwd}\n[enc route {case}] backward {bwd}")
    assert (fwd, bwd) == ENC_EXPECTED[case]


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_whole_model_launch_sequence(gpulib, case):
    """enc_fold on (default) and off (tail_spec = 0), and the tail's pending slab sum through both hand-overs to the encoder backward."""
    fwd, bwd = model_labels(gpulib, MODEL_CASES[case])
    print(f"[np route {case}] forward {fwd}\n[np route {case}] backward {bwd}")
    assert (fwd, bwd) == MODEL_EXPECTED[case]


def test_encoder_dim_w_32_vs_oracle(gpulib):
    """Weight-stationary convolutions with the generic Linear (dim_w != 64 under conv2_tc = 1), held to test_encoder_fwd_bwd_vs_oracle's
    tolerance; the oracle takes the Linear's shape from the parameters."""
    n0, n1, dim_w = 3, 2, 32
    p = _enc_params(dim_w)
    g = torch.Generator().manual_seed(n0 * 10 + n1)
    x0, x1 = torch.rand(n0, 1, 128, 128, generator=g), torch.rand(n1, 1, 128, 128, generator=g)
    df = torch.randn(n0 + n1, dim_w, generator=g)
    pr = {k: v.clone().requires_grad_() for k, v in p.items()}
    fr = O.vanilla_encoder(torch.cat([x0, x1]), pr)
    fr.backward(df)
    plist = [t.to(DEV) for t in p.values()]

    def run():
        f0, f1, saved = gpulib.enc_vanilla_fwd(x0.to(DEV), x1.to(DEV), plist, dim_w)
        grads = gpulib.enc_vanilla_bwd(x0.to(DEV), x1.to(DEV), plist, dim_w, df[:n0].contiguous().to(DEV), df[n0:].contiguous().to(DEV), saved)
        return torch.cat([f0, f1]), grads
    feat, grads = _with_options(gpulib, {"conv2_tc": 1}, run)
    print(f"[enc dim_w=32] features {U.rel_err(feat, fr):.2e}; " + ", ".join(f"{k} {U.rel_err(got, ref.grad):.2e}" for (k, ref), got in zip(pr.items(), grads)))
    assert U.rel_err(feat, fr) <= U.RTOL
    for (k, ref), got in zip(pr.items(), grads):
        assert U.rel_err(got, ref.grad) <= U.RTOL, k


# every option name mlhot_set_option accepted before the side lane left, with its default
OPTION_DEFAULTS = {"conv2_tc": 1, "conv2_split": 0, "tail_fused": 1, "tail_spec": 7935, "conv3_bwd_merged": 1, "materialize_a1": 0, "dbg": 0,
                   "favor2": 1, "trunk_dual_dgrad": 1, "trunk_wg_rows": 128, "trunk_fuse34": 1}


def test_side_fold_option_is_gone_and_every_other_name_stays(gpulib):
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError, match="unknown option side_fold"):
        gpulib.set_option("side_fold", 1)
    for name, value in OPTION_DEFAULTS.items():
        gpulib.set_option(name, value)
    for bad in (15, 129):
        with pytest.raises(MlhotError, match="trunk_wg_rows: 16 .. 128"):
            gpulib.set_option("trunk_wg_rows", bad)
    with pytest.raises(MlhotError, match="unknown option no_such_switch"):
        gpulib.set_option("no_such_switch", 0)


def test_gpu_build_sizes_are_what_they_were(gpulib):
    """tests/test_reported_sizes.py for the two sizes that differ between the builds: the conv12 block's scratch (GPU build only) and
    the whole model's scratch (the fused tails' per-task slabs).  Recorded from the parent commit's GPU build."""
    import ctypes as C
    from tests.test_reported_sizes import NP
    conv12 = {1: 454400, 32: 14532864, 33: 14532864, 255: 14532864, 256: 14532864, 480: 14532864}
    assert {n: gpulib.c.mlhot_conv12_scratch_bytes(n) for n in conv12} == conv12
    want = {"cnp": 359067904, "anp": 368836864}
    assert {k: gpulib.c.mlhot_np_scratch_bytes(C.byref(gpulib.np_dims(*NP[k][0]))) for k in want} == want
