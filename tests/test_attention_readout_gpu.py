"""The attention read-out on the MI355X: mlhot_favor_query_weights_fwd - out bit-equal to the plain entry, w against
float64, equal keys, row invariance, nothing written outside w, the masked state, the envelope - and predict(return_attention=True)
of both model families.  Inputs and float64 references: tests/attention_readout_cases.py.  Run with -m gpu.

The bars are the project's U.RTOL for values and Nc 2^-23 for the row sum (one rounding per quotient plus the Nc - 1 of D's sum).
The figures of a run on the MI355X, per input kind, are in profiles/INDEX_attention_readout.md (scripts/attention_readout_probe.py
--test-log reads this file's printed lines)."""
import ctypes as C
import functools
import importlib
import types

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = AC.T, AC.H
TILE = 16                      # query rows per workgroup (csrc/favor_tile.h QT)


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _heads(out, heads):
    """merged [T, N, d*H] (out[t, n, e*H + h]) -> [T, H, N, d]"""
    Tn, N, dh = out.shape
    return out.view(Tn, N, dh // heads, heads).permute(0, 3, 1, 2)


def _rowsum_excess(w):
    """max |sum_n w - 1| with the sum taken in float64"""
    return float((w.double().sum(dim=-1) - 1.0).abs().max())


def _setup(kind, d, m, Nc):
    from mlhot.ops import favor_keys
    q, k, v, proj = AC.inputs(kind, d, m, Nc)
    qd, vd, pd = _dev(q), _dev(v), proj.to(DEV)
    state = favor_keys(_dev(k), pd)
    assert state.route == "cached"
    return qd, state, vd, pd


# ---- 1. out is the plain entry's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_out_is_bit_equal_to_the_plain_entry(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup("live", d, m, Nc)
    for Nq in AC.NQS:
        rows = qd[:, :Nq].contiguous()
        labels, (out, w) = U.launch_labels(gpulib, lambda: favor_query(rows, state, vd, pd, weights=True))
        plain_labels, plain = U.launch_labels(gpulib, lambda: favor_query(rows, state, vd, pd))
        assert labels == ["favor.queryw"] and plain_labels == ["favor.query"]       # one launch each; the default call is the old one
        assert w.shape == (T, H, Nq, Nc) and w.is_contiguous() and w.dtype == torch.float32
        assert torch.equal(out, plain), (Nq,)
        assert torch.equal(out, gpulib.favor_query_fwd(rows, state.buf, vd, pd)), (Nq,)


# ---- 2. values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_weights_against_float64(gpulib, d, m, Nc, kind):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup(kind, d, m, Nc)
    v = AC.inputs(kind, d, m, Nc)[2]
    w64, _ = AC.want(kind, d, m, Nc)
    for Nq in AC.NQS:
        rows = qd[:, :Nq].contiguous()
        out, w = favor_query(rows, state, vd, pd, weights=True)
        assert torch.equal(out, favor_query(rows, state, vd, pd))
        err, excess = U.rel_err(w, w64[:, :, :Nq]), _rowsum_excess(w)
        through = U.rel_err(AR.apply(w.cpu(), v), _heads(out, H))
        line = (f"favor_query weights {kind} d={d} m={m} Nc={Nc} Nq={Nq}: w {err:.2e} of its scale, |sum_n w - 1| {excess:.2e} "
                f"({excess / AC.rowsum_bound(Nc):.2f} of the bound), sum_n w v against out {through:.2e}")
        print(line)
        assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0, line
        assert err <= U.RTOL, line
        assert excess <= AC.rowsum_bound(Nc), line
        assert through <= U.RTOL, line


# ---- 3. equal keys -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_equal_keys_share_one_weight_bit_for_bit(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup("equal", d, m, Nc)
    _, w = favor_query(qd, state, vd, pd, weights=True)
    assert torch.equal(w, w[..., :1].expand_as(w))                   # identical F_k rows go through one summation order


# ---- 4. row invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_weight_rows_do_not_depend_on_the_launch(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup("live", d, m, Nc)
    full = favor_query(qd, state, vd, pd, weights=True)[1]
    assert full.shape == (T, H, 100, Nc) and bool(torch.isfinite(full).all())

    def run(rows):
        return favor_query(rows.contiguous(), state, vd, pd, weights=True)[1]
    for n in (0, 15, 16, 57, 99):                                     # a row alone
        assert torch.equal(run(qd[:, n:n + 1]), full[:, :, n:n + 1]), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17), (5, TILE - 1), (5, TILE + 1), (31, 2 * TILE + 1)):
        assert torch.equal(run(qd[:, start:start + L]), full[:, :, start:start + L]), (start, L)
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(run(qd[:, perm]), full[:, :, perm])
    big = 3.0 * torch.randn(T, 200, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)          # other rows, another regime
    big[:, 37:137] = qd
    assert torch.equal(run(big)[:, :, 37:137], full)


# ---- 5. nothing else written -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", AC.DM[:3])
def test_nothing_is_written_outside_w(gpulib, d, m):
    """Nq 17: a full row tile and a tile of one row; Nc 15: a row length that is no multiple of 4.  w starts 3 floats into its
    buffer, so it has 4-byte alignment and no more."""
    Nq, Nc, lead, guard = 17, 15, 3, 4096
    qd, state, vd, pd = _setup("live", d, m, Nc)
    rows = qd[:, :Nq].contiguous()
    want_out, want_w = gpulib.favor_query_weights_fwd(rows, state.buf, vd, pd)
    n = T * H * Nq * Nc
    buf = torch.full((lead + guard + n + guard,), float("nan"), device=DEV)
    out = torch.full((T, Nq, d * H), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    w = buf[lead + guard:lead + guard + n]
    assert w.data_ptr() % 16 != 0 and w.data_ptr() % 4 == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = gpulib.c.mlhot_favor_query_weights_fwd(p(rows), p(state.buf), p(vd), p(pd), T, H, Nq, Nc, d, m, p(out), p(w), p(ws), 256, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert not bool(torch.isnan(w).any())                            # every element of w is overwritten
    assert bool(torch.isnan(buf[:lead + guard]).all()) and bool(torch.isnan(buf[lead + guard + n:]).all())
    assert torch.equal(w.view(T, H, Nq, Nc), want_w) and torch.equal(out, want_out)


# ---- 6. masked state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", AC.NCS)
@pytest.mark.parametrize("d,m", AC.DM)
def test_masked_columns_are_exact_zeros(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys, favor_query
    for lens in AC.masked_lens(Nc):
        q, kn, vz, proj, w64, out64 = AC.masked("live", d, m, Nc, lens)
        qd, vd, pd = _dev(q)[:, :17].contiguous(), _dev(vz), proj.to(DEV)
        state = favor_keys(_dev(kn), pd, lens=list(lens))
        out, w = favor_query(qd, state, vd, pd, weights=True)
        assert torch.equal(out, favor_query(qd, state, vd, pd))
        assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0
        for t, L in enumerate(lens):
            assert bool((w[t, :, :, L:] == 0.0).all()), (lens, t)
            assert float(w[t, :, :, :L].min()) > 0.0, (lens, t)
        err, excess = U.rel_err(w, w64[:, :, :17]), _rowsum_excess(w)
        print(f"favor_query weights, masked lens={lens} d={d} m={m} Nc={Nc}: w {err:.2e} of its scale, |sum_n w - 1| {excess:.2e} "
              f"({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
        assert err <= U.RTOL and excess <= AC.rowsum_bound(Nc)
        for t, L in enumerate(lens):                                   # ... and on the valid columns of every task on their own
            assert U.rel_err(w[t, :, :, :L], w64[t, :, :17, :L]) <= U.RTOL
        assert U.rel_err(out, _merged(out64[:, :, :17])) <= U.RTOL


def _merged(out):
    Tn, Hn, N, d = out.shape
    return out.permute(0, 2, 3, 1).reshape(Tn, N, d * Hn)


# ---- 7. envelope -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,d,m", [(33, 16, 16), (4, 24, 32), (4, 16, 8)])
def test_outside_the_envelope_nothing_is_written(gpulib, Nc, d, m):
    Nq = 5
    g = torch.Generator().manual_seed(3)
    q, v = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (Nq, Nc))
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((4096,), 7.0, device=DEV)
    out = torch.full((T, Nq, d * H), float("nan"), device=DEV)
    w = torch.full((T, H, Nq, Nc), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    fn = gpulib.c.mlhot_favor_query_weights_fwd
    assert fn(p(q), p(state), p(v), p(proj), T, H, Nq, Nc, d, m, p(out), p(w), p(ws), 256, None) == 4          # MLHOT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(w).all()) and bool((state == 7.0).all())
    assert "favor_query_weights_fwd serves Nc <= 32" in gpulib.c.mlhot_last_error().decode()


def test_a_null_w_is_an_argument_error(gpulib):
    d, m, Nc, Nq = 16, 16, 15, 5
    qd, state, vd, pd = _setup("live", d, m, Nc)
    out = torch.full((T, Nq, d * H), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rows = qd[:, :Nq].contiguous()
    rc = gpulib.c.mlhot_favor_query_weights_fwd(p(rows), p(state.buf), p(vd), p(pd), T, H, Nq, Nc, d, m, p(out), None, p(ws), 256, None)
    torch.cuda.synchronize()
    assert rc == 1 and bool(torch.isnan(out).all())                   # MLHOT_ERR_ARG, before anything is launched
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_keys, favor_query
    g = torch.Generator().manual_seed(3)
    q, k = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (Nq, 33))
    plain = favor_keys(k, pd)                                         # 33 shots: the keys stay outside the envelope
    assert plain.route == "plain"
    with pytest.raises(MlhotError, match="envelope"):
        favor_query(q, plain, k, pd, weights=True)


# ---- 8. the models -----------------------------------------------------------------------------------------------------------------
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFGDIS = dict(task="distractor", img_size=[128, 128, 1], input_dim=2, output_dim=2, img_agg="max", dim_w=16, seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64)
SHAPENET = dict(CFG1D, task="shapenet_1d", input_dim=3, output_dim=2)
PASCAL = dict(CFG1D, task="pascal_1d", input_dim=1, output_dim=1)
MODEL_CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention")),
    "anp_distractor": ("ANPDistractor", dict(CFGDIS, agg_mode="attention")),
    "anp_shapenet1d": ("ANPShapeNet1D", dict(SHAPENET, agg_mode="attention", dim_r=64)),
    "anp_pascal1d": ("ANPVanillaPascal1D", dict(PASCAL, agg_mode="attention", dim_r=64)),
    "cnp_3d_mean": ("CondNeuralProcess", dict(CFG3D, agg_mode="mean")),
    "cnp_shapenet1d_mean": ("CNPShapeNet1D", dict(SHAPENET, agg_mode="mean", dim_r=100)),
}
ATTENTIVE = [c for c in MODEL_CASES if c.startswith("anp")]
NQ = 7


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=2, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _images(case, n, seed):
    """(images [2, n, C, H, W], labels [2, n, L]) on the device."""
    cfg = MODEL_CASES[case][1]
    g = torch.Generator().manual_seed(seed)
    Hh, W, Cc = cfg["img_size"]
    Cc = Cc - 1 if cfg["task"] == "shapenet_3d" else Cc
    return torch.rand(2, n, Cc, Hh, W, generator=g).to(DEV), torch.rand(2, n, cfg["input_dim"], generator=g).to(DEV)


def _plain(model, state, qx, **kw):
    """predict without the keyword on the route the read-out runs: the vanilla family's composed route, ResNetNP's only one"""
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    return cached.predict(model, state, qx, **kw) if isinstance(model, ResNetNP) else cached.predict(model, state, qx, route="composed", **kw)


def _query_heads(model, state, qx, monkeypatch):
    """The query head projections predict hands to favor_query, [T, Nq, heads, d]: the model's own, caught at the call."""
    from mlhot import cached
    from networks import _resnet_np
    seen = []
    for mod in (cached, _resnet_np):
        real = mod.favor_query
        monkeypatch.setattr(mod, "favor_query", lambda qh, *a, _real=real, **kw: (seen.append(qh), _real(qh, *a, **kw))[1])
    cached.predict(model, state, qx, return_attention=True)
    monkeypatch.undo()
    assert len(seen) == 1
    return seen[0]


def _reference(model, state, qh):
    """float64 w from the model's own head projections: the state's kept keys, the caught query heads, the model's projection"""
    cpu = lambda t: t.detach().cpu().permute(0, 2, 1, 3)
    lens = state.keys.lens                                             # None: every slot is a shot
    return AR.weights(cpu(qh), cpu(state.kh), model.attn.projection_matrix.detach().cpu(), lens)


@pytest.mark.parametrize("Nc", [1, 5])
@pytest.mark.parametrize("case", ATTENTIVE)
def test_predict_returns_the_attention_beside_an_unchanged_mu(gpulib, case, Nc, monkeypatch):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model = _model(case)
    cx, cy = _images(case, Nc, 3)
    qx = _images(case, NQ, 4)[0]
    state = cached.condition(model, cx, cy)
    mu, attn = cached.predict(model, state, qx, return_attention=True)
    heads = state.kh.shape[2]
    assert attn.shape == (2, heads, NQ, Nc) and attn.dtype == torch.float32
    assert torch.equal(mu, _plain(model, state, qx))
    if isinstance(model, ResNetNP):                                    # the method is the same call
        mu2, attn2 = model.predict(state, qx, return_attention=True)
        assert torch.equal(mu2, mu) and torch.equal(attn2, attn)
    else:
        assert state.route == "composed"
    assert bool(torch.isfinite(attn).all()) and float(attn.min()) >= 0.0
    assert _rowsum_excess(attn) <= AC.rowsum_bound(Nc)
    cmu, cattn = cached.predict(model, state, qx, chunk=3, return_attention=True)
    assert torch.equal(cmu, _plain(model, state, qx, chunk=3))
    assert cattn.shape == attn.shape and torch.equal(cattn, attn)
    err = U.rel_err(attn, _reference(model, state, _query_heads(model, state, qx, monkeypatch)))
    print(f"predict(return_attention=True) {case} Nc={Nc}: attn {err:.2e} of its scale against float64 on the model's head projections")
    assert err <= U.RTOL


@pytest.mark.parametrize("case", ATTENTIVE)
def test_attention_of_a_ragged_state_and_of_its_extension(gpulib, case, monkeypatch):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 5, 5)
    nx, ny = _images(case, 1, 6)
    qx = _images(case, NQ, 7)[0]
    lens, cap = (1, 5), 8
    state = cached.condition(model, cx, cy, ctx_len=list(lens), capacity=cap)
    mu, attn = cached.predict(model, state, qx, return_attention=True)
    assert attn.shape == (2, state.kh.shape[2], NQ, cap)
    assert torch.equal(mu, _plain(model, state, qx))
    for t, L in enumerate(lens):
        assert bool((attn[t, :, :, L:] == 0.0).all()) and float(attn[t, :, :, :L].min()) > 0.0, t
    assert _rowsum_excess(attn) <= AC.rowsum_bound(cap)
    err = U.rel_err(attn, _reference(model, state, _query_heads(model, state, qx, monkeypatch)))
    print(f"predict(return_attention=True) {case} ctx_len={lens} of {cap} slots: attn {err:.2e} of its scale against float64")
    assert err <= U.RTOL
    grown = cached.extend(model, state, nx, ny)
    assert grown.lens == (2, 6)
    mu2, attn2 = cached.predict(model, grown, qx, return_attention=True)
    assert torch.equal(mu2, _plain(model, grown, qx))
    for t, L in enumerate(lens):
        assert float(attn2[t, :, :, L].min()) > 0.0 and bool((attn2[t, :, :, L + 1:] == 0.0).all()), t      # the new slot's column is in
    assert _rowsum_excess(attn2) <= AC.rowsum_bound(cap)


@pytest.mark.parametrize("case", ["cnp_3d_mean", "cnp_shapenet1d_mean"])
def test_models_without_attention_refuse(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 3, 8)
    qx = _images(case, NQ, 9)[0]
    state = cached.condition(model, cx, cy)
    assert state.kind == "latent"
    with pytest.raises(ValueError, match="has no attention"):
        cached.predict(model, state, qx, return_attention=True)
    assert cached.predict(model, state, qx).shape[:2] == (2, NQ)       # the state still serves the plain call


@pytest.mark.parametrize("case", ["anp_3d", "anp_shapenet1d"])
def test_a_summary_state_and_a_forced_fused_route_refuse(gpulib, case):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    model = _model(case)
    cx, cy = _images(case, 3, 10)
    qx = _images(case, NQ, 11)[0]
    summary = cached.condition(model, cx, cy, form="summary")
    with pytest.raises(ValueError, match="summary state keeps no per-shot rows"):
        cached.predict(model, summary, qx, return_attention=True)
    assert cached.predict(model, summary, qx).shape[:2] == (2, NQ)
    if not isinstance(model, ResNetNP):
        state = cached.condition(model, cx, cy)
        with pytest.raises(ValueError, match='route "fused"'):
            cached.predict(model, state, qx, route="fused", return_attention=True)
        assert cached.predict(model, state, qx) is not None and state.route == "fused"      # the default call keeps its route
