"""Prefix sweep for the vanilla family on the MI355X: the sweep launch (csrc/np_prefix.h) - invariance bit for bit,
values against float64 next to the composed route's, the envelope - and mlhot.cached.sweep against the plain forward at every
context size, the reference's fixtures, the launch structure and the evaluator.  Run with -m gpu.

Measured on the MI355X (the lines these tests print; profiles/INDEX_prefix_vanilla.md keeps them): see that file."""
import functools
import importlib
import types

import numpy as np
import pytest
import torch

from tests import np_prefix_ref as PR
from tests import np_query_ref as NR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = NR.T, NR.HEADS
DM = [(16, 16), (64, 266)]
NCS = [1, 2, 15, 32]
TILE = 16                      # target rows per workgroup (csrc/np_prefix.h)


def _tanh(d):
    return d == 64


@functools.lru_cache(maxsize=None)
def _params(d):
    return {k: v.to(DEV) for k, v in NR.params(d).items()}


def _dims(gpulib, d, m, Nc, attend):
    return gpulib.np_dims(T, Nc, 1, 3, NR.Y_DIM, d, d, NR.DIM_Z[d], [100, 100], NR.HIDDEN, "attention" if attend else "mean", _tanh(d), m if attend else 0)


class _Setup:
    """One synthetic case on the device: fused(x, ks) is the sweep launch, composed(x, ks) the parent commit's operators per k."""

    def __init__(self, gpulib, kind, d, m, Nc, Nq, attend):
        x, k, v, z = PR.case(kind, d, m, Nc, Nq)
        self.lib, self.d, self.Nc, self.attend, self.p = gpulib, d, Nc, attend, _params(d)
        self.x = x.to(DEV)
        self.dims = _dims(gpulib, d, m, Nc, attend)
        self.proj = NR.proj_matrix(d, m).to(DEV)
        self.z = z.to(DEV)
        self.kh = k.permute(0, 2, 1, 3).contiguous().to(DEV)                          # [T, Nc, H, d], the head projections' layout
        self.vh = v.permute(0, 2, 1, 3).contiguous().to(DEV)
        assert gpulib.np_prefix_supported(self.dims, Nc)

    def fused(self, x, ks=None):
        ks = list(range(1, self.Nc + 1)) if ks is None else list(ks)
        x = x.contiguous()
        if self.attend:
            return self.lib.np_prefix_fwd(self.dims, self.p, x, ks, kh=self.kh, vh=self.vh, proj=self.proj)
        return self.lib.np_prefix_fwd(self.dims, self.p, x, ks, z=self.z[[k - 1 for k in ks]].contiguous())

    def keys(self, k):
        from mlhot.ops import favor_keys
        return favor_keys(self.kh, self.proj, lens=(k,) * T)

    def composed(self, x, ks=None):
        from mlhot.cached import composed_tail
        ks = list(range(1, self.Nc + 1)) if ks is None else list(ks)
        x = x.contiguous()
        rows = x.view(-1, self.d)
        with torch.no_grad():
            if self.attend:
                return torch.stack([composed_tail(self.p, rows, T, x.shape[1], _tanh(self.d), keys=self.keys(k), vh=self.vh, proj=self.proj) for k in ks])
            return torch.stack([composed_tail(self.p, rows, T, x.shape[1], _tanh(self.d), z=self.z[k - 1].contiguous()) for k in ks])

    def predict(self, x, k):
        """np_query_fwd against the masked state of the first k shots (the cached-context route at that context size)."""
        if self.attend:
            return self.lib.np_query_fwd(self.dims, self.p, x.contiguous(), key_state=self.keys(k).buf, vh=self.vh, proj=self.proj)
        return self.lib.np_query_fwd(_dims(self.lib, self.d, 0, 0, False), self.p, x.contiguous(), z=self.z[k - 1].contiguous())


SHAPES = [(d, m, Nc, a) for a in (True, False) for d, m in DM for Nc in NCS]
SHAPE_IDS = [f"d{d}-m{m}-Nc{Nc}-{'attention' if a else 'latent'}" for d, m, Nc, a in SHAPES]


# ---- 1. invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,Nc,attend", SHAPES, ids=SHAPE_IDS)
def test_prefixes_do_not_depend_on_the_other_prefixes(gpulib, d, m, Nc, attend):
    s = _Setup(gpulib, "live", d, m, Nc, 17, attend)
    full = s.fused(s.x)
    assert full.shape == (Nc, T, 17, NR.Y_DIM) and bool(torch.isfinite(full).all())
    b = PR.group_boundary("live", d, m, Nc)
    for k in sorted({1, b, max(b - 1, 1), Nc}):                       # a prefix alone: the first, one that opens a group, its neighbour, the last
        assert torch.equal(s.fused(s.x, [k])[0], full[k - 1]), k
    for ks in ([1, Nc], list(range(1, Nc + 1, 2)), list(range(2, Nc + 1, 3)), list(range(max(Nc - 9, 1), Nc + 1)), [b]):
        ks = sorted(set(k for k in ks if 1 <= k <= Nc))
        if ks:
            assert torch.equal(s.fused(s.x, ks), full[[k - 1 for k in ks]]), ks


@pytest.mark.parametrize("kind", ["peak_first", "peak_last", "climb"])
def test_prefixes_alone_at_every_grouping(gpulib, kind):
    """One group, a last prefix alone in its group, every prefix its own group: each prefix alone gives its row of the full sweep."""
    d, m, Nc = 64, 266, 15
    s = _Setup(gpulib, kind, d, m, Nc, 5, True)
    full = s.fused(s.x)
    for k in range(1, Nc + 1):
        assert torch.equal(s.fused(s.x, [k])[0], full[k - 1]), k


@pytest.mark.parametrize("d,m,Nc,attend", SHAPES, ids=SHAPE_IDS)
def test_rows_do_not_depend_on_the_launch(gpulib, d, m, Nc, attend):
    s = _Setup(gpulib, "live", d, m, Nc, 100, attend)
    full = s.fused(s.x)
    assert full.shape == (Nc, T, 100, NR.Y_DIM) and bool(torch.isfinite(full).all())
    for Nq in (1, 15, 16, 17, 100):                                   # the leading rows as a launch of their own
        assert torch.equal(s.fused(s.x[:, :Nq]), full[:, :, :Nq]), Nq
    for n in (15, 16, 57, 99):                                        # a row alone
        assert torch.equal(s.fused(s.x[:, n:n + 1]), full[:, :, n:n + 1]), n
    for start, L in ((3, 15), (3, 16), (3, 17), (5, TILE - 1), (5, TILE + 1), (31, 2 * TILE + 1)):
        assert torch.equal(s.fused(s.x[:, start:start + L]), full[:, :, start:start + L]), (start, L)
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(s.fused(s.x[:, perm]), full[:, :, perm])
    big = 3.0 * torch.randn(T, 200, d, generator=torch.Generator().manual_seed(9)).to(DEV)              # other rows, another regime
    big[:, 37:137] = s.x
    assert torch.equal(s.fused(big)[:, :, 37:137], full)


# ---- 2. values ------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(*sh, kind) for sh in SHAPES for kind in (PR.ATTENTION_KINDS if sh[3] else PR.LATENT_KINDS)]


@pytest.mark.parametrize("d,m,Nc,attend,kind", VALUE_CASES, ids=[f"{SHAPE_IDS[SHAPES.index(c[:4])]}-{c[4]}" for c in VALUE_CASES])
def test_values_against_float64(gpulib, d, m, Nc, attend, kind):
    """The sweep launch against float64 for every prefix, next to the composed route (the parent commit's operators, one masked
    state and one composed tail per k) on the same inputs: at most twice its error and never above U.RTOL - the rule of
    test_cached_vanilla_gpu.py::test_values_against_float64.

    The sweep launch follows the composed route's arithmetic step by step (the same accumulator chains, favor_cached.h's diag_q,
    r = merged Wo^T in linear_rows' order); measured on the MI355X its error equals the composed route's in every printed line,
    the largest 1.46e-06 of mu's scale (profiles/INDEX_prefix_vanilla.md)."""
    s = _Setup(gpulib, kind, d, m, Nc, 100, attend)
    want = PR.want(kind, d, m, Nc, 100, attend, _tanh(d))
    for Nq in (1, 100):
        fused, composed = s.fused(s.x[:, :Nq]), s.composed(s.x[:, :Nq])
        same = [bool(torch.equal(fused[k - 1], s.predict(s.x[:, :Nq], k))) for k in range(1, Nc + 1)]
        worst = None
        for k in range(1, Nc + 1):
            ef, ec = U.rel_err(fused[k - 1], want[k - 1, :, :Nq]), U.rel_err(composed[k - 1], want[k - 1, :, :Nq])
            if worst is None or ef > worst[1]:
                worst = (k, ef, ec)
        tag = f"np_prefix {kind} d={d} m={m} Nc={Nc} {'attention' if attend else 'latent'} Nq={Nq}"
        print(f"{tag}: worst prefix k={worst[0]}: fused {worst[1]:.2e}, composed {worst[2]:.2e} of mu's scale; "
              f"fused == predict(condition(ctx_len=k)) bit for bit at {sum(same)} of {Nc} prefixes")
        assert bool(torch.isfinite(fused).all()), tag
        for k in range(1, Nc + 1):
            ef, ec = U.rel_err(fused[k - 1], want[k - 1, :, :Nq]), U.rel_err(composed[k - 1], want[k - 1, :, :Nq])
            line = f"{tag} k={k}: fused {ef:.2e}, composed {ec:.2e}"
            assert ef <= U.RTOL, line
            assert ef <= 2 * ec, line


# ---- 3. envelope ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Nc,d,m,attend", [(33, 32, 16, 16, True), (4, 33, 16, 16, True), (4, 33, 16, 16, False), (4, 4, 24, 32, True),
                                             (4, 4, 16, 8, True), (4, 4, 24, 32, False)])
def test_outside_the_envelope(gpulib, K, Nc, d, m, attend):
    import ctypes as C
    from mlhot.binding import MlhotError, NpParams
    Nq = 5
    dims = gpulib.np_dims(T, Nc, 1, 3, 2, d, d, 12, [100, 100], 100, "attention" if attend else "mean", True, m if attend else 0)
    assert not gpulib.np_prefix_supported(dims, K)
    x = torch.randn(T, Nq, d, device=DEV)
    mu = torch.full((K, T, Nq, 2), 7.0, device=DEV)
    ks = (C.c_int32 * K)(*range(1, K + 1))
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = gpulib.c.mlhot_np_prefix_fwd(C.byref(dims), C.byref(NpParams()), p(x), Nq, ks, K, None, None, None, p(mu), None, 0, None)
    assert rc == 4 and "np_prefix_fwd" in gpulib.c.mlhot_last_error().decode()      # MLHOT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((mu == 7.0).all())
    with pytest.raises(MlhotError, match="np_prefix_fwd"):
        gpulib.np_prefix_fwd(dims, {}, x, list(range(1, K + 1)), z=torch.zeros(K, T, 12, device=DEV))


def test_decoder_dimensions_outside_the_envelope(gpulib):
    for dz, dh, y in ((68, 100, 2), (64, 132, 2), (64, 100, 17), (62, 100, 2), (64, 98, 2)):
        assert not gpulib.np_prefix_supported(gpulib.np_dims(T, 5, 1, 3, y, 64, 64, dz, [100, 100], dh, "mean", True, 0), 5), (dz, dh, y)
    assert gpulib.np_prefix_supported(gpulib.np_dims(T, 15, 1, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 266), 15)      # the shipped ANP
    assert gpulib.np_prefix_supported(gpulib.np_dims(T, 32, 1, 3, 2, 64, 100, 64, [100, 100], 100, "mean", True, 0), 32)
    assert not gpulib.np_prefix_supported(gpulib.np_dims(T, 15, 1, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 266), 0)


# ---- 4. the models --------------------------------------------------------------------------------------------------------------
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64)
SHAPENET = dict(CFG1D, task="shapenet_1d", input_dim=3, output_dim=2)
PASCAL = dict(CFG1D, task="pascal_1d", input_dim=1, output_dim=1)
MODEL_CASES = {
    "anp_shapenet1d": ("ANPShapeNet1D", dict(SHAPENET, agg_mode="attention", dim_r=64)),
    "anp_pascal1d": ("ANPVanillaPascal1D", dict(PASCAL, agg_mode="attention", dim_r=64)),
    "cnp_shapenet1d_mean": ("CNPShapeNet1D", dict(SHAPENET, agg_mode="mean", dim_r=100)),
    "cnp_shapenet1d_max": ("CNPShapeNet1D", dict(SHAPENET, agg_mode="max", dim_r=100)),
    "cnp_shapenet1d_baco": ("CNPShapeNet1D", dict(SHAPENET, agg_mode="baco", dim_r=256)),
    "cnp_pascal1d": ("CNPVanillaPascal1D", dict(PASCAL, agg_mode="mean", dim_r=100)),
    # dim_z = 128 is outside the sweep launch's envelope: the composed route
    "anp_shapenet1d_z128": ("ANPShapeNet1D", dict(SHAPENET, agg_mode="attention", dim_r=64, dim_z=128)),
    "cnp_shapenet1d_z128": ("CNPShapeNet1D", dict(SHAPENET, agg_mode="mean", dim_r=100, dim_z=128)),
}
SERVED = [c for c in MODEL_CASES if not c.endswith("z128")]


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=2, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _batch(case, Nc, Nq, seed=3):
    g = torch.Generator().manual_seed(seed)
    cx, qx = torch.rand(2, Nc, 1, 128, 128, generator=g), torch.rand(2, Nq, 1, 128, 128, generator=g)
    return cx.to(DEV), torch.rand(2, Nc, MODEL_CASES[case][1]["input_dim"], generator=g).to(DEV), qx.to(DEV)


@functools.lru_cache(maxsize=None)
def _plain(case, Nc, Nq):
    """The plain test-mode forward at every context size 1..Nc: [Nc, T, Nq, y]."""
    cx, cy, qx = _batch(case, Nc, Nq)
    with torch.no_grad():
        return torch.stack([_model(case)(cx[:, :k].contiguous(), cy[:, :k].contiguous(), qx, test=True)[0] for k in range(1, Nc + 1)])


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_sweep_equals_the_plain_forward_at_every_context_size(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, 5, 7)
    want = _plain(case, 5, 7)
    got = cached.sweep(model, cx, cy, qx)
    route = cached.sweep.last_route
    errs = [U.rel_err(got[k], want[k]) for k in range(5)]
    print(f"sweep {case}: route {route}, per context size {' '.join(f'{e:.2e}' for e in errs)} of mu's scale")
    assert route == ("composed" if case.endswith("z128") else "fused") and got.shape == want.shape and max(errs) <= U.RTOL
    sub = cached.sweep(model, cx, cy, qx, ks=[2, 5])
    assert sub.shape == (2, *want.shape[1:]) and max(U.rel_err(sub[0], want[1]), U.rel_err(sub[1], want[4])) <= U.RTOL


@pytest.mark.parametrize("case", ["anp_shapenet1d_z128", "cnp_shapenet1d_z128"])
def test_forcing_the_fused_route_outside_the_envelope_raises(gpulib, case):
    from mlhot import cached
    cx, cy, qx = _batch(case, 5, 7)
    with pytest.raises(ValueError, match="np_prefix_fwd"):            # a missing kernel is an error, not a quiet other route
        cached.sweep(_model(case), cx, cy, qx, route="fused")


@pytest.mark.parametrize("case", SERVED)
def test_forced_composed_route_agrees_with_the_fused_one(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, 5, 7)
    fused = cached.sweep(model, cx, cy, qx, route="fused")
    assert cached.sweep.last_route == "fused"
    composed = cached.sweep(model, cx, cy, qx, route="composed")
    assert cached.sweep.last_route == "composed"
    err = max(U.rel_err(fused[k], composed[k]) for k in range(5))
    print(f"sweep {case}: fused against composed {err:.2e} of mu's scale")
    assert err <= U.RTOL


# ---- 5. the reference's fixtures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_cnp_pascal1d", "c2_cnp_shapenet1d_mean", "c3_anp_shapenet1d"])
def test_last_prefix_against_the_reference_fixtures(gpulib, name):
    from mlhot import cached
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx).to(DEV).eval()
    cx, qx, cy, _ = (t.to(DEV) for t in U.case_inputs(meta))
    mu = cached.sweep(model, cx, cy, qx, ks=[cx.shape[1]])
    err = U.rel_err(mu[-1], fx["mu"])
    print(f"sweep vs the reference ({name}): {err:.2e} of mu's scale, route {cached.sweep.last_route}")
    assert cached.sweep.last_route == "fused" and err <= U.RTOL


# ---- 6. launch structure --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["anp_shapenet1d", "cnp_shapenet1d_mean"])
def test_sweep_is_one_encoder_pass_and_one_tail_launch(gpulib, case):
    from mlhot import cached
    model = _model(case)
    Nc = 5
    cx, cy, qx = _batch(case, Nc, 7)
    enc_params = tuple(t.detach() for i in (0, 2, 5, 8) for t in (model.encoder_w0[i].weight, model.encoder_w0[i].bias))
    enc_labels, _ = U.launch_labels(gpulib, lambda: gpulib.enc_vanilla_fwd(cx.reshape(-1, 1, 128, 128), qx.reshape(-1, 1, 128, 128), enc_params, 64))
    lists = [U.launch_labels(gpulib, lambda ks=ks: cached.sweep(model, cx, cy, qx, ks=ks))[0] for ks in ([1], [Nc], None)]
    print(f"sweep {case}: {lists[2]}")
    assert enc_labels and lists[0] == lists[1] == lists[2]
    assert lists[2][:len(enc_labels)] == enc_labels and sum(l.startswith("enc.") for l in lists[2]) == sum(l.startswith("enc.") for l in enc_labels)
    assert lists[2].count("np.prefix") == 1 and lists[2][-1] == "np.prefix" and "np.query" not in lists[2]


# ---- 7. the evaluator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("case", ["anp_shapenet1d", "cnp_shapenet1d_mean"])
def test_evaluator_paired_sweep_against_the_plain_forward(gpulib, tmp_path, case, fold):
    """evaluate() with prefix_sweep = "paired" on the 1D synthetic loader: the logged losses equal the plain forward's on the same
    recorded batches at every context size (relative 1e-4 on the loss); prefix_sweep = True still refuses the loader."""
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot.synth import SyntheticData, host_convert
    from trainer.losses import LossFunc
    method, base = MODEL_CASES[case]
    K, n_iter = 4, 2
    logs = []
    cfg = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=2, iterations=0, val_iters=n_iter, max_ctx_num=K, contrastive=False,
                                logger=types.SimpleNamespace(info=logs.append), save_path=str(tmp_path), prefix_sweep="paired", **base)
    if fold:
        cfg.prefix_sweep_fold = True
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
    loss = LossFunc("mse", "shapenet_1d")

    class Recording(SyntheticData):
        taken = []

        def get_batch_u8(self, source, tasks_per_batch, shot):
            out = super().get_batch_u8(source, tasks_per_batch, shot)
            Recording.taken.append((source, shot, out))
            return out
    Recording.taken = []
    ev = ModelEvaluator(model=model, loss=loss, config=cfg, data=Recording("shapenet_1d"))
    val, test = ev.evaluate()
    assert any("paired" in m and "same tasks at every context size" in m for m in logs)
    for source, res in (("validation", val), ("test", test)):
        batches = [b for s, shot, b in Recording.taken if s == source and shot == K][-n_iter:]       # the sweep's own draws follow the property check's
        assert len(batches) == n_iter
        for k in range(1, K + 1):
            vals = []
            with torch.no_grad():
                for xs, xq, ys, yq in batches:
                    cx, qx = host_convert(xs).to(DEV), host_convert(xq).to(DEV)
                    mu = model.eval()(cx[:, :k].contiguous(), ys[:, :k].contiguous().to(DEV), qx, test=True)[0]
                    vals.append(loss.calc_loss(mu, None, yq.to(DEV), test=True).item())
            mean, std = float(np.mean(vals)), float(np.std(vals, ddof=1))
            print(f"[paired sweep {case} fold={fold}] {source} k={k}: mean {res[0][k - 1]:.6f} vs plain {mean:.6f}, std {res[1][k - 1]:.6f} vs {std:.6f}")
            assert abs(res[0][k - 1] - mean) <= 1e-4 * abs(mean), (source, k)
    cfg.prefix_sweep = True
    with pytest.raises(ValueError, match="not a prefix"):
        ev.evaluate()
