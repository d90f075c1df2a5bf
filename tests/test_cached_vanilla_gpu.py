"""Cached-context inference for the vanilla family on the MI355X: the one-launch query tail (csrc/np_query.h) - row invariance bit
for bit, values against float64 next to the composed route's, the envelope - and mlhot.cached.condition / predict against the plain
forward, the reference's fixtures and the launch count.  Run with -m gpu."""
import ctypes as C
import functools
import importlib
import types

import pytest
import torch

from tests import np_query_ref as NR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = NR.T, NR.HEADS
DM = [(16, 16), (64, 266)]
NCS = [1, 15, 32]
TILE = 16                      # target rows per workgroup (csrc/np_query.h QT)


def _tanh(d):
    return d == 64             # the shipped width runs decoder0's tanh, the small one the plain head


@functools.lru_cache(maxsize=None)
def _params(d):
    return {k: v.to(DEV) for k, v in NR.params(d).items()}


def _dims(gpulib, d, m, Nc, attend):
    return gpulib.np_dims(T, Nc if attend else 0, 1, 3, NR.Y_DIM, d, d, NR.DIM_Z[d], [100, 100], NR.HIDDEN,
                          "attention" if attend else "mean", _tanh(d), m if attend else 0)


class _Setup:
    """One synthetic case on the device: fused(x) is the kernel, composed(x) the same mathematics from the parent commit's operators."""

    def __init__(self, gpulib, kind, d, m, Nc, Nq, attend):
        from mlhot.ops import favor_keys
        x, k, v, z = NR.case(kind, d, m, Nc, Nq)
        self.lib, self.d, self.attend, self.p = gpulib, d, attend, _params(d)
        self.x = x.to(DEV)
        self.dims = _dims(gpulib, d, m, Nc, attend)
        self.proj = NR.proj_matrix(d, m).to(DEV)
        self.z = z.to(DEV)
        if attend:
            self.vh = v.permute(0, 2, 1, 3).contiguous().to(DEV)                      # [T, Nc, H, d], the head projections' layout
            self.keys = favor_keys(k.permute(0, 2, 1, 3).contiguous().to(DEV), self.proj)
            assert self.keys.route == "cached"
        assert gpulib.np_query_supported(self.dims)

    def fused(self, x):
        x = x.contiguous()
        if self.attend:
            return self.lib.np_query_fwd(self.dims, self.p, x, key_state=self.keys.buf, vh=self.vh, proj=self.proj)
        return self.lib.np_query_fwd(self.dims, self.p, x, z=self.z)

    def composed(self, x):
        from mlhot.cached import composed_tail
        x = x.contiguous()
        rows = x.view(-1, self.d)
        with torch.no_grad():
            if self.attend:
                return composed_tail(self.p, rows, T, x.shape[1], _tanh(self.d), keys=self.keys, vh=self.vh, proj=self.proj)
            return composed_tail(self.p, rows, T, x.shape[1], _tanh(self.d), z=self.z)


SHAPES = [(d, m, Nc, True) for d, m in DM for Nc in NCS] + [(d, m, 0, False) for d, m in DM]
SHAPE_IDS = [f"d{d}-m{m}-Nc{Nc}-{'attention' if a else 'latent'}" for d, m, Nc, a in SHAPES]


# ---- 1. invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,Nc,attend", SHAPES, ids=SHAPE_IDS)
def test_rows_do_not_depend_on_the_launch(gpulib, d, m, Nc, attend):
    s = _Setup(gpulib, "live", d, m, Nc, 100, attend)
    full = s.fused(s.x)
    assert full.shape == (T, 100, NR.Y_DIM) and bool(torch.isfinite(full).all())
    for n in (0, 15, 16, 57, 99):                                     # a row alone
        assert torch.equal(s.fused(s.x[:, n:n + 1]), full[:, n:n + 1]), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17), (5, TILE - 1), (5, TILE + 1), (31, 2 * TILE + 1)):
        assert torch.equal(s.fused(s.x[:, start:start + L]), full[:, start:start + L]), (start, L)
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(s.fused(s.x[:, perm]), full[:, perm])
    big = 3.0 * torch.randn(T, 200, d, generator=torch.Generator().manual_seed(9)).to(DEV)              # other rows, another regime
    big[:, 37:137] = s.x
    assert torch.equal(s.fused(big)[:, 37:137], full)


# ---- 2. values ------------------------------------------------------------------------------------------------------------------
# the key kinds (one key 50 above the rest, all-equal keys) do not reach the latent mode
VALUE_CASES = [(*sh, kind) for sh in SHAPES for kind in (("live", "big", "peak", "equal") if sh[3] else ("live", "big"))]


@pytest.mark.parametrize("d,m,Nc,attend,kind", VALUE_CASES, ids=[f"{i}-{c[4]}" for c in VALUE_CASES for i in [SHAPE_IDS[SHAPES.index(c[:4])]]])
def test_values_against_float64(gpulib, d, m, Nc, attend, kind):
    """The fused launch against float64, next to the composed route (the parent commit's operators: the yardstick) on the same
    inputs: at most twice its error - the orders of summation differ, and at a few 1e-7 that is ulps - and never above U.RTOL."""
    s = _Setup(gpulib, kind, d, m, Nc, 100, attend)
    want = NR.want(kind, d, m, Nc, 100, attend, _tanh(d))
    for Nq in (1, 100):
        fused, composed = s.fused(s.x[:, :Nq]), s.composed(s.x[:, :Nq])
        ef, ec = U.rel_err(fused, want[:, :Nq]), U.rel_err(composed, want[:, :Nq])
        line = f"np_query {kind} d={d} m={m} Nc={Nc} {'attention' if attend else 'latent'} Nq={Nq}: fused {ef:.2e}, composed {ec:.2e} of mu's scale"
        print(line)
        assert bool(torch.isfinite(fused).all()) and ef <= U.RTOL, line
        assert ef <= 2 * ec, line


# ---- 3. envelope ----------------------------------------------------------------------------------------------------------------
# Nc and m do not enter the latent mode: the head width alone there
@pytest.mark.parametrize("Nc,d,m,attend", [(33, 16, 16, True), (4, 24, 32, True), (4, 16, 8, True), (4, 24, 32, False)])
def test_outside_the_envelope(gpulib, Nc, d, m, attend):
    from mlhot.binding import NpParams
    Nq = 5
    dims = gpulib.np_dims(T, Nc if attend else 0, 1, 3, 2, d, d, 12, [100, 100], 100, "attention" if attend else "mean", True, m if attend else 0)
    assert not gpulib.np_query_supported(dims)
    x = torch.randn(T, Nq, d, device=DEV)
    mu = torch.full((T, Nq, 2), 7.0, device=DEV)
    ps = NpParams()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert gpulib.c.mlhot_np_query_fwd(C.byref(dims), C.byref(ps), p(x), Nq, None, None, None, p(mu), None) == 4      # MLHOT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((mu == 7.0).all())


def test_decoder_dimensions_outside_the_envelope(gpulib):
    for dz, dh, y in ((68, 100, 2), (64, 132, 2), (64, 100, 17), (62, 100, 2), (64, 98, 2)):
        assert not gpulib.np_query_supported(gpulib.np_dims(T, 0, 1, 3, y, 64, 64, dz, [100, 100], dh, "mean", True, 0)), (dz, dh, y)
    assert gpulib.np_query_supported(gpulib.np_dims(T, 15, 1, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 266))      # the shipped ANP
    assert gpulib.np_query_supported(gpulib.np_dims(T, 15, 1, 3, 2, 64, 100, 64, [100, 100], 100, "mean", True, 0))            # c1 / c2: dim_r does not enter
    assert not gpulib.np_query_supported(gpulib.np_dims(T, 15, 1, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 288))


# ---- the models -----------------------------------------------------------------------------------------------------------------
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
    # dim_z = 128 is outside the fused launch's envelope: the composed route
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


def _forward(model, cx, cy, qx, at_most=None):
    """The plain test-mode forward; `at_most`: over slices of that many targets (a target's output depends on the context and that
    target only)."""
    with torch.no_grad():
        step = qx.shape[1] if at_most is None else at_most
        return torch.cat([model(cx, cy, qx[:, i:i + step].contiguous(), test=True)[0] for i in range(0, qx.shape[1], step)], dim=1)


@pytest.mark.parametrize("Nc", [0, 1, 5])
@pytest.mark.parametrize("case", SERVED)
def test_predict_equals_the_plain_forward(gpulib, case, Nc):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, Nc, 7)
    want = _forward(model, cx, cy, qx)
    state = cached.condition(model, cx, cy)
    assert state.kind == ("empty" if Nc == 0 else "attention" if model.ATTENTION else "latent")
    got = cached.predict(model, state, qx)
    err = U.rel_err(got, want)
    print(f"predict {case} Nc={Nc}: {err:.2e} of mu's scale, route {state.route}")
    assert state.route == "fused" and got.shape == want.shape and err <= U.RTOL


@pytest.mark.parametrize("case", ["anp_shapenet1d_z128", "cnp_shapenet1d_z128"])
def test_dimensions_outside_the_envelope_take_the_composed_route(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, 5, 7)
    state = cached.condition(model, cx, cy)
    got = cached.predict(model, state, qx)
    err = U.rel_err(got, _forward(model, cx, cy, qx))
    print(f"predict {case}: {err:.2e} of mu's scale, route {state.route}")
    assert state.route == "composed" and err <= U.RTOL
    with pytest.raises(Exception, match="np_query_fwd"):               # a missing kernel is an error, not a quiet other route
        cached.predict(model, state, qx, route="fused")


@pytest.mark.parametrize("case", SERVED)
def test_one_state_serves_several_target_sets(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, _ = _batch(case, 5, 1)
    state = cached.condition(model, cx, cy)
    bitwise = []
    for seed, Nq in ((11, 7), (12, 3), (13, 10), (14, 40)):
        qx = _batch(case, 1, Nq, seed=seed)[2]
        want = _forward(model, cx, cy, qx, at_most=15 if Nq > 15 else None)
        got = cached.predict(model, state, qx)
        err = U.rel_err(got, want)
        print(f"predict {case}, one state, target set of {Nq}: {err:.2e} of mu's scale")
        assert got.shape == want.shape and err <= U.RTOL
        chunked = cached.predict(model, state, qx, chunk=3)
        bitwise.append(torch.equal(chunked, got))
        cerr = U.rel_err(chunked, got)
        print(f"predict {case}, chunk=3 against unchunked at Nq={Nq}: {cerr:.2e}, bit-equal: {bitwise[-1]}")
        assert cerr <= U.RTOL
    print(f"predict {case}: chunked == unchunked bit for bit in {sum(bitwise)} of {len(bitwise)} target sets "
          "(the query tail is row-invariant, so this shows whether the encoder's per-image bits are batch-stable)")


@pytest.mark.parametrize("Nc", [0, 5])
@pytest.mark.parametrize("case", SERVED)
def test_forced_composed_route_agrees_with_the_fused_one(gpulib, case, Nc):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, Nc, 7)
    state = cached.condition(model, cx, cy)
    fused = cached.predict(model, state, qx, route="fused")
    assert state.route == "fused"
    composed = cached.predict(model, state, qx, route="composed")
    assert state.route == "composed"
    err = U.rel_err(composed, fused)
    print(f"predict {case} Nc={Nc}: composed against fused {err:.2e} of mu's scale")
    assert err <= U.RTOL


@pytest.mark.parametrize("name", ["c1_cnp_pascal1d", "c2_cnp_shapenet1d_mean", "c3_anp_shapenet1d"])
def test_predict_against_the_reference_fixtures(gpulib, name):
    """The reference's own numbers: its recorded mu for its own seeded model and inputs."""
    from mlhot import cached
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx).to(DEV).eval()
    cx, qx, cy, _ = (t.to(DEV) for t in U.case_inputs(meta))
    state = cached.condition(model, cx, cy)
    mu = cached.predict(model, state, qx)
    err = U.rel_err(mu, fx["mu"])
    print(f"predict vs the reference ({name}): {err:.2e} of mu's scale, route {state.route}")
    assert state.route == "fused" and err <= U.RTOL


@pytest.mark.parametrize("Nq", [7, 40])
@pytest.mark.parametrize("case", ["anp_shapenet1d", "cnp_shapenet1d_mean"])
def test_predict_is_the_encoder_plus_one_launch(gpulib, case, Nq):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, 5, Nq)
    state = cached.condition(model, cx, cy)
    enc_params = tuple(t.detach() for i in (0, 2, 5, 8) for t in (model.encoder_w0[i].weight, model.encoder_w0[i].bias))
    enc_labels, _ = U.launch_labels(gpulib, lambda: gpulib.enc_vanilla_fwd(qx.reshape(-1, 1, 128, 128), None, enc_params, 64))
    labels, _ = U.launch_labels(gpulib, lambda: cached.predict(model, state, qx))
    print(f"predict {case} Nq={Nq}: {labels}")
    assert enc_labels and labels == enc_labels + ["np.query"]
