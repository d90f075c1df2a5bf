"""Cached-context inference on the MI355X: the split FAVOR+ kernels (csrc/favor_cached.h) - row invariance bit for bit, values and
the key state against float64, the envelope - and ResNetNP.condition / predict against the plain forward and the reference's
fixtures.  Run with -m gpu."""
import ctypes as C
import functools
import importlib
import os
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import favor_cached_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = 2, 2
DM = [(16, 16), (64, 266), (256, 1419), (256, 1536)]
NCS = [1, 15, 32]
TILE = 16                      # query rows per workgroup (csrc/favor_tile.h QT)


@functools.lru_cache(maxsize=None)
def _proj(d, m):
    if (d, m) == (64, 266):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor.npz"))["d64_big/proj"])
    if (d, m) == (256, 1419):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor_c5.npz"))["proj"])
    with torch.random.fork_rng():
        torch.manual_seed(77 + m)
        return O.gaussian_orthogonal_random_matrix(m, d).float()


@functools.lru_cache(maxsize=None)
def _inputs(kind, d, m, Nc, Nq):
    """(q, k, v, proj) in the oracle's layout [T, H, N, d], on the CPU."""
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nc + len(kind))
    q = 0.25 * torch.randn(T, H, Nq, d, generator=g)
    k = 0.25 * torch.randn(T, H, Nc, d, generator=g)
    v = torch.randn(T, H, Nc, d, generator=g)
    if kind == "big":                    # favor.npz's large-norm case: its own tensors where the shape is its own, the live regime x 4 elsewhere
        q, k = 4 * q, 4 * k
        if (d, m) == (64, 266):
            fx = np.load(os.path.join(U.GOLDEN, "favor.npz"))
            fq, fk, fv = (torch.from_numpy(fx[f"d64_big/{n}"]) for n in ("q", "k", "v"))       # [2, 8, 15, 64]: heads 0..H-1, shots cycled
            q = fq[:, :H][:, :, torch.arange(Nq) % fq.shape[2]].contiguous()
            k, v = fk[:, :H, torch.arange(Nc) % 15].contiguous(), fv[:, :H, torch.arange(Nc) % 15].contiguous()
    elif kind == "peak":                 # one key whose dd maximum sits ~50 above the rest: most key features are the 1e-4 floor
        k = 0.05 * torch.randn(T, H, Nc, d, generator=g)
        p = _proj(d, m)[m // 2]
        k[1, 0, Nc - 1] = p * (50.0 / (d ** -0.25 * float(p @ p)))
    elif kind == "equal":                # all keys equal
        k = k[:1, :1, :1].expand(T, H, Nc, d).contiguous()
    else:
        assert kind == "live"
    return q, k, v, _proj(d, m)


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


# ---- 1. invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", NCS)
@pytest.mark.parametrize("d,m", DM)
def test_query_rows_do_not_depend_on_the_launch(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys, favor_query
    q, k, v, proj = _inputs("live", d, m, Nc, 100)
    qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
    state = favor_keys(kd, pd)
    assert state.route == "cached"
    full = favor_query(qd, state, vd, pd)
    assert full.shape == (T, 100, d * H) and bool(torch.isfinite(full).all())

    def run(rows):
        return favor_query(rows.contiguous(), state, vd, pd)
    for n in (0, 15, 16, 57, 99):                                     # a row alone
        assert torch.equal(run(qd[:, n:n + 1]), full[:, n:n + 1]), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17), (5, TILE - 1), (5, TILE + 1), (31, 2 * TILE + 1)):
        assert torch.equal(run(qd[:, start:start + L]), full[:, start:start + L]), (start, L)
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(run(qd[:, perm]), full[:, perm])
    big = 3.0 * torch.randn(T, 200, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)          # other rows, another regime
    big[:, 37:137] = qd
    assert torch.equal(run(big)[:, 37:137], full)


# ---- 2. value -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["live", "big", "peak", "equal"])
@pytest.mark.parametrize("Nc", NCS)
@pytest.mark.parametrize("d,m", DM)
def test_query_values_against_float64(gpulib, d, m, Nc, kind):
    from mlhot.ops import favor_keys, favor_query
    q, k, v, proj = _inputs(kind, d, m, Nc, 100)
    if kind == "peak":
        dd = torch.einsum("thnd,md->thnm", d ** -0.25 * k.double(), proj.double())
        peak = dd[1, 0, Nc - 1].max().item()
        dd[1, 0, Nc - 1] = -1e30
        assert abs(peak - 50) < 1e-3 and 45 < peak - dd.max().item() < 55, (peak, dd.max().item())      # 50 above every other key
    want = R.merged(R.attention(q, k, v, proj))                       # row-wise in q: the rows of a smaller Nq are its first rows
    qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
    state = favor_keys(kd, pd)
    assert state.route == "cached"
    for Nq in (1, 16, 33, 100):
        got = favor_query(qd[:, :Nq].contiguous(), state, vd, pd)
        err = U.rel_err(got, want[:, :Nq])
        line = f"favor_query {kind} d={d} m={m} Nc={Nc} Nq={Nq}: {err:.2e} of out's scale"
        if Nq <= 32:
            plain = gpulib.favor_fwd(qd[:, :Nq].contiguous(), kd, vd, pd)[0]
            line += f"; mlhot_favor_fwd {U.rel_err(plain, want[:, :Nq]):.2e}"
        print(line)
        assert bool(torch.isfinite(got).all()) and err <= U.RTOL, line


# ---- 3. key state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["live", "big", "peak", "equal"])
@pytest.mark.parametrize("Nc", NCS)
@pytest.mark.parametrize("d,m", DM)
def test_key_state_against_float64(gpulib, d, m, Nc, kind):
    from mlhot.ops import favor_keys
    _, k, _, proj = _inputs(kind, d, m, Nc, 100)
    state = favor_keys(_dev(k), proj.to(DEV))
    fk, M = state.features()
    mp = (m + 15) // 16 * 16
    assert fk.shape == (T, H, Nc, mp) and gpulib.favor_keys_bytes(T, H, Nc, d, m) >= 4 * (fk.numel() + 1)
    want, wantM = R.key_features(k, proj)
    dd_scale = torch.einsum("thnd,md->thnm", d ** -0.25 * k.double(), proj.double()).abs().max().item()
    eF, eM = U.rel_err(fk[..., :m], want), abs(M.item() - wantM.item()) / max(dd_scale, 1e-30)
    print(f"favor_keys {kind} d={d} m={m} Nc={Nc}: F_k {eF:.2e} of its scale, M {M.item():.4f} off by {eM:.2e} of dd's scale")
    assert eF <= U.RTOL and eM <= U.RTOL
    assert (mp > m) == (m in (266, 1419))
    assert bool((fk[..., m:] == 0).all())                               # features >= m are exactly zero
    assert float(fk[..., :m].min()) >= m ** -0.5 * 1e-4 * (1 - 1e-6)      # the floor is in


# ---- 4. envelope ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,d,m", [(33, 16, 16), (4, 24, 32), (4, 16, 8)])
def test_outside_the_envelope(gpulib, Nc, d, m):
    from mlhot.ops import favor_keys, favor_query
    Nq = 5
    assert gpulib.favor_keys_bytes(T, H, Nc, d, m) == 0
    assert gpulib.c.mlhot_favor_query_ws_bytes(T, H, Nq, Nc, d, m) == 0
    g = torch.Generator().manual_seed(3)
    q, k, v = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (Nq, Nc, Nc))
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((4096,), 7.0, device=DEV)
    out = torch.full((T, Nq, d * H), 7.0, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert gpulib.c.mlhot_favor_keys_fwd(p(k), p(proj), T, H, Nc, d, m, p(state), 4 * state.numel(), None) == 4       # MLHOT_ERR_UNSUPPORTED
    assert gpulib.c.mlhot_favor_query_fwd(p(q), p(state), p(v), p(proj), T, H, Nq, Nc, d, m, p(out), p(ws), 256, None) == 4
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((out == 7.0).all())
    # the operators keep the keys and run mlhot_favor_fwd
    st = favor_keys(k, proj)
    assert st.route == "plain"
    assert torch.equal(favor_query(q, st, v, proj), gpulib.favor_fwd(q, k, v, proj)[0])


# ---- the model ------------------------------------------------------------------------------------------------------------------
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFGDIS = dict(task="distractor", img_size=[128, 128, 1], input_dim=2, output_dim=2, img_agg="max", dim_w=16, seed=2578, temperature=0.07)
MODEL_CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention")),
    "cnp_3d_mean": ("CondNeuralProcess", dict(CFG3D, agg_mode="mean")),
    "cnp_3d_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max")),
    "cnp_3d_baco": ("CondNeuralProcess", dict(CFG3D, agg_mode="baco")),
    "anp_distractor": ("ANPDistractor", dict(CFGDIS, agg_mode="attention")),
}


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=2, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _batch(cfg, Nc, Nq, seed=3):
    g = torch.Generator().manual_seed(seed)
    Hh, W, Cc = cfg["img_size"]
    Cc = Cc - 1 if cfg["task"] == "shapenet_3d" else Cc
    cx, qx = torch.rand(2, Nc, Cc, Hh, W, generator=g), torch.rand(2, Nq, Cc, Hh, W, generator=g)
    return cx.to(DEV), torch.rand(2, Nc, cfg["input_dim"], generator=g).to(DEV), qx.to(DEV)


@pytest.mark.parametrize("Nc", [0, 1, 5])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_predict_equals_the_plain_forward(gpulib, case, Nc):
    model = _model(case)
    cx, cy, qx = _batch(MODEL_CASES[case][1], Nc, 7)
    with torch.no_grad():
        want = model(cx, cy, qx, test=True)[0]
    state = model.condition(cx, cy)
    assert state.kind == ("empty" if Nc == 0 else "attention" if model.ATTENTION else "latent")
    got = model.predict(state, qx)
    err = U.rel_err(got, want)
    print(f"predict {case} Nc={Nc}: {err:.2e} of mu's scale")
    assert got.shape == want.shape and err <= U.RTOL


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_one_state_serves_several_target_sets(gpulib, case):
    model = _model(case)
    cfg = MODEL_CASES[case][1]
    cx, cy, _ = _batch(cfg, 5, 1)
    state = model.condition(cx, cy)
    bitwise = []
    for seed, Nq in ((11, 7), (12, 3), (13, 10)):
        qx = _batch(cfg, 1, Nq, seed=seed)[2]
        with torch.no_grad():
            want = model(cx, cy, qx, test=True)[0]
        got = model.predict(state, qx)
        err = U.rel_err(got, want)
        print(f"predict {case}, one state, target set of {Nq}: {err:.2e} of mu's scale")
        assert err <= U.RTOL
        chunked = model.predict(state, qx, chunk=3)
        bitwise.append(torch.equal(chunked, got))
        cerr = U.rel_err(chunked, got)
        print(f"predict {case}, chunk=3 against unchunked at Nq={Nq}: {cerr:.2e}, bit-equal: {bitwise[-1]}")
        assert cerr <= U.RTOL
    print(f"predict {case}: chunked == unchunked bit for bit in {sum(bitwise)} of {len(bitwise)} target sets "
          "(everything behind the trunks is row-invariant, so this shows whether the trunks' per-image bits are batch-stable)")


@pytest.mark.parametrize("name", ["p_anp_shapenet3d", "p_cnp_shapenet3d_max"])
def test_predict_against_the_reference_fixtures(gpulib, name):
    """The reference's own ANP / CondNeuralProcess at the fixtures' full context size K."""
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx).to(DEV).eval()
    views = torch.from_numpy(fx["views_u8"]).float().div(255.0).permute(0, 1, 4, 2, 3).contiguous().to(DEV)
    labels = torch.from_numpy(fx["labels"]).to(DEV)
    K = meta["K"]
    mu = model.predict(model.condition(views[:, :K].contiguous(), labels[:, :K].contiguous()), views)
    err = U.rel_err(mu, fx["mu"][K - 1])
    print(f"predict vs the reference ({name}, K = {K}): {err:.2e} of mu's scale")
    assert err <= U.RTOL
