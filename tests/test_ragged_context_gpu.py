"""Per-task context sizes and growing states on the MI355X: the masked key state (mlhot_favor_keys_ragged_fwd)
against the unmasked entry bit for bit at full lengths and against float64 (tests/ragged_ref.py) with poisoned invalid rows; the
untouched query kernels on a masked state (values, row invariance); condition(ctx_len=) / extend of both families against the plain
forward on the sliced context.  Run with -m gpu."""
import functools
import importlib
import os
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import favor_cached_ref as R
from tests import np_query_ref as NR
from tests import ragged_ref as RR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = 3, 2
DM = [(16, 16), (64, 266), (256, 1419)]


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
def _inputs(kind, d, m, Nc, Nq, heads=H):
    """(q, k, v, proj) in the oracle's layout [T, heads, N, d], on the CPU: tests/test_condition_gpu.py's value kinds at T = 3
    ("big": the live regime x 4 at every shape - its fixture holds two tasks)."""
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nc + len(kind))
    q = 0.25 * torch.randn(T, heads, Nq, d, generator=g)
    k = 0.25 * torch.randn(T, heads, Nc, d, generator=g)
    v = torch.randn(T, heads, Nc, d, generator=g)
    if kind == "big":
        q, k = 4 * q, 4 * k
    elif kind == "equal":
        k = k[:1, :1, :1].expand(T, heads, Nc, d).contiguous()
    else:
        assert kind == "live"
    return q, k, v, _proj(d, m)


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _state_floats(state):
    """The state's floats up to and including M, as raw bits (so that the comparison is one of bits)."""
    fk, _ = state.features()
    return state.buf.view(torch.int32)[:fk.numel() + 1]


def _poison(k, proj, lens, how):
    """k with every row behind lens[t] replaced: NaN, +Inf, or a finite key whose dd lies ~50 above every valid key (built like
    test_condition_gpu.py's "peak" key) - unmasked it would set M and drag every valid feature to the floor."""
    T_, H_, Nc, d = k.shape
    m = proj.shape[0]
    valid = RR.valid_mask(lens, Nc)
    out = k.clone()
    if how == "peak":
        dd = torch.einsum("thnd,md->thnm", d ** -0.25 * k.double(), proj.double())
        top = dd[valid[:, None, :].expand(T_, H_, Nc)].max().item()
        p = proj[m // 2]
        row = p * ((top + 50.0) / (d ** -0.25 * float(p @ p)))
        lead = float(d ** -0.25 * (row.double() @ proj.double().T).max())
        assert 45 < lead - top < 55, (lead, top)
    else:
        row = torch.full((d,), float("nan") if how == "nan" else float("inf"))
    out[~valid[:, None, :].expand(T_, H_, Nc)] = row
    return out


# ---- 1. full lengths equal the unmasked entry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("d,m", DM)
def test_full_lengths_equal_the_unmasked_entry(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys, favor_query
    q, k, v, proj = _inputs("live", d, m, Nc, 40)
    qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
    plain, masked = favor_keys(kd, pd), favor_keys(kd, pd, lens=[Nc] * T)
    assert plain.route == masked.route == "cached" and plain.lens is None and masked.lens == (Nc,) * T
    assert masked.buf.numel() == plain.buf.numel() >= gpulib.favor_keys_bytes(T, H, Nc, d, m) > 0
    assert torch.equal(_state_floats(masked), _state_floats(plain))
    assert torch.equal(favor_query(qd, masked, vd, pd), favor_query(qd, plain, vd, pd))


# ---- 2. masked values against float64 ---------------------------------------------------------------------------------------------
RAGGED = [(15, (15, 1, 8)), (17, (16, 17, 1)), (32, (1, 32, 16)), (32, (17, 15, 31))]      # both K1 templates, the 16-row tile edge from both sides
MASKED_CASES = [(d, m, Nc, lens) for d, m in DM[:2] for Nc, lens in RAGGED] + [(256, 1419, Nc, lens) for Nc, lens in RAGGED if Nc == 32]


@pytest.mark.parametrize("kind", ["live", "big", "equal"])
@pytest.mark.parametrize("d,m,Nc,lens", MASKED_CASES, ids=[f"d{d}-m{m}-Nc{Nc}-{'_'.join(map(str, lens))}" for d, m, Nc, lens in MASKED_CASES])
def test_masked_state_against_float64(gpulib, d, m, Nc, lens, kind):
    from mlhot.ops import favor_keys, favor_query
    q, k, v, proj = _inputs(kind, d, m, Nc, 33)
    valid = RR.valid_mask(lens, Nc)
    want, wantM = RR.key_features(k, proj, lens)
    want_out = R.merged(RR.attention_sliced(q, k, v, proj, lens))
    dd = torch.einsum("thnd,md->thnm", d ** -0.25 * k.double(), proj.double())
    dd_scale = dd[valid[:, None, :].expand(T, H, Nc)].abs().max().item()
    mp = (m + 15) // 16 * 16
    vz = torch.where(valid[:, None, :, None], v, torch.full((), 777.0))          # invalid rows of v: finite, anything
    qd, vd, pd = _dev(q), _dev(vz), proj.to(DEV)
    for how in ("nan", "inf", "peak"):
        state = favor_keys(_dev(_poison(k, proj, lens, how)), pd, lens=list(lens))
        fk, M = state.features()
        assert fk.shape == (T, H, Nc, mp) and state.lens == tuple(lens)
        assert bool(torch.isfinite(fk).all()) and bool(torch.isfinite(M).all())
        eF, eM = U.rel_err(fk[..., :m], want), abs(M.item() - wantM.item()) / max(dd_scale, 1e-30)
        print(f"favor_keys lens={lens} {kind} / {how} d={d} m={m} Nc={Nc}: F_k {eF:.2e} of its scale, M {M.item():.4f} off by {eM:.2e} of dd's scale")
        assert eF <= U.RTOL and eM <= U.RTOL
        inv = ~valid.to(DEV)[:, None, :].expand(T, H, Nc)
        assert bool((fk[inv] == 0).all())                                    # every invalid row is exactly zero over all mp
        assert bool((fk[..., m:] == 0).all())                                # features >= m are exactly zero
        assert float(fk[~inv][:, :m].min()) >= m ** -0.5 * 1e-4 * (1 - 1e-6)    # the floor is in on the valid rows
        for Nq in (1, 16, 33):
            got = favor_query(qd[:, :Nq].contiguous(), state, vd, pd)
            err = U.rel_err(got, want_out[:, :Nq])
            print(f"favor_query on it, Nq={Nq}: {err:.2e} of out's scale")
            assert bool(torch.isfinite(got).all()) and err <= U.RTOL


# ---- 3. uniform short lengths equal slicing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,L", [(15, 7), (17, 15), (32, 16), (32, 17)])
@pytest.mark.parametrize("d,m", DM[:2])
def test_uniform_short_lengths_equal_slicing(gpulib, d, m, Nc, L):
    from mlhot.ops import favor_keys
    _, k, _, proj = _inputs("live", d, m, Nc, 1)
    kd, pd = _dev(k), proj.to(DEV)
    fk, M = favor_keys(kd, pd, lens=[L] * T).features()
    fs, Ms = favor_keys(kd[:, :L].contiguous(), pd).features()
    dd_scale = torch.einsum("thnd,md->thnm", d ** -0.25 * k[:, :, :L].double(), proj.double()).abs().max().item()
    eF, eM = U.rel_err(fk[:, :, :L], fs), abs(M.item() - Ms.item()) / dd_scale
    same = torch.equal(fk[:, :, :L], fs) and torch.equal(M, Ms)
    print(f"favor_keys lens=[{L}]*{T} of Nc={Nc} against the sliced keys, d={d} m={m}: F_k {eF:.2e}, M {eM:.2e}; bit-equal: {same} "
          f"(K1 template {'the same' if (Nc <= 16) == (L <= 16) else 'another'})")
    assert eF <= U.RTOL and eM <= U.RTOL
    assert bool((fk[:, :, L:] == 0).all())


# ---- 4. row invariance survives ---------------------------------------------------------------------------------------------------
def _invariance(run, x):
    """run(rows [T, n, ...]) over 100 rows against single rows, 15 / 16 / 17-row slices and a permutation, bit for bit."""
    full = run(x)
    assert full.shape[:2] == (T, 100) and bool(torch.isfinite(full).all())
    for n in (0, 15, 16, 57, 99):
        assert torch.equal(run(x[:, n:n + 1]), full[:, n:n + 1]), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17), (31, 33)):
        assert torch.equal(run(x[:, start:start + L]), full[:, start:start + L]), (start, L)
    perm = torch.randperm(100, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(run(x[:, perm]), full[:, perm])


def test_row_invariance_of_favor_query_on_a_masked_state(gpulib):
    from mlhot.ops import favor_keys, favor_query
    d, m, Nc, lens = 64, 266, 32, (17, 15, 31)
    q, k, v, proj = _inputs("live", d, m, Nc, 100)
    valid = RR.valid_mask(lens, Nc)
    vd, pd = _dev(torch.where(valid[:, None, :, None], v, torch.zeros(()))), proj.to(DEV)
    state = favor_keys(_dev(_poison(k, proj, lens, "nan")), pd, lens=lens)
    _invariance(lambda rows: favor_query(rows.contiguous(), state, vd, pd), _dev(q))


def test_row_invariance_of_np_query_on_a_masked_state(gpulib):
    from mlhot.ops import favor_keys
    d, m, Nc, lens = 16, 16, 32, (17, 15, 31)
    _, k, v, proj = _inputs("live", d, m, Nc, 1, heads=NR.HEADS)
    valid = RR.valid_mask(lens, Nc)
    vd, pd = _dev(torch.where(valid[:, None, :, None], v, torch.zeros(()))), proj.to(DEV)
    state = favor_keys(_dev(_poison(k, proj, lens, "nan")), pd, lens=lens)
    dims = gpulib.np_dims(T, Nc, 1, 3, NR.Y_DIM, d, d, NR.DIM_Z[d], [100, 100], NR.HIDDEN, "attention", False, m)
    assert gpulib.np_query_supported(dims)
    params = {name: t.to(DEV) for name, t in NR.params(d).items()}
    x = torch.randn(T, 100, d, generator=torch.Generator().manual_seed(12)).to(DEV)
    _invariance(lambda rows: gpulib.np_query_fwd(dims, params, rows.contiguous(), key_state=state.buf, vh=vd, proj=pd), x)


# ---- 5. the models ----------------------------------------------------------------------------------------------------------------
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFGDIS = dict(task="distractor", img_size=[128, 128, 1], input_dim=2, output_dim=2, img_agg="max", dim_w=16, seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
             task="shapenet_1d", input_dim=3, output_dim=2)
MODEL_CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention")),
    "cnp_3d_mean": ("CondNeuralProcess", dict(CFG3D, agg_mode="mean")),
    "cnp_3d_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max")),
    "cnp_3d_baco": ("CondNeuralProcess", dict(CFG3D, agg_mode="baco")),
    "anp_distractor": ("ANPDistractor", dict(CFGDIS, agg_mode="attention")),
    "anp_shapenet1d": ("ANPShapeNet1D", dict(CFG1D, agg_mode="attention", dim_r=64)),
    "cnp_shapenet1d_mean": ("CNPShapeNet1D", dict(CFG1D, agg_mode="mean", dim_r=100)),
    "cnp_shapenet1d_max": ("CNPShapeNet1D", dict(CFG1D, agg_mode="max", dim_r=100)),
}
LATENT = [c for c in MODEL_CASES if "cnp" in c]
NQ = 7


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = MODEL_CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


def _images(case, n, seed):
    """(images [T, n, C, H, W], labels [T, n, L]) on the device."""
    cfg = MODEL_CASES[case][1]
    g = torch.Generator().manual_seed(seed)
    Hh, W, Cc = cfg["img_size"]
    Cc = Cc - 1 if cfg["task"] == "shapenet_3d" else Cc
    return torch.rand(T, n, Cc, Hh, W, generator=g).to(DEV), torch.rand(T, n, cfg["input_dim"], generator=g).to(DEV)


def _forward(model, cx, cy, qx):
    with torch.no_grad():
        return model(cx.contiguous(), cy.contiguous(), qx, test=True)[0]


@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_uniform_ctx_len_equals_the_forward_on_the_slice(gpulib, case, L):
    """(a) the spare slots hold other images and labels - and, in the second variant, the same scaled by 1e4 - and change nothing."""
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, L + 3, 3)
    qx = _images(case, NQ, 4)[0]
    want = _forward(model, cx[:, :L], cy[:, :L], qx)
    outs = []
    for scale in (1.0, 1e4):
        px, py = cx.clone(), cy.clone()
        px[:, L:] *= scale
        py[:, L:] *= scale
        state = cached.condition(model, px, py, ctx_len=[L] * T)
        assert state.lens == (L,) * T and state.capacity == state.Nc == L + 3
        got = cached.predict(model, state, qx)
        err = U.rel_err(got, want)
        print(f"predict(condition(ctx_len=[{L}]*{T} of {L + 3} slots, spare x {scale:g})) {case}: {err:.2e} of mu's scale")
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL
        outs.append(got)
    assert torch.equal(outs[0], outs[1])                               # a slot that is no shot is never read


@pytest.mark.parametrize("case", LATENT)
def test_mixed_ctx_len_of_the_latent_models(gpulib, case):
    """(b) task t of the mixed call against the uniform call at L = ctx_len[t]; the aggregate itself bit for bit against
    mlhot_agg_fwd on the slice of the kept rows."""
    from mlhot import cached
    model = _model(case)
    lens = [1, 5, 3]
    cx, cy = _images(case, 5, 5)
    qx = _images(case, NQ, 6)[0]
    state = cached.condition(model, cx, cy, ctx_len=lens)
    got = cached.predict(model, state, qx)
    assert state.kind == "latent" and state.lens == tuple(lens)
    for t, L in enumerate(lens):
        uniform = cached.predict(model, cached.condition(model, cx, cy, ctx_len=[L] * T), qx)
        err = U.rel_err(got[t], uniform[t])
        print(f"mixed ctx_len {lens} {case}, task {t} against the uniform call at L={L}: {err:.2e} of mu's scale")
        assert err <= U.RTOL
        lv = state.lv[:, :L].contiguous() if state.lv is not None else None
        r = gpulib.agg_fwd(model.agg_mode, state.rs[:, :L].contiguous(), lv)[0]
        assert torch.equal(state.r[t], r[t]), (t, L)


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_without_ctx_len_the_call_is_what_it_was(gpulib, case):
    """(c) no masked launch, no prefix aggregate, the same labels on every call and the same bits."""
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 5, 7)
    qx = _images(case, NQ, 8)[0]
    cached.condition(model, cx, cy)                                     # the head stacks are built on the first call
    labels, state = U.launch_labels(gpulib, lambda: cached.condition(model, cx, cy))
    labels2, state2 = U.launch_labels(gpulib, lambda: cached.condition(model, cx, cy))
    masked, _ = U.launch_labels(gpulib, lambda: cached.condition(model, cx, cy, ctx_len=[5] * T))
    print(f"condition {case}: {labels}; with ctx_len: {masked}")
    assert labels == labels2 and not any(l in ("favor.keys1r", "favor.keys2r", "agg_prefix_fwd") for l in labels)
    if state.kind == "attention":
        assert labels[-2:] == ["favor.keys1", "favor.keys2"] and masked[-2:] == ["favor.keys1r", "favor.keys2r"]
        assert state.keys.lens is None
    else:
        assert "agg_fwd" in labels and "agg_prefix_fwd" in masked
    assert state.lens == (5,) * T and state.capacity == 5
    assert torch.equal(cached.predict(model, state, qx), cached.predict(model, state2, qx))
    err = U.rel_err(cached.predict(model, state, qx), _forward(model, cx, cy, qx))
    assert err <= U.RTOL


# ---- 6. extend --------------------------------------------------------------------------------------------------------------------
A, B, CAP = (1, 3, 2), (2, 0, 1), 8


def _concat(first, a, second, b, n):
    """[T, n, ...]: task t's first a[t] slots of `first`, then its first b[t] slots of `second`, then zeros."""
    out = torch.zeros(T, n, *first.shape[2:], device=first.device)
    for t in range(T):
        out[t, :a[t]] = first[t, :a[t]]
        out[t, a[t]:a[t] + b[t]] = second[t, :b[t]]
    return out


@pytest.mark.parametrize("d,m", DM[:2])
def test_extend_at_the_operator_level(gpulib, d, m):
    """The kept rows with the new ones written behind them give the key state of the concatenated slots, bit for bit."""
    from mlhot import ragged
    from mlhot.ops import favor_keys
    _, k, _, proj = _inputs("live", d, m, CAP, 1)
    _, k2, _, _ = _inputs("big", d, m, 2, 1)
    kd, nd, pd = _dev(k), _dev(k2), proj.to(DEV)
    kept = torch.zeros_like(kd)
    src, dst = ragged.slot_indices((0,) * T, A, CAP, CAP, DEV)
    kept = ragged.scatter(kept, dst, ragged.pack(kd, src))
    before = kept.clone()
    src, dst = ragged.slot_indices(A, B, 2, CAP, DEV)
    grown = ragged.scatter(kept, dst, ragged.pack(nd, src))
    assert torch.equal(kept, before)                                    # the old rows stay as they are
    total = tuple(a + b for a, b in zip(A, B))
    direct = _concat(kd, A, nd, B, CAP)
    assert torch.equal(grown, direct)
    s1, s2 = favor_keys(grown, pd, lens=total), favor_keys(direct, pd, lens=total)
    assert torch.equal(_state_floats(s1), _state_floats(s2))
    noisy = direct.clone()
    noisy[~RR.valid_mask(total, CAP).to(DEV)] = float("nan")             # whatever an empty slot holds
    assert torch.equal(_state_floats(favor_keys(noisy, pd, lens=total)), _state_floats(s2))


@pytest.mark.parametrize("case", ["anp_3d", "cnp_3d_baco", "cnp_3d_max", "anp_distractor", "anp_shapenet1d", "cnp_shapenet1d_mean"])
def test_extend_of_the_models(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 3, 9)
    nx, ny = _images(case, 2, 10)
    mx, my = _images(case, 1, 11)
    qx = _images(case, NQ, 12)[0]
    s0 = cached.condition(model, cx, cy, ctx_len=list(A), capacity=CAP)
    assert s0.lens == A and s0.capacity == CAP
    mu0 = cached.predict(model, s0, qx)
    s1 = cached.extend(model, s0, nx, ny, new_len=list(B))
    ab = tuple(a + b for a, b in zip(A, B))
    assert s1 is not s0 and s1.lens == ab and s0.lens == A and s1.capacity == CAP
    want1 = cached.predict(model, cached.condition(model, _concat(cx, A, nx, B, 4), _concat(cy, A, ny, B, 4), ctx_len=list(ab)), qx)
    got1 = cached.predict(model, s1, qx)
    e1 = U.rel_err(got1, want1)
    s2 = cached.extend(model, s1, mx, my)                               # a second one: one more shot for every task
    abc = tuple(n + 1 for n in ab)
    assert s2.lens == abc
    cx2, cy2 = _concat(_concat(cx, A, nx, B, 5), ab, mx, (1,) * T, 5), _concat(_concat(cy, A, ny, B, 5), ab, my, (1,) * T, 5)
    want2 = cached.predict(model, cached.condition(model, cx2, cy2, ctx_len=list(abc)), qx)
    e2 = U.rel_err(cached.predict(model, s2, qx), want2)
    plain = [_forward(model, cx2[t:t + 1, :abc[t]].expand(T, -1, -1, -1, -1), cy2[t:t + 1, :abc[t]].expand(T, -1, -1), qx[t:t + 1].expand(T, -1, -1, -1, -1))[0]
             for t in range(T)] if s0.kind == "latent" else None
    print(f"extend {case}: {A} + {B} against condition on the concatenated slots {e1:.2e}, + one more {e2:.2e} of mu's scale")
    assert e1 <= U.RTOL and e2 <= U.RTOL
    if plain is not None:                                               # a latent task depends on its own shots only: the plain forward per task
        e3 = U.rel_err(cached.predict(model, s2, qx), torch.stack(plain))
        print(f"  and against the plain forward on each task's own {abc} shots: {e3:.2e}")
        assert e3 <= U.RTOL
    assert torch.equal(cached.predict(model, s0, qx), mu0)              # the old state still predicts what it predicted
    assert torch.equal(cached.predict(model, s1, qx), got1)
    big = _images(case, CAP, 13)
    with pytest.raises(ValueError, match="capacity="):
        cached.extend(model, s2, *big)
    assert s2.lens == abc and torch.equal(cached.predict(model, s2, qx), cached.predict(model, s2, qx))
    # a state made without ctx_len has no spare slot; with capacity= it has
    with pytest.raises(ValueError, match="capacity="):
        cached.extend(model, cached.condition(model, cx, cy), mx, my)
    s3 = cached.extend(model, cached.condition(model, cx, cy, capacity=4), mx, my)
    cx3, cy3 = torch.cat([cx, mx], dim=1), torch.cat([cy, my], dim=1)
    e4 = U.rel_err(cached.predict(model, s3, qx), _forward(model, cx3, cy3, qx))
    print(f"  condition(capacity=4) + extend by one against the plain forward on 4 shots: {e4:.2e}")
    assert s3.lens == (4,) * T and e4 <= U.RTOL
