"""mlhot.cached.concat / regroup / summarize on the MI355X, both families: paged states joined against a fresh
condition on all their shots, to the bit; the other forms, promoted where the total outgrows them, against a fresh condition and the
model's own forward to U.RTOL of mu's scale, with everything predict offers on the result's form; the key stabiliser; regrouped
batches; latent states per agg_mode; and the bridge to summary states.  Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, NQ = 2, 7
V1D = dict(seed=2578, img_size=[128, 128, 1], input_dim=3, output_dim=2, img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d")
CASES = {
    "vanilla_anp": ("ANPShapeNet1D", dict(V1D, agg_mode="attention", dim_r=64), (1, 128, 128), 3),
    "resnet_anp": ("ANP", dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
                               agg_mode="attention"), (3, 64, 64), 4),
    "cnp_mean": ("CNPShapeNet1D", dict(V1D, agg_mode="mean", dim_r=100), (1, 128, 128), 3),
    "cnp_max": ("CNPShapeNet1D", dict(V1D, agg_mode="max", dim_r=100), (1, 128, 128), 3),
    "cnp_baco": ("CNPShapeNet1D", dict(V1D, agg_mode="baco", dim_r=256), (1, 128, 128), 3),
}
ATTENTION = ["vanilla_anp", "resnet_anp"]
LATENT = ["cnp_mean", "cnp_max", "cnp_baco"]


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg, _, _ = CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _batch(case, n=300):
    """(ctx images [T, n, ...], ctx labels, target images [T, NQ, ...]) on the device; left unchanged by every test."""
    _, _, img, L = CASES[case]
    g = torch.Generator().manual_seed(13)
    return tuple(t.to(DEV) for t in (torch.rand(T, n, *img, generator=g), torch.rand(T, n, L, generator=g), torch.rand(T, NQ, *img, generator=g)))


def _cut(cx, cy, a, b):
    return cx[:, a:b].contiguous(), cy[:, a:b].contiguous()


def _plain(model, state, qx, **kw):
    from mlhot import cached
    from networks._resnet_np import ResNetNP
    return cached.predict(model, state, qx, **kw) if isinstance(model, ResNetNP) else cached.predict(model, state, qx, route="composed", **kw)


def _same_state(got, want):
    assert got.form == want.form and got.lens == want.lens and got.capacity == want.capacity and got.kind == want.kind
    assert torch.equal(got.kh, want.kh) and torch.equal(got.vh, want.vh)
    for a, b in zip(got.keys.features(), want.keys.features()):                                     # F_k and M
        assert torch.equal(a, b)


# ---- paged against a fresh condition, to the bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ATTENTION)
def test_paged_states_joined_are_the_state_conditioned_on_all_shots(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    parts = [cached.condition(model, *_cut(cx, cy, a, b), form="paged") for a, b in ((0, 200), (200, 260), (260, 300))]
    labels, got = U.launch_labels(gpulib, lambda: cached.concat(model, parts))
    assert labels.count("rows.gather") == 1 and not any("trunk" in l or "conv" in l or "enc." in l for l in labels), labels
    want = cached.condition(model, cx, cy, form="paged", capacity=300)
    assert got.form == "paged" and got.lens == (300, 300) and [p.lens for p in parts] == [(200, 200), (60, 60), (40, 40)]
    _same_state(got, want)
    assert torch.equal(cached.predict(model, got, qx), cached.predict(model, want, qx))
    # per-task context sizes: the shots of every task close up behind one another.  A task gets as little from states[1] as a state
    # can hold: condition takes ctx_len in 1 .. Nslots, so no state has a task without a shot (a part of none exists for the host
    # plan alone: tests/test_context_join_cpu.py)
    with pytest.raises(ValueError, match=r"ctx_len must lie in 1\.\.60"):
        cached.condition(model, *_cut(cx, cy, 200, 260), ctx_len=[60, 0], form="paged")
    a = cached.condition(model, *_cut(cx, cy, 0, 200), ctx_len=[200, 150], form="paged")
    b = cached.condition(model, *_cut(cx, cy, 200, 260), ctx_len=[60, 1], form="paged")
    got = cached.concat(model, [a, b])
    fx, fy = cx[:, :260].clone(), cy[:, :260].clone()
    fx[1, 150], fy[1, 150] = cx[1, 200], cy[1, 200]
    want = cached.condition(model, fx, fy, ctx_len=[260, 151], form="paged", capacity=260)
    assert got.lens == (260, 151) and got.capacity == 260
    _same_state(got, want)
    assert torch.equal(cached.predict(model, got, qx), cached.predict(model, want, qx))
    assert not bool(got.kh[1, 151:].any()) and not bool(got.vh[1, 151:].any())                       # the fill is zero rows


# ---- the other forms against a fresh condition, to U.RTOL ----------------------------------------------------------------------------
@pytest.mark.parametrize("src,na,nb,form", [("keys", 5, 7, "keys"), ("keys", 20, 20, "long"), ("long", 100, 100, "paged")])
@pytest.mark.parametrize("case", ATTENTION)
def test_joined_states_of_the_other_forms(gpulib, case, src, na, nb, form):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    n = na + nb
    a, b = (cached.condition(model, *_cut(cx, cy, lo, hi), form=src) for lo, hi in ((0, na), (na, n)))
    got = cached.concat(model, [a, b], form=None if n > {"long": 32, "paged": 256}.get(form, 0) else form)     # promoted by the total, or on request
    assert got.form == form and got.lens == (n, n) and got.capacity == n and got.keys.route == {"keys": "cached"}.get(form, form)
    mu = _plain(model, got, qx)
    fresh = _plain(model, cached.condition(model, *_cut(cx, cy, 0, n), form=form), qx)
    with torch.no_grad():
        fwd = model(*_cut(cx, cy, 0, n), qx, test=True)[0]
    e1, e2 = U.rel_err(mu, fresh), U.rel_err(mu, fwd)
    print(f"concat {case} {src} {na} + {nb} -> {form}: {e1:.2e} of mu's scale against a fresh condition, {e2:.2e} against forward(test=True)")
    assert bool(torch.isfinite(mu).all()) and e1 <= U.RTOL and e2 <= U.RTOL
    # everything predict offers on the result's form
    mu2, att = cached.predict(model, got, qx, return_attention=True)
    assert torch.equal(mu2, mu) and att.shape == (T, 8, NQ, n) and float((att.sum(dim=-1) - 1).abs().max()) <= n * 2 ** -23
    mask = torch.ones(T, NQ, n, dtype=torch.bool, device=DEV)
    assert torch.equal(cached.predict(model, got, qx, context_mask=mask), mu)
    mask[:, :, na:] = False                                                                         # states[1]'s shots masked: states[0]'s columns alone
    half, hatt = cached.predict(model, got, qx, context_mask=mask, return_attention=True)
    assert bool(torch.isfinite(half).all()) and not bool(hatt[..., na:].any())
    loo = cached.leave_one_out(model, got, qx)
    assert loo.shape[:3] == (T, n, NQ) and bool(torch.isfinite(loo).all())
    # extend and evict serve the result like any state of its form
    room = cached.concat(model, [a, b], capacity=n + 2, form=form if n + 2 <= {"keys": 32, "long": 256}.get(form, 4096) else None)
    grown = cached.extend(model, room, *_cut(cx, cy, n, n + 2))
    assert grown.lens == (n + 2, n + 2) and grown.form == room.form
    e3 = U.rel_err(_plain(model, grown, qx), _plain(model, cached.condition(model, *_cut(cx, cy, 0, n + 2), form=room.form), qx))
    assert e3 <= U.RTOL
    with pytest.raises(ValueError, match=f"would hold {n + 3} context shots, the state's capacity is {n + 2}"):
        cached.extend(model, grown, *_cut(cx, cy, 0, 1))
    less = cached.evict(model, got, [list(range(na)), [0]])                                        # task 0 keeps states[1]'s shots alone
    assert less.lens == (nb, n - 1) and less.form == form
    kx, ky = cx[:, :n - 1].clone(), cy[:, :n - 1].clone()
    kx[0, :nb], ky[0, :nb] = cx[0, na:n], cy[0, na:n]
    kx[1], ky[1] = cx[1, 1:n], cy[1, 1:n]
    kept = cached.condition(model, kx, ky, ctx_len=[nb, n - 1], capacity=n, form=form)
    assert U.rel_err(_plain(model, less, qx), _plain(model, kept, qx)) <= U.RTOL


# ---- the key stabiliser --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ATTENTION)
def test_the_stabiliser_is_the_maximum_over_all_shots_of_the_result(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    bx, by = _cut(cx, cy, 3, 7)
    bx[1, 2] *= 40.0                                                                                # one shot of states[1] far above the rest
    a = cached.condition(model, *_cut(cx, cy, 0, 3), form="paged")
    b = cached.condition(model, bx, by, form="paged")
    Ma, Mb = a.keys.features()[1].item(), b.keys.features()[1].item()
    print(f"stabiliser {case}: M of states[0] {Ma:.3f}, of states[1] {Mb:.3f}")
    assert Mb > Ma, (Ma, Mb)                                                                        # the shot holds the maximum
    got = cached.concat(model, [a, b], form="paged")
    want = cached.condition(model, torch.cat([cx[:, :3], bx], dim=1), torch.cat([cy[:, :3], by], dim=1), form="paged")
    assert got.keys.features()[1].item() == Mb == want.keys.features()[1].item()
    _same_state(got, want)
    assert cached.concat(model, [a, a], form="paged").keys.features()[1].item() == Ma                              # without it the stabiliser is the rest's


# ---- regroup -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ATTENTION)
def test_regrouped_batches(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case)
    a = cached.condition(model, *_cut(cx, cy, 0, 9), ctx_len=[9, 6], form="paged")
    b = cached.condition(model, *_cut(cx, cy, 9, 14), ctx_len=[4, 5], form="paged")
    got = cached.regroup(model, [a, b], [(0, 1), (1, 0)], form="paged")                                           # the batch (a task 1, b task 0)
    fx, fy = torch.zeros_like(cx[:, :6]), torch.zeros_like(cy[:, :6])
    fx[0], fy[0] = cx[1, :6], cy[1, :6]
    fx[1, :4], fy[1, :4] = cx[0, 9:13], cy[0, 9:13]
    want = cached.condition(model, fx, fy, ctx_len=[6, 4], form="paged")
    assert got.lens == (6, 4) and got.capacity == 6
    _same_state(got, want)
    assert torch.equal(cached.predict(model, got, qx), cached.predict(model, want, qx))
    keys = cached.regroup(model, [a, b], [(0, 1), (1, 0)], form="keys")                             # the same rows behind the 32-slot kernels
    assert keys.form == "keys" and U.rel_err(_plain(model, keys, qx), cached.predict(model, want, qx)) <= U.RTOL
    twice = cached.regroup(model, [a, b], [(0, 0), (0, 0)])                                         # one object in both slots
    assert twice.lens == (9, 9) and torch.equal(twice.kh[0], a.kh[0]) and torch.equal(twice.kh[1], a.kh[0]) and torch.equal(twice.vh[1], a.vh[0])
    same_q = qx[:1].expand(T, -1, -1, -1, -1).contiguous()
    mu = cached.predict(model, twice, same_q)
    assert torch.equal(mu[0], mu[1]) and bool(torch.isfinite(mu).all())
    joined, parts = cached.concat(model, [a, b], form="paged"), cached.regroup(model, [a, b], [[(0, 0), (1, 0)], [(0, 1), (1, 1)]], form="paged")
    assert joined.lens == (13, 11)
    _same_state(parts, joined)                                                                      # a task from two parts is concat's task
    assert torch.equal(cached.predict(model, parts, qx), cached.predict(model, joined, qx))
    assert a.lens == (9, 6) and b.lens == (4, 5)


# ---- latent --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LATENT)
def test_latent_states_joined_predict_as_the_state_conditioned_on_all_shots(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy, qx = _batch(case, 16)
    a, b = cached.condition(model, *_cut(cx, cy, 0, 5)), cached.condition(model, *_cut(cx, cy, 5, 12))
    labels, got = U.launch_labels(gpulib, lambda: cached.concat(model, [a, b]))
    assert labels.count("rows.gather") == 1 and not any("conv" in l or "enc." in l for l in labels), labels
    assert got.kind == "latent" and got.lens == (12, 12) and got.capacity == 12 and (got.lv is not None) == (case == "cnp_baco")
    want = cached.condition(model, *_cut(cx, cy, 0, 12))
    mu, ref = cached.predict(model, got, qx), cached.predict(model, want, qx)
    err = U.rel_err(mu, ref)
    print(f"concat {case} 5 + 7: {err:.2e} of mu's scale against condition on the 12, bit-equal: {torch.equal(mu, ref)}")
    assert bool(torch.isfinite(mu).all()) and err <= U.RTOL
    if case == "cnp_max":
        assert torch.equal(mu, ref)
    picked = cached.regroup(model, [a, b], [(1, 1), [(0, 0), (1, 0)]], capacity=14)
    assert picked.lens == (7, 12) and picked.capacity == 14
    fx, fy = cx[:, :12].clone(), cy[:, :12].clone()
    fx[0, :7], fy[0, :7] = cx[1, 5:12], cy[1, 5:12]
    fx[1], fy[1] = cx[0, :12], cy[0, :12]
    ref2 = cached.predict(model, cached.condition(model, fx, fy, ctx_len=[7, 12], capacity=14), qx)
    assert U.rel_err(cached.predict(model, picked, qx), ref2) <= U.RTOL
    grown = cached.extend(model, picked, *_cut(cx, cy, 12, 14))
    assert grown.lens == (9, 14)


# ---- summarize -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,n", [("keys", 12), ("long", 40), ("paged", 280)])
@pytest.mark.parametrize("case", ATTENTION)
def test_summarize_bridges_to_the_summary_states(gpulib, case, form, n):
    from mlhot import cached
    from mlhot.ops import favor_absorb
    model = _model(case)
    cx, cy, qx = _batch(case)
    lens = [n, max(n // 2 + 1, 1)]
    state = cached.condition(model, *_cut(cx, cy, 0, n), ctx_len=lens, form=form)
    labels, got = U.launch_labels(gpulib, lambda: cached.summarize(model, state))
    assert not any("trunk" in l or "conv" in l or "enc." in l for l in labels), labels
    assert got.form == "summary" and got.lens == tuple(lens) and got.Nc == n and got.kh is None and state.form == form
    direct = favor_absorb(None, state.kh, state.vh, model.attn.projection_matrix, lens=lens)
    for x, y in zip(got.keys.summary(), direct.summary()):
        assert torch.equal(x, y)
    err = U.rel_err(_plain(model, got, qx), _plain(model, state, qx))
    print(f"summarize {case} {form} {lens}: {err:.2e} of mu's scale against predict on the per-shot state")
    assert err <= U.RTOL
    other = cached.condition(model, *_cut(cx, cy, n, n + 8), form="summary")
    merged = cached.merge(model, [got, other])
    assert merged.lens == (n + 8, lens[1] + 8)
    fx, fy = cx[:, :n + 8].clone(), cy[:, :n + 8].clone()
    fx[1, lens[1]:lens[1] + 8], fy[1, lens[1]:lens[1] + 8] = cx[1, n:n + 8], cy[1, n:n + 8]
    whole = cached.condition(model, fx, fy, ctx_len=[n + 8, lens[1] + 8], form="summary")
    assert U.rel_err(_plain(model, merged, qx), _plain(model, whole, qx)) <= U.RTOL
    picked = cached.select(model, [got, other], [(0, 1), [(1, 0), (0, 0)]])
    assert picked.lens == (lens[1], n + 8) and bool(torch.isfinite(_plain(model, picked, qx)).all())
