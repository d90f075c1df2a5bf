"""mlhot.cached.evict / retract / slide on the MI355X, both families: an evicted state against a fresh condition on
the kept shots, a window slid over a stream against a fresh condition on its last shots, the read-out and leave-one-out on an
evicted "long" state, a retracted summary against the summary of the remaining shots, and the old states' bits.  Bars: 1e-4 of mu's
scale for evict and slide (the measured difference is printed), tests/test_cached_summary_gpu.py's U.RTOL of mu's scale for retract.
Run with -m gpu."""
import functools
import importlib
import types

import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, NQ, CAP = 3, 5, 8
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
             task="shapenet_1d", input_dim=3, output_dim=2)
CASES = {
    "anp_3d": ("ANP", dict(CFG3D, agg_mode="attention")),
    "cnp_3d_mean": ("CondNeuralProcess", dict(CFG3D, agg_mode="mean")),
    "cnp_3d_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max")),
    "cnp_3d_baco": ("CondNeuralProcess", dict(CFG3D, agg_mode="baco")),
    "anp_shapenet1d": ("ANPShapeNet1D", dict(CFG1D, agg_mode="attention", dim_r=64)),
    "cnp_shapenet1d_mean": ("CNPShapeNet1D", dict(CFG1D, agg_mode="mean", dim_r=100)),
}
ATTENTION = [c for c in CASES if c.startswith("anp")]
LENS, DROP = (8, 5, 2), ([0, 3, 7], [], [0])


@functools.lru_cache(maxsize=None)
def _model(case):
    method, cfg = CASES[case]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _images(case, n, seed):
    cfg = CASES[case][1]
    g = torch.Generator().manual_seed(seed)
    Hh, W, Cc = cfg["img_size"]
    Cc = Cc - 1 if cfg["task"] == "shapenet_3d" else Cc
    return torch.rand(T, n, Cc, Hh, W, generator=g).to(DEV), torch.rand(T, n, cfg["input_dim"], generator=g).to(DEV)


def _kept(cx, cy, lens, drop):
    """The kept shots of every task in front, in their order: (images, labels, ctx_len)."""
    kx, ky, kl = torch.zeros_like(cx), torch.zeros_like(cy), []
    for t, (L, d) in enumerate(zip(lens, drop)):
        keep = [s for s in range(L) if s not in d]
        kx[t, :len(keep)], ky[t, :len(keep)] = cx[t, keep], cy[t, keep]
        kl.append(len(keep))
    return kx, ky, kl


@pytest.mark.parametrize("case", list(CASES))
def test_evict_is_a_fresh_condition_on_the_kept_shots(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, CAP, 3)
    qx = _images(case, NQ, 4)[0]
    state = cached.condition(model, cx, cy, ctx_len=list(LENS), capacity=CAP)
    before = cached.predict(model, state, qx)
    labels, got_state = U.launch_labels(gpulib, lambda: cached.evict(model, state, DROP))
    assert labels.count("rows.compact") == 1 and not any("trunk" in l or "conv" in l for l in labels), labels
    assert got_state.lens == (5, 5, 1) and got_state.capacity == CAP and got_state.kind == state.kind and got_state.form == state.form
    rows = (got_state.kh, got_state.vh) if state.kind == "attention" else (got_state.rs, got_state.lv)
    for x in rows:
        if x is not None:
            assert all(not bool(x[t, L:].any()) for t, L in enumerate(got_state.lens))             # the freed slots are zero rows
    kx, ky, kl = _kept(cx, cy, LENS, DROP)
    want = cached.predict(model, cached.condition(model, kx, ky, ctx_len=kl, capacity=CAP), qx)
    got = cached.predict(model, got_state, qx)
    err = U.rel_err(got, want)
    print(f"predict(evict(condition(capacity={CAP}), {DROP})) {case}: {err:.2e} of mu's scale against a fresh condition on the kept shots")
    assert bool(torch.isfinite(got).all()) and err <= 1e-4
    assert torch.equal(cached.predict(model, state, qx), before)                                  # the old state predicts its old bits
    nx, ny = _images(case, 2, 5)
    grown = cached.extend(model, got_state, nx, ny, new_len=[2, 1, 2])                            # the freed slots take new shots
    assert grown.lens == (7, 6, 3) and bool(torch.isfinite(cached.predict(model, grown, qx)).all())
    if case == "anp_3d":
        assert torch.equal(cached.predict(model, model.evict(state, DROP), qx), got)


@pytest.mark.parametrize("case", list(CASES))
def test_slide_follows_a_stream(gpulib, case):
    from mlhot import cached
    model = _model(case)
    sx, sy = _images(case, 13, 6)
    qx = _images(case, NQ, 7)[0]
    state = cached.condition(model, sx[:, :1].contiguous(), sy[:, :1].contiguous(), capacity=4)
    for s in range(1, 13):
        state = cached.slide(model, state, sx[:, s:s + 1].contiguous(), sy[:, s:s + 1].contiguous())
        assert state.lens == (min(s + 1, 4),) * T and state.capacity == 4
    want = cached.predict(model, cached.condition(model, sx[:, 9:].contiguous(), sy[:, 9:].contiguous(), ctx_len=[4] * T, capacity=4), qx)
    got = cached.predict(model, state, qx)
    err = U.rel_err(got, want)
    print(f"slide over 12 single-shot steps, capacity 4, {case}: {err:.2e} of mu's scale against a fresh condition on the last 4 shots")
    assert bool(torch.isfinite(got).all()) and err <= 1e-4
    with pytest.raises(ValueError, match="capacity is 4"):
        cached.slide(model, state, sx[:, :5].contiguous(), sy[:, :5].contiguous())
    whole = cached.slide(model, state, sx[:, :4].contiguous(), sy[:, :4].contiguous())              # a whole new window
    assert whole.lens == (4,) * T


@pytest.mark.parametrize("case", ATTENTION)
def test_read_out_and_leave_one_out_on_an_evicted_long_state(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 40, 8)
    qx = _images(case, NQ, 9)[0]
    lens, drop = (40, 33, 3), ([0, 31, 32, 39], [5], [1])
    state = cached.evict(model, cached.condition(model, cx, cy, ctx_len=list(lens), form="long"), drop)
    assert state.form == "long" and state.lens == (36, 32, 2)
    mu, att = cached.predict(model, state, qx, return_attention=True)
    assert att.shape[-1] == 40 and all(not bool(att[t, ..., L:].any()) for t, L in enumerate(state.lens))
    assert float((att.sum(dim=-1) - 1).abs().max()) <= 40 * 2 ** -23
    loo = cached.leave_one_out(model, state, qx)
    assert loo.shape[:3] == (T, 40, NQ) and bool(torch.isfinite(loo).all())
    mask = torch.ones(T, NQ, 40, dtype=torch.bool, device=DEV)
    assert torch.equal(cached.predict(model, state, qx, context_mask=mask), mu)


@pytest.mark.parametrize("case", ATTENTION)
def test_retract_is_the_summary_of_the_remaining_shots(gpulib, case):
    from mlhot import cached
    model = _model(case)
    cx, cy = _images(case, 40, 10)
    qx = _images(case, NQ, 11)[0]
    state = cached.condition(model, cx, cy, form="summary")
    before = cached.predict(model, state, qx)
    old_len = [33, 0, 4]
    got_state = cached.retract(model, state, cx[:, :33].contiguous(), cy[:, :33].contiguous(), old_len=old_len)
    assert got_state.form == "summary" and got_state.lens == (7, 40, 36)
    rx, ry = torch.zeros_like(cx), torch.zeros_like(cy)
    for t, L in enumerate(old_len):
        rx[t, :40 - L], ry[t, :40 - L] = cx[t, L:], cy[t, L:]
    want = cached.predict(model, cached.condition(model, rx, ry, ctx_len=[40 - L for L in old_len], form="summary"), qx)
    got = cached.predict(model, got_state, qx)
    err = U.rel_err(got, want)
    print(f"predict(retract(summary of 40, {old_len})) {case}: {err:.2e} of mu's scale against the summary of the remaining shots")
    assert bool(torch.isfinite(got).all()) and err <= U.RTOL
    assert torch.equal(cached.predict(model, state, qx), before)                                  # the old state predicts its old bits
    again = cached.extend(model, got_state, cx[:, :4].contiguous(), cy[:, :4].contiguous(), new_len=[4, 0, 4])
    assert again.lens == (11, 40, 40)
