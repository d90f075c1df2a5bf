"""Sliding-window cached contexts without a GPU: every refusal of evict / retract / slide (host checks, raised
before anything touches a device), the plan arithmetic, the float64 retracting stream against the float64 absorb of the remaining
shots, and the amplification kappa of every retract case the GPU tests use - the check that keeps their bounds meaningful."""
import importlib
import types

import pytest
import torch

from tests import context_window_cases as WC
from tests import context_window_ref as WR

T = 3
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
             task="shapenet_1d", input_dim=3, output_dim=2)


def _model(method="ANPShapeNet1D", **kw):
    cfg = dict(CFG1D, agg_mode="attention", dim_r=64)
    cfg.update(kw)
    c = types.SimpleNamespace(device=torch.device("cpu"), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval()


def _state(model, kind="attention", form="keys", lens=(4, 2, 1), cap=4):
    """A host-only ContextState of `model`: enough for every check that runs before the first launch."""
    from mlhot.context import ContextState, fingerprint
    rows = torch.zeros(T, cap, 8, 64) if kind == "attention" else torch.zeros(T, cap, 64)
    kw = dict(kh=rows, vh=rows) if kind == "attention" else dict(rs=rows)
    if form == "summary":
        kw = {}
    return ContextState(model, T, cap, fingerprint(model), kind, lens=lens, form=form, **kw)


def test_evict_refusals():
    from mlhot import cached
    model, other = _model(), _model()
    st = _state(model)
    ok = [[0], [], []]
    for bad, match in ((_state(other), "not made by this model"), (object(), "not made by this model"),
                       (_state(model, form="summary"), "summary state keeps no per-shot rows"), (_state(model, kind="empty"), "no context shot")):
        with pytest.raises(ValueError, match=match):
            cached.evict(model, bad, ok)
    for drop, match in (([[0], []], "2 entries"), ([[4], [], []], "outside 0..3"), ([[], [2], []], "outside 0..1"), ([[-1], [], []], "outside"),
                        ([[1, 1], [], []], "twice"), ([[], [], [0]], "without a context shot"), ([[0, 1, 2, 3], [], []], "without a context shot"),
                        ([[0.0], [], []], "integers"), ([[True], [], []], "integers"), (3, "sequence"), ([1, 2, 3], "sequence"),
                        (torch.zeros(3, 1, dtype=torch.int64), "host sequence")):
        with pytest.raises(ValueError, match=match):
            cached.evict(model, st, drop)
    model.train()
    with pytest.raises(ValueError, match="test-mode"):
        cached.evict(model, st, ok)
    model.eval()
    with torch.no_grad():
        next(model.parameters()).add_(0.0)              # an in-place update: the state is stale
    with pytest.raises(ValueError, match="stale"):
        cached.evict(model, st, ok)
    bbb = _model("ANPMRShapeNet1D") if importlib.util.find_spec("networks.ANPMRShapeNet1D") else None
    if bbb is not None:
        with pytest.raises(ValueError, match="Bayes-by-backprop"):
            cached.evict(bbb, st, ok)
    with pytest.raises(ValueError, match="not built for this class"):
        cached.evict(torch.nn.Linear(2, 2), st, ok)


def test_resnet_evict_is_the_method_and_refuses_alike():
    from mlhot import cached
    cfg = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", agg_mode="attention")
    c = types.SimpleNamespace(device=torch.device("cpu"), tasks_per_batch=T, **cfg)
    model = importlib.import_module("networks.ANP").ANP(c).eval()
    st = _state(model)
    for call in (lambda d: cached.evict(model, st, d), lambda d: model.evict(st, d)):
        with pytest.raises(ValueError, match="twice"):
            call([[0, 0], [], []])
        with pytest.raises(ValueError, match="without a context shot"):
            call([[], [], [0]])
    model.train()
    with pytest.raises(ValueError, match="test-mode"):
        model.evict(st, [[0], [], []])


def test_retract_and_slide_refusals():
    from mlhot import cached
    model = _model()
    x, y = torch.zeros(T, 2, 1, 128, 128), torch.zeros(T, 2, 3)
    summ = _state(model, form="summary", lens=(5, 2, 1))
    with pytest.raises(ValueError, match="no summary"):
        cached.retract(model, _state(model), x, y)
    with pytest.raises(ValueError, match="task 1 holds 2 context shots and would give up 2"):
        cached.retract(model, summ, x, y)
    with pytest.raises(ValueError, match="task 2 holds 1 context shots and would give up 1"):
        cached.retract(model, summ, x, y, old_len=[2, 1, 1])
    with pytest.raises(ValueError, match="old_len|new_len"):
        cached.retract(model, summ, x, y, old_len=[3, 0, 0])
    with pytest.raises(ValueError, match="holds 3 tasks"):
        cached.retract(model, summ, x[:2], y[:2])
    with pytest.raises(ValueError, match="no new context slot"):
        cached.retract(model, summ, x[:, :0], y[:, :0])
    with pytest.raises(ValueError, match="summary"):
        cached.slide(model, summ, x, y)
    with pytest.raises(ValueError, match="no context shot"):
        cached.slide(model, _state(model, kind="empty"), x, y)
    small = _state(model, lens=(1, 1, 1), cap=1)
    with pytest.raises(ValueError, match="takes 2 new context shots, the state's capacity is 1"):
        cached.slide(model, small, x, y)
    model.train()
    for call in (lambda: cached.retract(model, summ, x, y, old_len=[1, 0, 0]), lambda: cached.slide(model, _state(model), x, y)):
        with pytest.raises(ValueError, match="test-mode"):
            call()


def test_plan_arithmetic():
    from mlhot import ragged
    rows, total = ragged.keep_rows((5, 3, 1), [(0, 3), (), ()], 6)
    assert rows == [[1, 2, 4, -1, -1, -1], [0, 1, 2, -1, -1, -1], [0, -1, -1, -1, -1, -1]] and total == (3, 3, 1)
    st = types.SimpleNamespace(lens=(5, 3, 1), capacity=6, kind="latent")
    assert ragged.evict_args("evict", st, [[3, 0], [], ()]) == [(0, 3), (), ()]                 # sorted: the kept shots keep their order
    add, drop = ragged.slide_args("slide", st, 3, 4, [4, 3, 0])
    assert add == (4, 3, 0) and drop == [(0, 1, 2), (), ()]                                      # only what the spare slots do not take
    assert ragged.slide_args("slide", st, 3, 6, [6, 0, 1])[1] == [(0, 1, 2, 3, 4), (), ()]       # a whole new window
    plan = ragged.KeepPlan((5, 3, 1), [(0, 3), (), ()], 6, "cpu")
    assert plan.rows.dtype == torch.int32 and plan.rows.tolist() == rows and plan.lens.tolist() == [3, 3, 1] and plan.total == (3, 3, 1)
    assert plan.last.tolist() == [2 * 3 + 0, 2 * 3 + 1, 0 * 3 + 2]
    src = torch.arange(3 * 6 * 2, dtype=torch.float32).view(3, 6, 2)
    src[0, 3] = float("nan")
    got = WR.compact(src, rows)
    assert torch.equal(got[0, :3], src[0, [1, 2, 4]]) and not bool(got[:, 3:].any()) and bool(torch.isfinite(got).all())


def test_row_plans_of_the_gpu_cases():
    for cap, _ in WC.ROW_SHAPES:
        for kind in WC.PLANS:
            rows = WC.row_plan(kind, 2, cap)
            assert len(rows) == 2 and all(len(r) == cap for r in rows)
            kept = [p for p in rows[0] if 0 <= p < cap]
            assert kept == sorted(kept)
    assert 255 not in WC.row_plan("drop_255_256", 1, 257)[0] and 256 not in WC.row_plan("drop_255_256", 1, 257)[0]
    for _, cap in WC.EVICT_FORMS:
        lens, drop = WC.evict_lens(cap), WC.evict_drop(cap)
        assert lens[0] == cap and lens[2] - len(drop[2]) == 1 and WC.PEAK[1] in drop[WC.PEAK[0]]
        assert all(len(set(d)) == len(d) and max(d) < L for d, L in zip(drop, lens))


@pytest.mark.parametrize("regime", WC.REGIMES)
@pytest.mark.parametrize("N,R,which", WC.RETRACTS)
@pytest.mark.parametrize("d,m", WC.SHAPES)
def test_float64_retract_is_the_absorb_of_the_rest_and_kappa_is_small(d, m, N, R, which, regime):
    q, k, v, proj = WC.retract_inputs(regime, d, m, N)
    lens, old, rest = WC.retract_split(N, R, which)
    full = WR.absorbed(k, v, proj, [N] * WC.RETRACT_T)
    before_a = full.a.clone()
    n = max(lens)
    st = WR.absorbed(k, v, proj, [N] * WC.RETRACT_T)
    for s in range(0, n, 32):
        e = min(s + 32, n)
        st.retract(WC.gathered(k, old, n)[:, :, s:e], WC.gathered(v, old, n)[:, :, s:e], proj, [min(max(L - s, 0), e - s) for L in lens])
    nr = max(len(r) for r in rest)
    want = WR.absorbed(WC.gathered(k, rest, nr), WC.gathered(v, rest, nr), proj, [len(r) for r in rest], M=full.M)
    assert want.M == full.M == st.M and st.cnt == want.cnt == [N - L for L in lens]
    for name in ("A", "a", "vs"):
        scale = getattr(full, name).abs().max().item()
        err = (getattr(st, name) - getattr(want, name)).abs().max().item() / scale
        assert err <= 1e-12, (name, err)
    kap = (before_a / st.a).max().item()
    print(f"retract {regime} d={d} m={m} {N}-{R} {which}: kappa {kap:.3f}")
    assert kap == pytest.approx(WR.kappa(full, want, m), rel=1e-9) and kap <= 4.0
    assert bool(torch.isfinite(st.query(q, proj)).all())
