"""Joining and regrouping per-shot and latent cached contexts without a GPU: mlhot.ragged.gather_rows against a
plain-Python restatement, every refusal of concat / regroup / summarize by its message (host checks, raised before anything is
launched), the launch sequence of the three calls on a recording stand-in for the library, and merge / select refusing what they
always refused, word for word."""
import importlib
import types

import pytest
import torch

from tests import context_join_ref as JR

T = 3
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
             task="shapenet_1d", input_dim=3, output_dim=2)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape")


def _model(method="ANPShapeNet1D", **kw):
    cfg = dict(CFG3D, agg_mode="attention") if method in ("ANP", "CondNeuralProcess") else dict(CFG1D, agg_mode="attention", dim_r=64)
    cfg.update(kw)
    c = types.SimpleNamespace(device=torch.device("cpu"), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval()


def _cnp(mode="mean"):
    return _model("CNPShapeNet1D", agg_mode=mode, dim_r=256 if mode == "baco" else 100)


def _state(model, kind="attention", form="keys", lens=(4, 2, 1), cap=4, tasks=T):
    """A host-only ContextState of `model`: enough for every check that runs before the first launch, and for the recording library."""
    from mlhot.context import ContextState, fingerprint
    if kind == "attention":
        kw = dict(kh=torch.zeros(tasks, cap, 8, 64), vh=torch.zeros(tasks, cap, 8, 64))
    else:
        R = 256 if getattr(model, "agg_mode", "") == "baco" else 100
        kw = dict(rs=torch.zeros(tasks, cap, R), lv=torch.zeros(tasks, cap, R) if getattr(model, "agg_mode", "") == "baco" else None)
    if form == "summary" or kind == "empty":
        kw = {}
    return ContextState(model, tasks, cap, fingerprint(model), kind, lens=lens, form=form, **kw)


# ---- the host plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(JR.PLAN_CASES))
@pytest.mark.parametrize("capacity", [None, 64])
def test_gather_rows_is_its_restatement(case, capacity):
    from mlhot import ragged
    parts = JR.PLAN_CASES[case]
    lens, caps = [s[0] for s in JR.PLAN_STATES], [s[1] for s in JR.PLAN_STATES]
    totals = [sum(lens[i][j] for i, j in task) for task in parts]
    capacity = max(totals) if capacity is None else capacity
    want_rows, want_lens = JR.gather_rows(parts, lens, caps, capacity)
    rows, total = ragged.gather_rows(parts, lens, caps, capacity)
    assert rows == want_rows and total == want_lens == tuple(totals)
    assert all(len(r) == capacity for r in rows)
    for r, n in zip(rows, total):
        assert all(pair == (-1, -1) for pair in r[n:]) and all(ps >= 0 and pr >= 0 for ps, pr in r[:n])       # the fill, and only the fill
    plan = ragged.GatherPlan(parts, lens, caps, capacity, "cpu")
    assert plan.rows.dtype == torch.int32 and tuple(plan.rows.shape) == (3, capacity, 2) and plan.rows.tolist() == [[list(p) for p in r] for r in want_rows]
    assert plan.total == want_lens and plan.lens.tolist() == list(want_lens) and plan.lens.dtype == torch.int32
    assert plan.last.tolist() == [(n - 1) * 3 + t for t, n in enumerate(want_lens)] and plan.last.dtype == torch.int64
    assert plan.rows.data_ptr() % 8 == 0 and plan.lens.untyped_storage().data_ptr() == plan.rows.untyped_storage().data_ptr()     # ONE buffer


def test_gather_rows_by_hand():
    from mlhot import ragged
    rows, total = ragged.gather_rows([[(1, 1), (0, 0)], [(0, 0)]], [(2, 1), (1, 3)], [2, 5], 6)
    assert rows == [[(1, 5), (1, 6), (1, 7), (0, 0), (0, 1), (-1, -1)], [(0, 0), (0, 1)] + [(-1, -1)] * 4] and total == (5, 2)
    # the reference of the kernel tests reads such a table the same way
    a, b = torch.arange(2 * 2 * 4, dtype=torch.float32).view(2, 2, 4), 100 + torch.arange(2 * 5 * 4, dtype=torch.float32).view(2, 5, 4)
    got = JR.gathered([a, b], torch.tensor(rows))
    assert torch.equal(got[0, :3], b[1, :3]) and torch.equal(got[0, 3:5], a[0]) and not bool(got[0, 5].any()) and not bool(got[1, 2:].any())
    assert [len(p) for p in JR.kernel_plans(1, 1, 8, 0)] == [1] * JR.SPECIALS and len(JR.kernel_plans(3, 5, 2, 0)) == 1
    assert JR.kernel_plans(3, 5, 2, 0)[0][0][:5] == [(-1, -1), (2, 0), (1, 66), (0, -5), (1, 65)]


def test_regroup_args_resolve_form_and_capacity():
    from mlhot import ragged
    metas = [((16, 4, 1), 16), ((16, 5, 1), 32)]
    for a, b, form in ((16, 16, "keys"), (17, 16, "long"), (128, 128, "long"), (129, 128, "paged"), (4000, 96, "paged")):
        parts, total, got, cap = ragged.join_args("concat", [((a, 1, 1), a), ((b, 1, 1), b)], 3, True)
        assert (got, cap, total) == (form, a + b, (a + b, 2, 2)) and parts == [[(0, t), (1, t)] for t in range(3)]
    assert ragged.join_args("concat", metas, 3, True, form="paged", capacity=40)[2:] == ("paged", 40)
    assert ragged.join_args("concat", metas, 3, False)[2:] == (None, 32)
    assert ragged.regroup_args("regroup", metas, [(0, 1), [(1, 1)], [(1, 0), (0, 0)]], 3, True)[:2] == ([[(0, 1)], [(1, 1)], [(1, 0), (0, 0)]], (4, 5, 32))
    assert [ragged.smallest_form(n) for n in (1, 32, 33, 256, 257, 4096)] == ["keys", "keys", "long", "long", "paged", "paged"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
class _NoLaunch:
    """Stands in for the library where nothing may be launched: any attribute is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached before the refusal")


@pytest.fixture
def nothing_launches(monkeypatch):
    from mlhot import context, ops
    for mod in (context, ops):
        monkeypatch.setattr(mod, "lib", lambda: _NoLaunch())


def test_concat_refusals(nothing_launches):
    from mlhot import cached
    model, other = _model(), _model()
    a, b = _state(model), _state(model, lens=(1, 1, 3))
    for states, match in (([a, _state(other)], r"concat: the state was not made by this model's condition\(\) \(states\[1\]\)"),
                          ([a, object()], r"concat: .*not made by this model.*states\[1\]"),
                          ([], "concat: needs at least one state"), (a, "concat: states must be a sequence"), (7, "concat: states must be a sequence"),
                          ([a] * 9, r"concat: 9 states; a call takes at most 8 - calls nest"),
                          ([a, _state(model, form="summary")], r"concat: states\[1\] is a summary state.*mlhot.cached.merge.*select.*summarize"),
                          ([_state(model, kind="empty"), a], r"concat: states\[0\] holds no context shot"),
                          ([a, _state(model, tasks=2, lens=(1, 1))], r"concat: states\[1\] holds 2 tasks, states\[0\] 3, the model 3")):
        with pytest.raises(ValueError, match=match):
            cached.concat(model, states)
    latent = _state(_cnp(), kind="latent")
    latent.owner = model                                    # a latent state among attention states (no model makes both)
    with pytest.raises(ValueError, match=r"concat: states\[1\] is a 'latent' state, states\[0\] a 'attention' one - attention and latent states do not mix"):
        cached.concat(model, [a, latent])
    with pytest.raises(ValueError, match=r"concat: task 0 over all states holds 5 context shots in all, the capacity is 4"):
        cached.concat(model, [a, b], capacity=4)
    with pytest.raises(ValueError, match=r'concat: capacity = 33 is outside the keys attention kernels\' envelope \(at most 32 context slots per task\); form="long"'):
        cached.concat(model, [a, b], form="keys", capacity=33)
    with pytest.raises(ValueError, match=r"concat: capacity = 257 is outside the long attention kernels' envelope"):
        cached.concat(model, [a, b], form="long", capacity=257)
    with pytest.raises(ValueError, match=r'concat: capacity = 4097 is above the 4096 slots.*form="summary": mlhot.cached.summarize'):
        cached.concat(model, [a, b], capacity=4097)
    big = _state(model, form="paged", lens=(2100, 1, 1), cap=2100)
    with pytest.raises(ValueError, match=r'concat: capacity = 4200 is above the 4096 slots.*form="summary": mlhot.cached.summarize'):
        cached.concat(model, [big, big])
    with pytest.raises(ValueError, match=r'concat: form must be one of \("keys", "long", "paged"\) or None, got \'summary\'; mlhot.cached.summarize'):
        cached.concat(model, [a, b], form="summary")
    with pytest.raises(ValueError, match="concat: capacity must be an integer"):
        cached.concat(model, [a, b], capacity=8.0)
    rowless = _state(model)
    rowless.kh = None
    with pytest.raises(ValueError, match=r"concat: states\[0\] carries no per-shot rows"):
        cached.concat(model, [rowless])
    odd = _state(model)
    odd.vh = torch.zeros(T, 4, 2, 25)                                                               # rows of 50 floats
    with pytest.raises(ValueError, match=r"concat: states\[1\] keeps per-shot rows of 50 floats; mlhot_rows_gather moves rows whose width is a multiple of 4"):
        cached.concat(model, [a, odd])
    model.train()
    with pytest.raises(ValueError, match=r"concat is a test-mode path: call model.eval\(\) first"):
        cached.concat(model, [a, b])
    model.eval()
    with torch.no_grad():
        next(model.parameters()).add_(0.0)                  # an in-place update: the states are stale
    with pytest.raises(ValueError, match=r"concat: the state is stale .* \(states\[0\]\)"):
        cached.concat(model, [a, b])
    if importlib.util.find_spec("networks.ANPMRShapeNet1D"):
        with pytest.raises(ValueError, match="concat: Bayes-by-backprop"):
            cached.concat(_model("ANPMRShapeNet1D"), [a, b])
    with pytest.raises(ValueError, match="concat: cached-context inference is not built for this class"):
        cached.concat(torch.nn.Linear(2, 2), [a, b])


def test_regroup_refusals(nothing_launches):
    from mlhot import cached
    model = _model()
    a, b = _state(model), _state(model, lens=(1, 1, 3))
    ok = [(0, 0), (1, 0), (0, 2)]
    for picks, match in ((7, "regroup: picks must be a sequence"), ([(0, 0)], "regroup: 1 picks, the model was built for tasks_per_batch = 3"),
                         ([(0, 0), [], (0, 1)], r"regroup: picks\[1\] is empty"),
                         ([(0, 0), 5, (0, 1)], r"regroup: picks\[1\] must be a \(state_index, task_index\) pair or a list of such pairs"),
                         ([(0, 0), [(0, 1, 2)], (0, 1)], r"regroup: picks\[1\] holds \(0, 1, 2\), which is no \(state_index, task_index\) pair"),
                         ([(0, 0), [(0, 1.0)], (0, 1)], r"regroup: picks\[1\] holds \(0, 1.0\), which is no"),
                         ([(0, 0), [(0, 1), (1, 1), (0, 1)], (0, 1)], r"regroup: picks\[1\] names \(0, 1\) twice"),
                         ([(0, 0), (2, 0), (0, 1)], r"regroup: picks\[1\] names \(2, 0\), which is out of range - there are 2 states"),
                         ([(0, 0), (0, 1), (1, 3)], r"regroup: picks\[2\] names \(1, 3\), which is out of range - states\[1\] holds 3 tasks"),
                         ([(0, 0), (0, 1), (-1, 0)], r"regroup: picks\[2\] names \(-1, 0\), which is out of range"),
                         ([[(0, 0), (1, 2)] * 1 + [(0, 1), (0, 2), (1, 0), (1, 1), (0, 0), (1, 2), (0, 1)], (0, 0), (0, 0)],
                          r"regroup: picks\[0\] names 9 parts; a task takes at most 8 per call - calls nest")):
        with pytest.raises(ValueError, match=match):
            cached.regroup(model, [a, b], picks)
    with pytest.raises(ValueError, match=r"regroup: picks\[1\] holds 7 context shots in all, the capacity is 6"):
        cached.regroup(model, [a, b], [(0, 0), [(0, 0), (1, 2)], (0, 2)], capacity=6)
    for states, match in (([a, _state(model, form="summary")], r"regroup: states\[1\] is a summary state"), ([], "regroup: needs at least one state"),
                          ([a] * 9, "regroup: 9 states; a call takes at most 8 - calls nest"), ([_state(_model())], "regroup: .*not made by this model")):
        with pytest.raises(ValueError, match=match):
            cached.regroup(model, states, ok)
    model.train()
    with pytest.raises(ValueError, match="regroup is a test-mode path"):
        cached.regroup(model, [a, b], ok)


def test_latent_and_summarize_refusals(nothing_launches):
    from mlhot import cached
    cnp, anp = _cnp(), _model()
    z = _state(cnp, kind="latent")
    with pytest.raises(ValueError, match=r"concat: form= belongs to the attention models .*got form='long'"):
        cached.concat(cnp, [z, z], form="long")
    with pytest.raises(ValueError, match=r"regroup: form= belongs to the attention models"):
        cached.regroup(cnp, [z], [(0, 0)] * 3, form="keys")
    with pytest.raises(ValueError, match="summarize: the state is a 'latent' state"):
        cached.summarize(cnp, z)
    with pytest.raises(ValueError, match="summarize: the state holds no context shot"):
        cached.summarize(anp, _state(anp, kind="empty"))
    with pytest.raises(ValueError, match="summarize: the state is a summary already"):
        cached.summarize(anp, _state(anp, form="summary"))
    with pytest.raises(ValueError, match="summarize: the state was not made by this model"):
        cached.summarize(anp, _state(_model()))
    anp.train()
    with pytest.raises(ValueError, match="summarize is a test-mode path"):
        cached.summarize(anp, _state(anp))


def test_resnet_family_refuses_alike(nothing_launches):
    from mlhot import cached
    model = _model("ANP")
    a = _state(model)
    with pytest.raises(ValueError, match=r"concat: states\[1\] is a summary state"):
        cached.concat(model, [a, _state(model, form="summary")])
    with pytest.raises(ValueError, match=r"regroup: picks\[0\] names \(0, 1\) twice"):
        cached.regroup(model, [a], [[(0, 1), (0, 1)], (0, 0), (0, 0)])
    model.train()
    for call in (lambda: cached.concat(model, [a]), lambda: cached.summarize(model, a)):
        with pytest.raises(ValueError, match="test-mode"):
            call()


# ---- the launch sequences ------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records the entries the lifecycle reaches, in order.  It has no encoder entry - reaching for one
    is an AttributeError."""

    def __init__(self):
        self.calls, self.seen = [], {}

    def rows_gather(self, sources, plan, T, cap):
        self.calls.append("rows_gather")
        self.seen.update(sources=sources, plan=plan, T=T, cap=cap)
        return [torch.zeros(T, cap, *x.shape[2:]) for x in sources[0]]

    def _keys(self, name, kh, lens):
        self.calls.append(name)
        self.seen.update(kh=kh, lens=lens)
        return torch.zeros(64, dtype=torch.uint8)

    def favor_keys_bytes(self, *a):
        return 64

    favor_long_supported = favor_paged_supported = favor_summary_bytes = favor_keys_bytes

    def favor_keys_ragged_fwd(self, kh, proj, lens):
        return self._keys("favor_keys_ragged_fwd", kh, lens)

    def favor_keys_long_fwd(self, kh, proj, lens):
        return self._keys("favor_keys_long_fwd", kh, lens)

    def favor_keys_paged_fwd(self, kh, proj, lens):
        return self._keys("favor_keys_paged_fwd", kh, lens)

    def agg_prefix_fwd(self, mode, feats, lv):
        self.calls.append("agg_prefix_fwd")
        self.seen.update(mode=mode, lv=lv)
        return torch.zeros(feats.shape[1], feats.shape[0], feats.shape[2]), None

    def linear_fwd(self, x, w, b, act):
        self.calls.append("linear_fwd")
        return torch.zeros(x.shape[0], w.shape[0])

    def favor_summary_init(self, T, H, d, m, device):
        self.calls.append("favor_summary_init")
        return torch.zeros(64, dtype=torch.uint8)

    def favor_summary_absorb(self, kh, vh, proj, buf, lens=None, out=None):
        self.calls.append("favor_summary_absorb")
        self.seen.setdefault("chunks", []).append((kh.shape[1], None if lens is None else lens.tolist()))
        return buf


@pytest.fixture
def rec(monkeypatch):
    from mlhot import cached, context, ops, ragged
    r = _Recorder()
    for mod in (context, ops):
        monkeypatch.setattr(mod, "lib", lambda: r)
    for mod in (cached, ops):
        monkeypatch.setattr(mod, "_need_gpu", lambda *ts: None)
    r.plans = []
    real = ragged.GatherPlan

    def counted(*a, **k):
        r.plans.append(real(*a, **k))
        return r.plans[-1]
    monkeypatch.setattr(ragged, "GatherPlan", counted)
    return r


@pytest.mark.parametrize("a,b,form,entry", [(16, 16, "keys", "favor_keys_ragged_fwd"), (17, 16, "long", "favor_keys_long_fwd"),
                                            (128, 128, "long", "favor_keys_long_fwd"), (129, 128, "paged", "favor_keys_paged_fwd")])
def test_concat_uploads_once_gathers_once_and_runs_the_forms_key_launches(rec, a, b, form, entry):
    from mlhot import cached
    from mlhot.context import fingerprint
    model = _model()
    sa = _state(model, form="keys" if a <= 32 else "long", lens=(a, 2, 1), cap=a)
    sb = _state(model, form="paged", lens=(b, 1, 3), cap=b + 4)                       # the forms mix freely
    sa.wq = ("wq of a",)
    got = cached.concat(model, [sa, sb])
    assert rec.calls == ["rows_gather", entry] and len(rec.plans) == 1                # no encoder entry exists on the recorder
    plan = rec.plans[0]
    assert rec.seen["plan"] is plan.rows and (rec.seen["T"], rec.seen["cap"]) == (T, a + b) and [len(s) for s in rec.seen["sources"]] == [2, 2]
    assert rec.seen["sources"][0][0] is sa.kh and rec.seen["sources"][1][1] is sb.vh
    assert rec.seen["lens"].untyped_storage().data_ptr() == plan.rows.untyped_storage().data_ptr()         # the ONE upload serves the key launch too
    assert plan.rows[0, a].tolist() == [1, 0] and plan.rows[1, 2].tolist() == [1, b + 4] and plan.rows[1, 3].tolist() == [-1, -1]
    assert got.form == form and got.capacity == got.Nc == a + b and got.lens == (a + b, 3, 4) and got.kind == "attention"
    assert got.owner is model and got.fingerprint == fingerprint(model) and got.wq is sa.wq and got.kh.data_ptr() == rec.seen["kh"].data_ptr()
    assert tuple(got.kh.shape) == (T, a + b, 8, 64) and got.vh.shape == got.kh.shape and got.keys.route == {"keys": "cached"}.get(form, form)
    assert sa.lens == (a, 2, 1) and sb.lens == (b, 1, 3)
    spare = cached.concat(model, [sa, sb], form="paged", capacity=300)
    assert spare.form == "paged" and spare.capacity == 300 and rec.calls[-2:] == ["rows_gather", "favor_keys_paged_fwd"]


def test_regroup_takes_concats_launches_and_concat_is_a_regroup(rec):
    from mlhot import cached
    model = _model()
    sa, sb = _state(model, lens=(4, 2, 1)), _state(model, form="long", lens=(40, 1, 3), cap=40)
    got = cached.regroup(model, [sa, sb], [(1, 2), [(0, 0), (1, 1)], [(0, 1), (0, 0)]])
    assert rec.calls == ["rows_gather", "favor_keys_ragged_fwd"] and got.lens == (3, 5, 6) and got.capacity == 6 and got.form == "keys"
    assert rec.plans[0].rows[:, :3].tolist() == [[[1, 80], [1, 81], [1, 82]], [[0, 0], [0, 1], [0, 2]], [[0, 4], [0, 5], [0, 0]]]
    joined = cached.concat(model, [sa, sb])
    again = cached.regroup(model, [sa, sb], [[(0, t), (1, t)] for t in range(T)])
    assert torch.equal(rec.plans[1].rows, rec.plans[2].rows) and joined.lens == again.lens == (44, 3, 4) and joined.form == again.form == "long"


@pytest.mark.parametrize("mode", ["mean", "max", "baco"])
def test_latent_concat_runs_the_prefix_aggregate_and_the_linear(rec, mode):
    from mlhot import cached
    model = _cnp(mode)
    sa, sb = _state(model, kind="latent", lens=(4, 2, 1)), _state(model, kind="latent", lens=(1, 7, 3), cap=8)
    got = cached.concat(model, [sa, sb])
    assert rec.calls == ["rows_gather", "agg_prefix_fwd", "linear_fwd"] and len(rec.plans) == 1
    assert [len(s) for s in rec.seen["sources"]] == [2 if mode == "baco" else 1] * 2 and rec.seen["mode"] == mode
    assert (rec.seen["lv"] is not None) == (mode == "baco")
    assert got.kind == "latent" and got.lens == (5, 9, 4) and got.capacity == 9 and tuple(got.rs.shape) == (T, 9, 256 if mode == "baco" else 100)
    assert tuple(got.z.shape) == (T, 64) and (got.lv is not None) == (mode == "baco")
    picked = cached.regroup(model, [sa, sb], [(1, 1), (0, 0), [(0, 2), (1, 2)]], capacity=12)
    assert picked.lens == (7, 4, 4) and picked.capacity == 12 and rec.calls[3:] == ["rows_gather", "agg_prefix_fwd", "linear_fwd"]


def test_summarize_absorbs_the_packed_rows_in_chunks_of_32(rec):
    from mlhot import cached
    model = _model()
    st = _state(model, form="long", lens=(40, 33, 3), cap=48)
    st.kh = torch.randn(T, 48, 8, 64)
    st.wq = ("wq",)
    got = cached.summarize(model, st)
    assert rec.calls == ["favor_summary_init", "favor_summary_absorb", "favor_summary_absorb"]       # 48 slots: two chunks, nothing else
    assert rec.seen["chunks"] == [(32, [32, 32, 3]), (16, [8, 1, 0])]
    assert got.form == "summary" and got.kind == "attention" and got.lens == (40, 33, 3) and got.Nc == 40 and got.capacity is None
    assert got.kh is None and got.vh is None and got.wq is st.wq and got.keys.route == "summary" and st.form == "long"


# ---- merge and select are untouched --------------------------------------------------------------------------------------------------
def test_merge_and_select_refuse_what_they_always_refused(nothing_launches):
    from mlhot import cached
    model = _model()
    picks = [(0, 0)] * T
    for form, slots in (("keys", 32), ("long", 256), ("paged", 4096)):
        st = _state(model, form=form)
        want = (rf"{{}}: states\[0\] has form '{form}' - it holds per-shot rows in at most {slots} slots, not sums over shots; "
                r'condition the parts with form="summary"')
        with pytest.raises(ValueError, match=want.format("merge")):
            cached.merge(model, [st])
        with pytest.raises(ValueError, match=want.format("select")):
            cached.select(model, [st], picks)
    cnp = _cnp()
    z = _state(cnp, kind="latent")
    want = (r"{}: states\[0\] is a 'latent' state - it is stored behind its finishing Linear, which is not a sum over shots any more; "
            r'only attention states of form="summary" {}')
    with pytest.raises(ValueError, match=want.format("merge", "merge")):
        cached.merge(cnp, [z])
    with pytest.raises(ValueError, match=want.format("select", "select")):
        cached.select(cnp, [z], picks)
