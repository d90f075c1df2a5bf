"""Merging FAVOR+ summary states without a GPU: the float64 merge of tests/favor_merge_ref.py against the float64
stream over the whole case - the contract of the feature -, the host build's entry, every refusal of mlhot.ops.favor_merge and
mlhot.cached.merge that is decided on the host, and the group-of-8 fold order on a recording stub of the binding call."""
import ctypes as C
import importlib
import math
import types

import pytest
import torch

from tests import favor_merge_ref as MR
from tests import favor_summary_ref as S

CFGV = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
            n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
             tasks_per_batch=2)
MODELS = {
    "resnet_anp": ("ANP", dict(CFG3D, agg_mode="attention")),
    "resnet_cnp_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max")),
    "vanilla_anp": ("ANPShapeNet1D", dict(CFGV, agg_mode="attention", dim_r=64)),
    "vanilla_cnp_mean": ("CNPShapeNet1D", dict(CFGV, agg_mode="mean", dim_r=100)),
}


# ---- the contract: parts built apart and merged = the stream over everything -----------------------------------------------------------
@pytest.mark.parametrize("split", MR.SPLITS)
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("chunking", [n for n, calls in S.CHUNKINGS.items() if len(calls) > 1])
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_merged_parts_equal_the_streamed_whole(d, m, chunking, kind, split):
    c = S.case(kind, d, m, chunking)
    want = S.streamed(c)
    parts = [MR.part(c, calls) for calls in MR.groups(c, split)]
    got = MR.merge(parts)
    for name, x, y in (("A", got.A, want.A), ("a", got.a, want.a), ("vs", got.vs, want.vs)):
        err = (x - y).abs().max().item() / y.abs().max().item()
        assert err <= 1e-12, f"{name} {kind} d={d} m={m} {chunking} {split}: {err:.2e} of its scale"
    assert got.M == want.M == max(p.M for p in parts) and got.cnt == want.cnt == c["totals"]
    assert bool(torch.isfinite(got.A).all()) and bool(torch.isfinite(got.a).all())


def test_fresh_states_add_nothing_and_a_floor_is_a_common_factor():
    c = S.case("live", 16, 16, "7_32_31")
    st = S.streamed(c)
    fresh = S.State(2, S.H, 16, 16)
    for order in ([st, fresh], [fresh, st], [fresh, st, fresh]):
        got = MR.merge(order)
        assert torch.equal(got.A, st.A) and torch.equal(got.a, st.a) and torch.equal(got.vs, st.vs) and got.M == st.M and got.cnt == st.cnt
    none = MR.merge([fresh, fresh])
    assert none.M == -math.inf and not none.A.any() and none.cnt == [0, 0]                  # exp(-inf - -inf) is never formed
    assert MR.merge([st], floor=st.M - 3.0).M == st.M and torch.equal(MR.merge([st], floor=st.M - 3.0).A, st.A)
    # a floor above M: A and a take ONE common factor, vs and cnt none.  favor_query's quotient cancels the factor up to its eps terms
    # (the key feature's +eps is relative to the stabiliser, so a raised stabiliser weighs it exp(floor - M) times more): at 1 / 64
    # above M the float64 result moves by far less than the fp32 bar of the GPU tests, at 3 above it visibly does
    up = MR.merge([st], floor=st.M + 3.0)
    assert up.M == st.M + 3.0 and torch.equal(up.vs, st.vs) and up.cnt == st.cnt
    assert (up.A - math.exp(-3.0) * st.A).abs().max().item() <= 1e-15 * st.A.abs().max().item()
    assert (up.a - math.exp(-3.0) * st.a).abs().max().item() <= 1e-15 * st.a.abs().max().item()
    q, base = c["q"], st.query(c["q"], c["proj"])
    near = MR.merge([st], floor=st.M + 2.0 ** -6).query(q, c["proj"])
    assert (near - base).abs().max().item() <= 2.5e-5 * base.abs().max().item()
    assert (up.query(q, c["proj"]) - base).abs().max().item() > 1e-4 * base.abs().max().item()


# ---- the host build -----------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_entry_and_it_is_unsupported(hostsim):
    c = hostsim.c
    buf = torch.full((1024,), 7.0)
    other = torch.full((1024,), 3.0)
    table = (C.c_void_p * 1)(other.data_ptr())
    assert c.mlhot_favor_summary_merge(table, 1, None, 2, 2, 64, 266, C.c_void_p(buf.data_ptr()), 4096, None) == 4      # MLHOT_ERR_UNSUPPORTED
    assert "favor_summary_merge" in c.mlhot_last_error().decode()
    assert bool((buf == 7.0).all()) and bool((other == 3.0).all())
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError, match="favor_summary_merge serves"):                  # the wrapper refuses before it allocates
        hostsim.favor_summary_merge([other.view(torch.uint8)], 2, 2, 64, 266)


# ---- favor_merge's refusals -----------------------------------------------------------------------------------------------------------
def _keys(route="summary", dims=(2, 5, 2, 16, 16), lens=(5, 3), dtype=torch.uint8):
    from mlhot.ops import FavorKeyState
    return FavorKeyState(route, dims, buf=torch.zeros(64, dtype=dtype), lens=lens)


def test_favor_merge_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_merge
    with pytest.raises(MlhotError, match="at least one summary state"):
        favor_merge([])
    with pytest.raises(MlhotError, match="must be a sequence"):
        favor_merge(None)
    with pytest.raises(MlhotError, match=r"states\[1\] is a Tensor"):
        favor_merge([_keys(), torch.zeros(3)])
    with pytest.raises(MlhotError, match=r"states\[1\] has route 'cached'.*hold rows, not sums"):
        favor_merge([_keys(), _keys("cached")])
    with pytest.raises(MlhotError, match=r"states\[0\] has route 'plain'"):
        favor_merge([_keys("plain")])
    with pytest.raises(MlhotError, match=r"states\[2\] was built for T=2 H=2 d=16 m=32, states\[0\] for T=2 H=2 d=16 m=16"):
        favor_merge([_keys(), _keys(), _keys(dims=(2, 9, 2, 16, 32))])
    with pytest.raises(MlhotError, match=r"states\[1\] was built for T=1 "):
        favor_merge([_keys(), _keys(dims=(1, 5, 2, 16, 16), lens=(5,))])
    with pytest.raises(MlhotError, match=r"states\[1\] lies on cpu as torch.float32"):
        favor_merge([_keys(), _keys(dtype=torch.float32)])
    for floor in (1.0, torch.zeros(2), torch.zeros(1, dtype=torch.float64)):
        with pytest.raises(MlhotError, match="floor must be None or one fp32 value"):
            favor_merge([_keys()], floor=floor)


# ---- the fold order -------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records which buffers every favor_summary_merge call was handed, by name."""

    def __init__(self):
        self.calls, self.names = [], {}

    def name(self, buf):
        return self.names[buf.data_ptr()]

    def favor_summary_merge(self, bufs, T, H, d, m, floor=None):
        out = torch.zeros(64, dtype=torch.uint8)
        self.calls.append(([self.name(b) for b in bufs], (T, H, d, m), floor))
        self.names[out.data_ptr()] = f"r{len(self.calls) - 1}"
        self.keep = getattr(self, "keep", []) + [out]                     # addresses stay unique
        return out


@pytest.mark.parametrize("n,want", [
    (1, [[0]]),
    (8, [list(range(8))]),
    (9, [list(range(8)), ["r0", 8]]),
    (15, [list(range(8)), ["r0", *range(8, 15)]]),
    (16, [list(range(8)), ["r0", *range(8, 15)], ["r1", 15]]),
    (17, [list(range(8)), ["r0", *range(8, 15)], ["r1", 15, 16]]),
])
def test_more_than_eight_states_fold_in_groups_left_to_right(monkeypatch, n, want):
    from mlhot import ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    states = [_keys(lens=(i + 1, 2 * i)) for i in range(n)]
    for i, s in enumerate(states):
        rec.names[s.buf.data_ptr()] = i
    floor = torch.zeros(1)
    out = ops.favor_merge(states, floor=floor)
    assert [c[0] for c in rec.calls] == want
    assert all(c[1] == (2, 2, 16, 16) and c[2] is floor for c in rec.calls)
    assert out.route == "summary" and out.buf is rec.keep[-1]
    lens = (sum(i + 1 for i in range(n)), sum(2 * i for i in range(n)))
    assert out.lens == lens and out.dims == (2, max(lens), 2, 16, 16)
    assert all(s.lens == (i + 1, 2 * i) for i, s in enumerate(states))


def test_a_merged_state_without_a_shot_in_a_task_is_still_refused_by_favor_query(monkeypatch):
    from mlhot import ops
    from mlhot.binding import MlhotError
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    states = [_keys(lens=(5, 0)), _keys(lens=(2, 0))]
    for i, s in enumerate(states):
        rec.names[s.buf.data_ptr()] = i
    merged = ops.favor_merge(states)
    assert merged.lens == (7, 0)
    with pytest.raises(MlhotError, match=r"has absorbed no shot \(shots per task: \[7, 0\]\)"):
        ops.favor_query(torch.zeros(2, 3, 2, 16), merged, None, torch.zeros(16, 16))


# ---- mlhot.cached.merge's refusals ----------------------------------------------------------------------------------------------------
def _model(name):
    method, cfg = MODELS[name]
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval()


def _summary_state(model, lens=(40, 31)):
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    from networks._resnet_np import ResNetNP
    d = 256 if isinstance(model, ResNetNP) else 64
    keys = FavorKeyState("summary", (2, max(lens), 8, d, model.attn.projection_matrix.shape[0]), buf=torch.zeros(64, dtype=torch.uint8), lens=tuple(lens))
    return ContextState(model, 2, max(lens), fingerprint(model), "attention", keys=keys, lens=lens, form="summary")


@pytest.mark.parametrize("name", ["resnet_anp", "vanilla_anp"])
def test_cached_merge_refusals_and_bookkeeping(monkeypatch, name):
    from mlhot import cached, ops
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    model = _model(name)
    a, b = _summary_state(model, (17, 17)), _summary_state(model, (23, 9))
    with pytest.raises(ValueError, match="at least one state"):
        cached.merge(model, [])
    with pytest.raises(ValueError, match="must be a sequence"):
        cached.merge(model, a)
    keys = ContextState(model, 2, 5, fingerprint(model), "attention", keys=FavorKeyState("cached", (2, 5, 8, 64, 16), buf=None), vh=torch.zeros(1))
    with pytest.raises(ValueError, match=r"states\[1\] has form 'keys'.*per-shot rows in at most 32 slots"):
        cached.merge(model, [a, keys])
    other = _model(name)
    with pytest.raises(ValueError, match=r"not made by this model's condition\(\) \(states\[1\]\)"):
        cached.merge(model, [a, _summary_state(other)])
    with pytest.raises(ValueError, match="not made by this model"):
        cached.merge(other, [a, b])
    with pytest.raises(ValueError, match="not made by this model"):
        cached.merge(model, [a, "state"])
    three = _summary_state(model)
    three.T = 3
    with pytest.raises(ValueError, match=r"states\[1\] holds 3 tasks"):
        cached.merge(model, [a, three])
    # what passes the host checks: lens add up, Nc is their maximum, the inputs are untouched (the launch is the recorder's)
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    rec.names[a.keys.buf.data_ptr()], rec.names[b.keys.buf.data_ptr()] = "a", "b"
    merged = cached.merge(model, [a, b])
    assert [c[0] for c in rec.calls] == [["a", "b"]]
    assert merged.lens == (40, 26) and merged.Nc == 40 and merged.form == "summary" and merged.kind == "attention" and merged.capacity is None
    assert merged.owner is model and merged.fingerprint == fingerprint(model) and merged.vh is None and merged.kh is None
    assert a.lens == (17, 17) and b.lens == (23, 9)
    model.train()
    with pytest.raises(ValueError, match=r"merge is a test-mode path: call model.eval\(\) first"):
        cached.merge(model, [a, b])
    model.eval()
    with torch.no_grad():
        next(model.parameters()).add_(1.0)
    with pytest.raises(ValueError, match=r"stale - a parameter of the model changed since condition\(\)"):
        cached.merge(model, [a, b])


@pytest.mark.parametrize("name", ["resnet_cnp_max", "vanilla_cnp_mean"])
def test_cached_merge_refuses_a_latent_state(name):
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    model = _model(name)
    z = ContextState(model, 2, 4, fingerprint(model), "latent", z=torch.zeros(2, 64))
    with pytest.raises(ValueError, match=r"states\[0\] is a 'latent' state - it is stored behind its finishing Linear"):
        cached.merge(model, [z, z])
