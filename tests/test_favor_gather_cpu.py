"""Picking and combining tasks across FAVOR+ summary states without a GPU: the float64 gather of
tests/favor_gather_ref.py against the float64 stream over each output task's shots under the forced stabiliser M' - the contract of
the feature -, the host build's entry, every refusal of mlhot.ops.favor_gather and mlhot.cached.select that is decided on the host,
and the tables of the group-of-8 fold on a recording stub of the binding call."""
import ctypes as C
import math

import pytest
import torch

from tests import favor_gather_ref as G
from tests import favor_summary_ref as S
from tests.test_favor_merge_cpu import _keys, _model, _summary_state

# name -> (task counts of the sources (0: a fresh one), the table)
TABLES = {
    "identity": ((2,), [[(0, 0)], [(0, 1)]]),
    "swap_across": ((2, 2), [[(0, 1)], [(1, 0)]]),
    "duplicate_task": ((2, 2), [[(1, 1)], [(1, 1)], [(0, 0)]]),
    "two_parts": ((2, 2), [[(0, 0), (1, 0)], [(0, 1), (1, 1)]]),
    "one_and_five_into_three": ((1, 5), [[(1, 4), (0, 0)], [(1, 0)], [(1, 2), (1, 3)]]),
    "empty_task": ((2, 2), [[(0, 0)], [], [(1, 1), (0, 1)]]),
    "fresh_source": ((2, 0, 2), [[(0, 0), (1, 0)], [(1, 0), (2, 1)]]),
    "eight_parts": ((3, 3, 3), [[(i, u) for i in range(3) for u in range(3)][:8], [(2, 2)]]),
}


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("name", list(TABLES))
@pytest.mark.parametrize("d,m", [(16, 16), (64, 266)])
def test_gathered_states_equal_the_stream_under_the_forced_stabiliser(d, m, name, kind):
    tasks, parts = TABLES[name]
    lib = G.library(kind, tasks, S.H, d, m)
    states = [src.state for src in lib]
    got = G.gather(states, parts)
    assert got.M == max(st.M for st in states)
    want = G.direct(lib, parts, got.M)
    for what, x, y in (("A", got.A, want.A), ("a", got.a, want.a), ("vs", got.vs, want.vs)):
        err = (x - y).abs().max().item() / y.abs().max().item()
        assert err <= 1e-12, f"{what} {name} {kind} d={d} m={m}: {err:.2e} of its scale"
    assert got.cnt == want.cnt == [sum(lib[i].lens[u] for i, u in row) for row in parts]
    assert got.A.shape[0] == len(parts) and bool(torch.isfinite(got.A).all()) and bool(torch.isfinite(got.a).all())
    for t, row in enumerate(parts):
        if not row:                                                                     # an empty task: the rows of a fresh state
            assert not got.A[t].any() and not got.a[t].any() and not got.vs[t].any() and got.cnt[t] == 0


def test_unnamed_states_enter_the_kernels_stabiliser_and_the_op_drops_them():
    lib = G.library("peak_last", (2, 2), S.H, 16, 16)
    states = [src.state for src in lib]
    parts = [[(0, 1)], [(0, 0)]]
    assert states[1].M > states[0].M + 10
    assert G.gather(states, parts).M == states[1].M and G.op(states, parts).M == states[0].M
    got = G.op(states, parts)
    assert torch.equal(got.A[0], states[0].A[1]) and torch.equal(got.A[1], states[0].A[0]) and got.cnt == [5, 5]      # a permutation: rows unchanged
    up = G.op(states, parts, floor=states[0].M + 3.0)
    assert up.M == states[0].M + 3.0 and torch.equal(up.vs, got.vs)
    assert (up.A - math.exp(-3.0) * got.A).abs().max().item() <= 1e-15 * got.A.abs().max().item()
    none = G.op(states, [[], []])
    assert none.M == -math.inf and not none.A.any() and none.cnt == [0, 0]


# ---- the host build -----------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_entry_and_it_is_unsupported(hostsim):
    c = hostsim.c
    buf, other = torch.full((1024,), 7.0), torch.full((1024,), 3.0)
    parts = torch.zeros(2, 1, 2, dtype=torch.int32)
    table, counts = (C.c_void_p * 1)(other.data_ptr()), (C.c_int * 1)(2)
    rc = c.mlhot_favor_summary_gather(table, counts, 1, C.c_void_p(parts.data_ptr()), 1, None, 2, 2, 64, 266, C.c_void_p(buf.data_ptr()), 4096, None)
    assert rc == 4                                                                       # MLHOT_ERR_UNSUPPORTED
    assert "favor_summary_gather" in c.mlhot_last_error().decode()
    for n, P in ((0, 1), (9, 1), (1, 0), (1, 9)):                                        # MLHOT_ERR_ARG before anything else
        assert c.mlhot_favor_summary_gather(table, counts, n, C.c_void_p(parts.data_ptr()), P, None, 2, 2, 64, 266, C.c_void_p(buf.data_ptr()), 4096, None) == 1
    assert bool((buf == 7.0).all()) and bool((other == 3.0).all())


# ---- favor_gather's refusals --------------------------------------------------------------------------------------------------------
def test_favor_gather_refusals():
    from mlhot.ops import favor_gather
    ok = [[(0, 0)], [(0, 1)]]
    with pytest.raises(ValueError, match="at least one summary state"):
        favor_gather([], ok)
    with pytest.raises(ValueError, match="must be a sequence"):
        favor_gather(None, ok)
    with pytest.raises(ValueError, match=r"states\[1\] is a Tensor"):
        favor_gather([_keys(), torch.zeros(3)], ok)
    with pytest.raises(ValueError, match=r"states\[1\] has route 'cached'.*hold rows, not sums"):
        favor_gather([_keys(), _keys("cached")], ok)
    with pytest.raises(ValueError, match=r"states\[0\] has route 'long'.*hold rows, not sums"):
        favor_gather([_keys("long")], ok)
    with pytest.raises(ValueError, match=r"states\[0\] has route 'plain'"):
        favor_gather([_keys("plain")], ok)
    with pytest.raises(ValueError, match=r"states\[2\] was built for H=2 d=16 m=32, states\[0\] for H=2 d=16 m=16"):
        favor_gather([_keys(), _keys(), _keys(dims=(2, 9, 2, 16, 32))], ok)
    with pytest.raises(ValueError, match=r"states\[1\] lies on cpu as torch.float32"):
        favor_gather([_keys(), _keys(dtype=torch.float32)], ok)
    for floor in (1.0, torch.zeros(2), torch.zeros(1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="floor must be None or one fp32 value"):
            favor_gather([_keys()], ok, floor=floor)
    with pytest.raises(ValueError, match="parts is empty"):
        favor_gather([_keys()], [])
    with pytest.raises(ValueError, match="parts must be a sequence"):
        favor_gather([_keys()], 3)
    with pytest.raises(ValueError, match=r"parts\[1\]\[0\] names state 1; there are 1 states"):
        favor_gather([_keys()], [[(0, 0)], [(1, 0)]])
    with pytest.raises(ValueError, match=r"parts\[0\]\[1\] names state -1"):
        favor_gather([_keys()], [[(0, 0), (-1, 0)]])
    with pytest.raises(ValueError, match=r"parts\[0\]\[0\] names task 2 of states\[0\], which holds 2 tasks"):
        favor_gather([_keys()], [[(0, 2)]])
    with pytest.raises(ValueError, match=r"parts\[0\]\[0\] names task 1 of states\[1\], which holds 1 tasks"):
        favor_gather([_keys(), _keys(dims=(1, 5, 2, 16, 16), lens=(5,))], [[(1, 1)]])
    with pytest.raises(ValueError, match=r"parts\[0\] names 9 parts; a task takes at most 8"):
        favor_gather([_keys()], [[(0, 0)] * 9])
    with pytest.raises(ValueError, match=r"parts\[0\]\[0\] must be a \(state_index, task_index\) pair"):
        favor_gather([_keys()], [[3]])
    with pytest.raises(ValueError, match=r"parts\[0\]\[0\] must hold two integers"):
        favor_gather([_keys()], [[(0, 0.5)]])


# ---- the fold: which states and which table every launch gets -------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records the buffers (by name), task counts and table of every favor_summary_gather call."""

    def __init__(self):
        self.calls, self.names, self.keep = [], {}, []

    def favor_summary_gather(self, bufs, tasks, parts, H, d, m, floor=None):
        out = torch.zeros(64, dtype=torch.uint8)
        self.calls.append(([self.names[b.data_ptr()] for b in bufs], list(tasks), parts.tolist(), (H, d, m), floor))
        self.names[out.data_ptr()] = f"r{len(self.calls) - 1}"
        self.keep.append(out)
        return out

    def favor_summary_init(self, T, H, d, m, device):
        out = torch.zeros(8, dtype=torch.uint8)
        self.names[out.data_ptr()] = "fresh"
        self.keep.append(out)
        return out


def _recorded(monkeypatch, states, parts, floor=None):
    from mlhot import ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    for i, s in enumerate(states):
        rec.names[s.buf.data_ptr()] = i
    return ops.favor_gather(states, parts, floor=floor), rec


def test_unnamed_states_are_dropped_and_lens_add_up(monkeypatch):
    states = [_keys(lens=(5, 3)), _keys(lens=(7, 7)), _keys(dims=(3, 9, 2, 16, 16), lens=(1, 2, 9))]
    floor = torch.zeros(1)
    out, rec = _recorded(monkeypatch, states, [[(2, 2), (0, 1)], [], [(2, 0)], [(0, 1)]], floor)
    assert len(rec.calls) == 1
    names, tasks, table, dims, fl = rec.calls[0]
    assert names == [0, 2] and tasks == [2, 3] and dims == (2, 16, 16) and fl is floor                   # states[1] is named by no part
    assert table == [[[1, 2], [0, 1]], [[-1, 0], [-1, 0]], [[1, 0], [-1, 0]], [[0, 1], [-1, 0]]]         # P = 2, rows ended by state -1
    assert out.route == "summary" and out.lens == (12, 0, 1, 3) and out.dims == (4, 12, 2, 16, 16) and out.buf is rec.keep[-1]
    assert [s.lens for s in states] == [(5, 3), (7, 7), (1, 2, 9)]


@pytest.mark.parametrize("n", [8, 9, 17])
def test_more_than_eight_named_states_fold_in_groups(monkeypatch, n):
    """Task t takes task t of the states i with i % 3 == t: every state is named, no task has more than 8 parts."""
    states = [_keys(dims=(3, 4, 2, 16, 16), lens=(i + 1, i + 2, i + 3)) for i in range(n)]
    parts = [[(i, t) for i in range(n) if i % 3 == t] for t in range(3)]
    out, rec = _recorded(monkeypatch, states, parts)
    want = {8: [list(range(8))], 9: [list(range(8)), ["r0", 8]], 17: [list(range(8)), ["r0", *range(8, 15)], ["r1", 15, 16]]}[n]
    assert [c[0] for c in rec.calls] == want
    assert all(c[1] == [3] * len(c[0]) for c in rec.calls)
    first = [[[i, t] for i in range(8) if i % 3 == t] for t in range(3)]
    assert [[e for e in row if e[0] >= 0] for row in rec.calls[0][2]] == first
    if n == 17:                                       # the running result leads every task's row, then the group's states at slots 1 ..
        assert [[e for e in row if e[0] >= 0] for row in rec.calls[1][2]] == [[[0, t]] + [[i - 7, t] for i in range(8, 15) if i % 3 == t] for t in range(3)]
        assert [[e for e in row if e[0] >= 0] for row in rec.calls[2][2]] == [[[0, 0], [1, 0]], [[0, 1], [2, 1]], [[0, 2]]]
    assert out.lens == tuple(sum(i + 1 + t for i in range(n) if i % 3 == t) for t in range(3))


def test_a_task_that_starts_in_a_later_group_gets_no_running_part(monkeypatch):
    states = [_keys() for _ in range(9)]
    parts = [[(i, 0) for i in range(8)], [(8, u) for u in (0, 1)] * 4]                  # task 1: eight parts, all of the ninth state
    out, rec = _recorded(monkeypatch, states, parts)
    assert [c[0] for c in rec.calls] == [list(range(8)), ["r0", 8]]
    assert rec.calls[1][2] == [[[0, 0]] + [[-1, 0]] * 7, [[1, 0], [1, 1]] * 4]
    assert out.lens == (40, 32)


def test_no_part_at_all_is_the_fresh_state(monkeypatch):
    from mlhot import ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    out = ops.favor_gather([_keys()], [[], []])
    assert rec.calls[0][0] == ["fresh"] and rec.calls[0][1] == [1] and rec.calls[0][2] == [[[-1, -1]], [[-1, -1]]]
    assert out.lens == (0, 0) and out.dims == (2, 0, 2, 16, 16)
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError, match="has absorbed no shot"):
        ops.favor_query(torch.zeros(2, 3, 2, 16), out, None, torch.zeros(16, 16))


# ---- mlhot.cached.select's refusals and bookkeeping ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet_anp", "vanilla_anp"])
def test_cached_select_refusals_and_bookkeeping(monkeypatch, name):
    from mlhot import cached, ops
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    model = _model(name)
    a, b = _summary_state(model, (17, 17)), _summary_state(model, (23, 9))
    ok = [(0, 1), (1, 0)]
    with pytest.raises(ValueError, match="at least one state"):
        cached.select(model, [], ok)
    with pytest.raises(ValueError, match="must be a sequence"):
        cached.select(model, a, ok)
    keys = ContextState(model, 2, 5, fingerprint(model), "attention", keys=FavorKeyState("cached", (2, 5, 8, 64, 16), buf=None), vh=torch.zeros(1))
    with pytest.raises(ValueError, match=r"select: states\[1\] has form 'keys'.*per-shot rows in at most 32 slots"):
        cached.select(model, [a, keys], ok)
    long = ContextState(model, 2, 40, fingerprint(model), "attention", keys=FavorKeyState("long", (2, 40, 8, 64, 16), buf=None), vh=torch.zeros(1), form="long")
    with pytest.raises(ValueError, match=r"select: states\[0\] has form 'long'.*per-shot rows in at most 256 slots"):
        cached.select(model, [long], ok)
    other = _model(name)
    with pytest.raises(ValueError, match=r"not made by this model's condition\(\) \(states\[1\]\)"):
        cached.select(model, [a, _summary_state(other)], ok)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.select(other, [a, b], ok)
    with pytest.raises(ValueError, match=r"3 picks, the model was built for tasks_per_batch = 2"):
        cached.select(model, [a, b], [(0, 0), (0, 1), (1, 0)])
    with pytest.raises(ValueError, match=r"picks\[1\] is empty"):
        cached.select(model, [a, b], [(0, 0), []])
    with pytest.raises(ValueError, match=r"picks\[0\] names \(1, 0\) twice"):
        cached.select(model, [a, b], [[(1, 0), (0, 0), (1, 0)], (0, 1)])
    with pytest.raises(ValueError, match=r"picks\[1\] names 9 parts"):
        cached.select(model, [a, b], [(0, 0), [(0, 0), (0, 1), (1, 0), (1, 1)] * 2 + [(0, 0)]])
    with pytest.raises(ValueError, match=r"parts\[1\]\[0\] names task 2 of states\[1\]"):
        cached.select(model, [a, b], [(0, 0), (1, 2)])
    with pytest.raises(ValueError, match=r"parts\[0\]\[0\] names state 2"):
        cached.select(model, [a, b], [(2, 0), (1, 0)])
    rec = _Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    rec.names[a.keys.buf.data_ptr()], rec.names[b.keys.buf.data_ptr()] = "a", "b"
    a.wq = ("wq",)
    got = cached.select(model, [a, b], [(0, 1), [(1, 0), (0, 1)]])                      # the same pair in different tasks is fine
    assert [c[0] for c in rec.calls] == [["a", "b"]] and rec.calls[0][2] == [[[0, 1], [-1, 0]], [[1, 0], [0, 1]]]
    assert got.lens == (17, 40) and got.Nc == 40 and got.T == 2 and got.form == "summary" and got.kind == "attention" and got.capacity is None
    assert got.owner is model and got.fingerprint == fingerprint(model) and got.vh is None and got.kh is None and got.wq is a.wq
    assert a.lens == (17, 17) and b.lens == (23, 9)
    model.train()
    with pytest.raises(ValueError, match=r"select is a test-mode path: call model.eval\(\) first"):
        cached.select(model, [a, b], ok)
    model.eval()
    with torch.no_grad():
        next(model.parameters()).add_(1.0)
    with pytest.raises(ValueError, match=r"stale - a parameter of the model changed since condition\(\)"):
        cached.select(model, [a, b], ok)


@pytest.mark.parametrize("name", ["resnet_cnp_max", "vanilla_cnp_mean"])
def test_cached_select_refuses_a_latent_state(name):
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    model = _model(name)
    z = ContextState(model, 2, 4, fingerprint(model), "latent", z=torch.zeros(2, 64))
    with pytest.raises(ValueError, match=r"states\[0\] is a 'latent' state - it is stored behind its finishing Linear"):
        cached.select(model, [z, z], [(0, 0), (1, 1)])
