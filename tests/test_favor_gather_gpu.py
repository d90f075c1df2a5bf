"""mlhot.ops.favor_gather / mlhot_favor_summary_gather on the MI355X (csrc/favor_summary.h): the identities bit for
bit over the WHOLE buffer (out pre-filled with NaN), the tables against the float64 stream over each output task's shots under the
forced stabiliser M' (tests/favor_gather_ref.py), the query through a gathered state, poisoned paddings, and the refusals.  The bar is
tests/test_favor_summary_gpu.py's: U.RTOL of each quantity's scale.  No test hands the kernel an invalid table.

The fold of more than 8 named states is held to favor_merge's: an identity table over 9 states would need 9 parts per task, which the
op refuses, so most states hold shots in ONE task only and a task takes (i, t) of exactly the states that hold shots for it - every
state is named, no task has more than 8 parts, and favor_merge of the same states adds the same terms in the same order plus exact
zeros (fma(s, 0, o) is o).  The states that stand first and second in a launch's chain (0 and 1; 8 and 15 behind the running result)
hold shots in every task: fold_step rounds the second product of a chain and fuses the first onto it, so a zero there would change
which product is rounded.  Run with -m gpu."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import favor_cached_ref as R
from tests import favor_gather_ref as G
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 2, 16, 16), (3, 2, 64, 266)]            # (T, H, d, m): mp == m; padded feature rows and T H = 6, so cnt has padding
BIG = (2, 8, 256, 1419)


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _absorbed(src, lens=None):
    from mlhot.ops import favor_absorb
    lens = src.lens if lens is None else lens
    return favor_absorb(None, _dev(src.k), _dev(src.v), src.proj.to(DEV), lens=None if all(n == src.k.shape[2] for n in lens) else lens)


@functools.lru_cache(maxsize=None)
def _states(kind, tasks, H, d, m):
    return tuple(_absorbed(src) for src in G.library(kind, tasks, H, d, m))


def _m_at(T, H, d, m):
    mp = (m + 15) // 16 * 16
    return T * H * (mp * d + mp + d)


def _raw(gpulib, states, parts, floor=None):
    """The binding call on a NaN-filled out -> the whole buffer as int32 words."""
    P = max(1, max(len(r) for r in parts))
    table = torch.tensor([list(r) + [(-1, 0)] * (P - len(r)) for r in parts], dtype=torch.int32).to(DEV)
    _, _, H, d, m = states[0].dims
    nb = gpulib.favor_summary_bytes(len(parts), H, d, m)
    out = torch.full((nb // 4,), float("nan"), device=DEV).view(torch.uint8)
    got = gpulib.favor_summary_gather([s.buf for s in states], [s.dims[0] for s in states], table, H, d, m, floor=floor, out=out)
    assert got.data_ptr() == out.data_ptr()
    return out.view(torch.int32)


def _expected(gpulib, states, rows, M):
    """The whole buffer of a state whose task t holds the rows of (state i, task u) = rows[t], unchanged; paddings zero."""
    _, _, H, d, m = states[0].dims
    T = len(rows)
    buf = torch.zeros(gpulib.favor_summary_bytes(T, H, d, m), dtype=torch.uint8, device=DEV)
    views = gpulib.favor_summary_views(buf, T, H, d, m)
    for t, (i, u) in enumerate(rows):
        for dst, src in zip(views[:4], states[i].summary()[:4]):
            dst[t] = src[u]
    views[0][:, :, m:] = 0
    views[1][:, :, m:] = 0
    views[4][0] = M
    return buf.view(torch.int32)


def _errors(state, want, m):
    A, a, vs, cnt, M = state.summary()
    return U.rel_err(A[:, :, :m], want.A), U.rel_err(a[:, :, :m], want.a), U.rel_err(vs, want.vs)


# ---- 1. bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,d,m", SHAPES + [BIG])
def test_identity_permutation_and_duplicate_bit_for_bit(gpulib, T, H, d, m):
    a, b = _states("peak_last", (T, T), H, d, m)
    Ma, Mb = a.summary()[4].item(), b.summary()[4].item()
    assert Mb > Ma + 10
    ident = [[(0, t)] for t in range(T)]
    assert torch.equal(_raw(gpulib, [a], ident), _expected(gpulib, [a], [r[0] for r in ident], Ma))       # the state itself, paddings zeroed
    perm = [[(0, (t + 1) % T)] for t in range(T)]
    assert torch.equal(_raw(gpulib, [a], perm), _expected(gpulib, [a], [r[0] for r in perm], Ma))
    # a duplicate, more tasks than the source holds, rows of the state that carries M' (its scale is exactly 1) next to an unnamed one
    dup = [[(1, T - 1)], [(1, T - 1)], [(1, 0)], [(1, T - 1)]]
    assert torch.equal(_raw(gpulib, [a, b], dup), _expected(gpulib, [a, b], [r[0] for r in dup], Mb))
    before = a.buf.clone()
    _raw(gpulib, [a], ident)
    assert torch.equal(a.buf, before)                                                   # the inputs are only read


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("T,H,d,m", SHAPES)
def test_identity_table_over_n_states_equals_favor_merge(gpulib, T, H, d, m, n):
    from mlhot.ops import favor_gather, favor_merge
    states = list(_states("live", (T,) * 8, H, d, m)[:n])
    parts = [[(i, t) for i in range(n)] for t in range(T)]
    merged = favor_merge(states)
    assert torch.equal(_raw(gpulib, states, parts), merged.buf.view(torch.int32))
    got = favor_gather(states, parts)
    assert torch.equal(got.buf.view(torch.int32), merged.buf.view(torch.int32)) and got.lens == merged.lens and got.dims == merged.dims
    low = torch.tensor([min(s.summary()[4].item() for s in states) - 1.0], device=DEV)
    assert torch.equal(_raw(gpulib, states, parts, floor=low), merged.buf.view(torch.int32))               # a floor below every M changes nothing
    up = torch.tensor([max(s.summary()[4].item() for s in states) + 3.0], device=DEV)
    assert torch.equal(_raw(gpulib, states, parts, floor=up), favor_merge(states, floor=up).buf.view(torch.int32))


def test_identity_table_over_two_states_equals_favor_merge_at_the_large_shape(gpulib):
    from mlhot.ops import favor_merge
    T, H, d, m = BIG
    states = list(_states("peak_last", (T, T), H, d, m))
    assert torch.equal(_raw(gpulib, states, [[(0, t), (1, t)] for t in range(T)]), favor_merge(states).buf.view(torch.int32))


@pytest.mark.parametrize("n", [9, 17])
def test_nine_and_seventeen_named_states_equal_favor_merges_fold(gpulib, n, monkeypatch):
    from mlhot.ops import favor_gather, favor_merge
    T, H, d, m = 4, 2, 64, 266
    lib = G.library("live", (T,) * n, H, d, m, seed=n)
    full = (0, 1, 8, 15)                               # the first two terms of every launch's chain: states with shots in every task
    singles = [i for i in range(n) if i not in full]
    owner = {i: k % T for k, i in enumerate(singles)}
    states = [_absorbed(src, [5 if i in full or owner[i] == t else 0 for t in range(T)]) for i, src in enumerate(lib)]
    parts = [[(i, t) for i in range(n) if i in full or owner[i] == t] for t in range(T)]
    assert max(len(r) for r in parts) == (8 if n == 17 else 5) and G.named(parts) == list(range(n))
    calls, real = [], gpulib.favor_summary_gather
    monkeypatch.setattr(gpulib, "favor_summary_gather", lambda bufs, *a, **kw: (calls.append(len(bufs)), real(bufs, *a, **kw))[1])
    got, merged = favor_gather(states, parts), favor_merge(states)
    assert calls == ([8, 2] if n == 9 else [8, 8, 3])
    at = _m_at(T, H, d, m)
    gf, mf = got.buf.view(torch.float32), merged.buf.view(torch.float32)
    assert not bool(torch.isnan(gf[:at + 16]).any())
    assert torch.equal(gf[:at + 16], mf[:at + 16])                                      # A, a, vs and M's block (a skipped +0 may leave a -0: float equality)
    assert torch.equal(got.buf.view(torch.int32)[at + 16:], merged.buf.view(torch.int32)[at + 16:])        # cnt and its padding
    assert got.lens == merged.lens == tuple(5 * len(r) for r in parts)
    assert got.summary()[4].item() == max(s.summary()[4].item() for s in states)


@pytest.mark.parametrize("T,H,d,m", SHAPES)
def test_a_state_that_no_part_names_changes_nothing(gpulib, T, H, d, m):
    from mlhot.ops import favor_gather
    a, b, c = _states("peak", (T, T, T), H, d, m)
    assert c.summary()[4].item() > a.summary()[4].item() + 10                            # the unnamed state would raise M' by far
    with_c = favor_gather([a, c, b], [[(0, t), (2, (t + 1) % T)] for t in range(T)])
    without = favor_gather([a, b], [[(0, t), (1, (t + 1) % T)] for t in range(T)])
    assert torch.equal(with_c.buf.view(torch.int32), without.buf.view(torch.int32)) and with_c.lens == without.lens


# ---- 2. against float64 -----------------------------------------------------------------------------------------------------------------
def _tables(T):
    """name -> (task counts of the sources (0: a fresh one), the table): P = 1, 2 and 8, a fresh source, an empty task, T_i != T_out."""
    return {
        "p1": ((T, T), [[(t % 2, (t + 1) % T)] for t in range(T)]),
        "p2": ((T, T), [[(0, t), (1, (t + 1) % T)] for t in range(T)]),
        "p8": ((T, T, T, T), [[(i % 4, (t + i // 4) % T) for i in range(8)] for t in range(T)]),
        "fresh_source": ((T, 0, T), [[(0, t), (1, 0), (2, t)] for t in range(T)]),
        "empty_task": ((T, T), [[]] + [[(1, t), (0, 0)] for t in range(1, T)]),
        "one_and_five_into_three": ((1, 5), [[(1, 4), (0, 0)], [(1, 0)], [(1, 2), (1, 3)]]),
    }


def _check(gpulib, kind, tasks, parts, H, d, m, floor=None, label=""):
    from mlhot.ops import favor_gather
    lib, states = G.library(kind, tasks, H, d, m), _states(kind, tasks, H, d, m)
    fl = None if floor is None else torch.tensor([floor], device=DEV)
    got = favor_gather(states, parts, floor=fl)
    M64 = G.op([src.state for src in lib], parts, -math.inf if floor is None else floor).M
    want = G.direct(lib, parts, M64)
    A, a, vs, cnt, M = got.summary()
    errs = _errors(got, want, m)
    Ms = [states[i].summary()[4].item() for i in G.named(parts)]
    print(f"gather {label} {kind} H={H} d={d} m={m}: A {errs[0]:.2e}, a {errs[1]:.2e}, vs {errs[2]:.2e} of their scales; M of the named states "
          f"{min(Ms):.3f} .. {max(Ms):.3f}, M' {M.item():.3f}")
    assert max(errs) <= U.RTOL
    assert M.item() == (max(Ms) if floor is None else max(Ms + [fl.item()]))             # the maximum over the named states (and the floor), exactly
    assert cnt.cpu().tolist() == [[n] * H for n in want.cnt] and list(got.lens) == want.cnt and got.dims == (len(parts), max(want.cnt), H, d, m)
    assert bool((A[:, :, m:] == 0).all()) and bool((a[:, :, m:] == 0).all())
    for t, row in enumerate(parts):
        if not row:
            assert not bool(A[t].any()) and not bool(a[t].any()) and not bool(vs[t].any())
    return got, want, lib


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("T,H,d,m", SHAPES)
def test_states_with_different_stabilisers_against_float64(gpulib, T, H, d, m, kind):
    tasks, parts = _tables(T)["p2"]
    _check(gpulib, kind, tasks, parts, H, d, m, label="p2")


@pytest.mark.parametrize("name", ["p1", "p8", "fresh_source", "empty_task", "one_and_five_into_three"])
@pytest.mark.parametrize("T,H,d,m", SHAPES)
def test_tables_against_float64(gpulib, T, H, d, m, name):
    tasks, parts = _tables(T)[name]
    for kind in ("live", "peak_last"):
        _check(gpulib, kind, tasks, parts, H, d, m, label=name)


def test_the_large_shape_against_float64(gpulib):
    T, H, d, m = BIG
    tasks, parts = _tables(T)["p2"]
    _check(gpulib, "peak_last", tasks, parts, H, d, m, label="p2")


@pytest.mark.parametrize("T,H,d,m", SHAPES)
def test_a_floor_above_every_stabiliser_and_the_query(gpulib, T, H, d, m):
    from mlhot.ops import favor_query
    tasks, parts = _tables(T)["p2"]
    lib, states = G.library("live", tasks, H, d, m), _states("live", tasks, H, d, m)
    top = max(s.summary()[4].item() for s in states)
    q = G.queries(T, H, d)
    for floor in (None, top + 3.0):
        got, want, _ = _check(gpulib, "live", tasks, parts, H, d, m, floor=floor, label=f"floor {floor}")
        out = favor_query(_dev(q), got, None, lib[0].proj.to(DEV))
        ref = R.merged(want.query(q, lib[0].proj))
        err = U.rel_err(out, ref)
        print(f"favor_query through a gathered state H={H} d={d} m={m} floor {floor}: {err:.2e} of out's scale")
        assert out.shape == ref.shape and bool(torch.isfinite(out).all()) and err <= U.RTOL


# ---- 3. an input's paddings are never trusted -----------------------------------------------------------------------------------------------
def test_poisoned_paddings_of_the_sources_give_clean_output(gpulib):
    from mlhot.ops import FavorKeyState
    T, H, d, m = SHAPES[1]
    tasks, parts = _tables(T)["p2"]
    states = _states("live", tasks, H, d, m)
    clean = _raw(gpulib, states, parts)
    poisoned = []
    for s in states:
        buf = s.buf.clone()
        A, a, vs, cnt, M = gpulib.favor_summary_views(buf, T, H, d, m)
        A[:, :, m:] = float("nan")
        a[:, :, m:] = float("nan")
        f, at = buf.view(torch.float32), _m_at(T, H, d, m)
        f[at + 1:at + 16] = float("nan")                                                # the rest of M's block
        f[at + 16 + T * H:] = float("nan")                                              # cnt's padding
        poisoned.append(FavorKeyState("summary", s.dims, buf=buf, lens=s.lens))
    assert m % 16 and (T * H) % 16
    got = _raw(gpulib, poisoned, parts)
    assert torch.equal(got, clean) and not bool(torch.isnan(got.view(torch.float32)).any())


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_as_it_was(gpulib, monkeypatch):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_gather
    c = gpulib.c
    T, H, d, m = SHAPES[1]
    nb = gpulib.favor_summary_bytes(T, H, d, m)
    states = [torch.full((nb // 4,), 3.0, device=DEV) for _ in range(9)]
    out = torch.full((nb // 4,), 7.0, device=DEV)
    parts = torch.zeros(T, 1, 2, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    table = lambda ts: (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
    counts = lambda n, T=T: (C.c_int * max(n, 1))(*[T] * n)
    call = lambda ts, n, P, d=d, m=m, nb=nb, cnt=None: c.mlhot_favor_summary_gather(table(ts), cnt or counts(n), n, p(parts), P, None, T, H, d, m, p(out), nb, None)
    ARG, UNSUPPORTED = 1, 4                                                              # MLHOT_ERR_* (csrc/common.h)
    codes = {
        "out is input 1": (call([states[0], out, states[1]], 3, 1), ARG),
        "out overlaps input 0": (call([out[4:]], 1, 1), ARG),
        "n = 0": (call([], 0, 1), ARG),
        "n = 9": (call(states, 9, 1), ARG),
        "P = 0": (call(states[:2], 2, 0), ARG),
        "P = 9": (call(states[:2], 2, 9), ARG),
        "state_bytes too large": (call(states[:2], 2, 1, nb=nb + 16), ARG),
        "state_bytes too small": (call(states[:2], 2, 1, nb=nb - 16), ARG),
        "d = 24": (call(states[:2], 2, 1, d=24, m=32), UNSUPPORTED),
        "m = 1537": (call(states[:2], 2, 1, d=16, m=1537), UNSUPPORTED),
        "T_i = 2^20": (call(states[:2], 2, 1, cnt=(C.c_int * 2)(T, 1 << 20)), UNSUPPORTED),
    }
    torch.cuda.synchronize()
    for what, (got, want) in codes.items():
        assert got == want, (what, got, want)
    assert bool((out == 7.0).all()) and all(bool((s == 3.0).all()) for s in states)
    u8 = [s.view(torch.uint8) for s in states]
    with pytest.raises(MlhotError, match="out overlaps input state 0"):                   # an out that aliases an input
        gpulib.favor_summary_gather(u8[:2], [T, T], parts, H, d, m, out=u8[0])
    with pytest.raises(MlhotError, match="takes 1 .. 8 states per call"):
        gpulib.favor_summary_gather(u8, [T] * 9, parts, H, d, m)
    torch.cuda.synchronize()
    assert all(bool((s == 3.0).all()) for s in states)
    # out-of-range and over-long tables: refused on the host, before any launch
    a, b = _states("live", (T, T), H, d, m)
    monkeypatch.setattr(gpulib, "favor_summary_gather", lambda *a, **kw: pytest.fail("a refused table reached the launch"))
    for bad, match in (([[(2, 0)]], "names state 2"), ([[(0, T)]], f"names task {T} of states"), ([[(0, -1)]], "names task -1"),
                       ([[(0, 0)] * 9], "names 9 parts")):
        with pytest.raises(ValueError, match=match):
            favor_gather([a, b], bad)
