"""mlhot.ops.favor_merge / mlhot_favor_summary_merge on the MI355X (csrc/favor_summary.h): parts absorbed apart and
merged against the float64 stream over the whole case, the query through a merged state, the identities bit for bit, what is written
and what is not, the n edges and the refusals.  The bar is tests/test_favor_summary_gpu.py's: U.RTOL of each quantity's scale.
Run with -m gpu."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import favor_cached_ref as R
from tests import favor_merge_ref as MR
from tests import favor_summary_ref as S
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = S.H
MULTI = [n for n, calls in S.CHUNKINGS.items() if len(calls) > 1]


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _absorb(c, calls):
    """favor_absorb over some of the case's calls, from a fresh state (tests/test_favor_summary_gpu.py's _absorb)."""
    from mlhot.ops import favor_absorb
    state, pd = None, c["proj"].to(DEV)
    for kc, vc, lens in calls:
        n = kc.shape[2]
        state = favor_absorb(state, _dev(kc), _dev(vc), pd, lens=None if all(L == n for L in lens) else lens)
    return state


def _parts(c, split):
    return [_absorb(c, calls) for calls in MR.groups(c, split)]


def _fields(state):
    """Every defined field of a summary state - A, a, vs, cnt, M - as one int32 vector (bit equality, NaN-proof).  The rest of M's block
    of 16 and cnt's padding are not part of it: favor_absorb into a new buffer leaves them unwritten."""
    return torch.cat([x.reshape(-1).view(torch.int32) for x in state.summary()])


def _state_errors(state, want, m):
    A, a, vs, cnt, M = state.summary()
    return U.rel_err(A[:, :, :m], want.A), U.rel_err(a[:, :, :m], want.a), U.rel_err(vs, want.vs)


@functools.lru_cache(maxsize=None)
def _whole(kind, d, m, chunking):
    c = S.case(kind, d, m, chunking)
    return _absorb(c, c["chunks"])


# ---- 1. the merged state against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", MR.SPLITS)
@pytest.mark.parametrize("kind", ["live", "peak_last", "peak_first_t0"])
@pytest.mark.parametrize("chunking", MULTI)
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_state_against_float64(gpulib, d, m, chunking, kind, split):
    from mlhot.ops import favor_merge
    c = S.case(kind, d, m, chunking)
    T, mp = c["T"], (m + 15) // 16 * 16
    parts = _parts(c, split)
    before = [_fields(p).clone() for p in parts]
    merged = favor_merge(parts)
    want = S.streamed(c)
    A, a, vs, cnt, M = merged.summary()
    assert A.shape == (T, H, mp, d) and merged.route == "summary"
    errs = _state_errors(merged, want, m)
    chain = _state_errors(_whole(kind, d, m, chunking), want, m)
    print(f"merge {split} {kind} d={d} m={m} {chunking}: A {errs[0]:.2e}, a {errs[1]:.2e}, vs {errs[2]:.2e} of their scales; "
          f"the absorb chain on the same case: A {chain[0]:.2e}, a {chain[1]:.2e}, vs {chain[2]:.2e}")
    assert max(errs) <= U.RTOL
    assert M.item() == max(p.summary()[4].item() for p in parts)                       # the maximum of the parts' stabilisers, exactly
    assert cnt.cpu().tolist() == [[n] * H for n in c["totals"]] and list(merged.lens) == c["totals"] and merged.dims == (T, max(c["totals"]), H, d, m)
    assert [sum(p.lens[t] for p in parts) for t in range(T)] == c["totals"]
    assert bool((A[:, :, m:] == 0).all()) and bool((a[:, :, m:] == 0).all())            # features >= m are exactly zero
    for p, b in zip(parts, before):
        assert torch.equal(_fields(p), b)                                           # the inputs stay as they were


# ---- 2. the query through a merged state -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("chunking", ["7_32_31", "ragged"])
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_query_through_a_merged_state(gpulib, d, m, chunking, kind):
    from mlhot.ops import favor_merge, favor_query
    c = S.case(kind, d, m, chunking)
    want = R.merged(S.reference(c))
    merged = favor_merge(_parts(c, "per_call"))
    qd, pd = _dev(c["q"]), c["proj"].to(DEV)
    got = favor_query(qd, merged, None, pd)
    err, chain = U.rel_err(got, want), U.rel_err(favor_query(qd, _whole(kind, d, m, chunking), None, pd), want)
    line = f"favor_query through a merged state {kind} d={d} m={m} {chunking}: {err:.2e} of out's scale; through the absorb chain {chain:.2e}"
    print(line)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL, line


# ---- 3. identities, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_identities_bit_for_bit(gpulib, d, m):
    from mlhot.ops import FavorKeyState, favor_absorb, favor_merge, favor_query
    c = S.case("live", d, m, "7_32_31")
    T = c["T"]
    s = _whole("live", d, m, "7_32_31")
    qd, pd = _dev(c["q"]), c["proj"].to(DEV)
    assert torch.equal(_fields(favor_merge([s])), _fields(s))
    kc, vc, _ = c["chunks"][0]
    by_absorb = favor_absorb(None, _dev(kc), _dev(vc), pd, lens=[0] * T)
    by_init = FavorKeyState("summary", (T, 0, H, d, m), buf=gpulib.favor_summary_init(T, H, d, m, DEV), lens=(0,) * T)
    for fresh in (by_absorb, by_init):
        assert fresh.summary()[4].item() == -math.inf
        for order in ([s, fresh], [fresh, s], [fresh, s, fresh]):
            got = favor_merge(order)
            assert torch.equal(_fields(got), _fields(s)) and got.lens == s.lens and got.dims == s.dims
    none = favor_merge([by_init, by_absorb])                                        # -inf against -inf: no exp(-inf - -inf)
    assert torch.equal(_fields(none), _fields(by_init)) and none.lens == (0,) * T
    parts = _parts(c, "per_call")
    once, again = favor_merge(parts), favor_merge(parts)
    assert torch.equal(_fields(once), _fields(again))
    Ms = [p.summary()[4].item() for p in parts]
    low = torch.tensor([min(Ms) - 1.0], device=DEV)
    assert torch.equal(_fields(favor_merge(parts, floor=low)), _fields(once))       # a floor below every M changes nothing
    assert torch.equal(_fields(favor_merge(parts, floor=torch.tensor([-math.inf], device=DEV))), _fields(once))
    # a floor above every M: M' == floor, A and a take the common factor exp(max M - floor), vs and cnt none.  The quotient of
    # favor_query cancels that factor up to its eps terms - the key feature's +eps is relative to the stabiliser, so raising it by
    # delta weighs the eps terms exp(delta) times more.  At delta = 1 / 64 the float64 result moves by <= 2.4e-5 of out's scale on
    # these inputs (tests/test_favor_merge_cpu.py holds the d = 16 figure), a quarter of the bar; against the float64 state WITH the
    # floor the bar holds at any delta, here 3.
    base = favor_query(qd, once, None, pd)
    for delta in (2.0 ** -6, 3.0):
        fl = torch.tensor([max(Ms) + delta], device=DEV)
        up = favor_merge(parts, floor=fl)
        A, a, vs, cnt, M = up.summary()
        assert M.item() == fl.item() and torch.equal(vs, once.summary()[2]) and torch.equal(cnt, once.summary()[3])
        want = MR.merge([MR.part(c, calls) for calls in MR.groups(c, "per_call")], floor=fl.item())
        got = favor_query(qd, up, None, pd)
        err = U.rel_err(got, R.merged(want.query(c["q"], c["proj"])))
        moved = U.rel_err(got, base)
        print(f"floor {delta} above M d={d} m={m}: state A {U.rel_err(A[:, :, :m], want.A):.2e}, query against float64 with the floor {err:.2e}, "
              f"against the unfloored query {moved:.2e}")
        assert U.rel_err(A[:, :, :m], want.A) <= U.RTOL and U.rel_err(a[:, :, :m], want.a) <= U.RTOL and err <= U.RTOL
        if delta < 1:
            assert moved <= U.RTOL


# ---- 4. everything is written, nothing else is touched -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_every_field_is_written_and_nothing_else(gpulib, d, m, n):
    c = S.case("live", d, m, "7_32_31")
    T = c["T"]
    parts = _parts(c, "per_call")[:n]
    nb = gpulib.favor_summary_bytes(T, H, d, m)
    guard = 4096
    big = torch.full(((nb + guard) // 4,), float("nan"), device=DEV)                 # out and a guard region behind state_bytes
    before = [p.buf.clone() for p in parts]
    out = gpulib.favor_summary_merge([p.buf for p in parts], T, H, d, m, out=big.view(torch.uint8))
    assert out.data_ptr() == big.data_ptr()
    A, a, vs, cnt, M = gpulib.favor_summary_views(out, T, H, d, m)
    for x in (A, a, vs, M):
        assert bool(torch.isfinite(x).all())
    assert bool((A[:, :, m:] == 0).all()) and bool((a[:, :, m:] == 0).all())
    assert cnt.cpu().tolist() == [[sum(p.lens[t] for p in parts)] * H for t in range(T)]
    words = big.view(torch.int32)
    at = (A.numel() + a.numel() + vs.numel())
    assert not bool(words[at + 1:at + 16].any()) and not bool(words[at + 16 + T * H:nb // 4].any())      # M's block and cnt's padding: zeros
    assert bool(torch.isnan(big[nb // 4:]).all())                                    # the guard is as it was
    fresh = gpulib.favor_summary_merge([p.buf for p in parts], T, H, d, m)
    assert torch.equal(fresh.view(torch.int32), words[:nb // 4])                     # what out held before does not matter
    for p, b in zip(parts, before):
        assert torch.equal(p.buf, b)


# ---- 5. the n edges ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _singles(n, d=64, m=266):
    """n one-shot states of (64, 266), the dominating key in the LAST one, and the float64 state of all n shots."""
    from mlhot.ops import favor_absorb
    T = 2
    g = torch.Generator().manual_seed(31 + n)
    proj = S.proj_for(d, m)
    k, v = 0.25 * torch.randn(T, H, n, d, generator=g), torch.randn(T, H, n, d, generator=g)
    k[1, 0, n - 1] = proj[m // 2] * (20.0 / (d ** -0.25 * float(proj[m // 2] @ proj[m // 2])))
    q = 0.25 * torch.randn(T, H, 7, d, generator=g)
    pd = proj.to(DEV)
    states = [favor_absorb(None, _dev(k[:, :, i:i + 1]), _dev(v[:, :, i:i + 1]), pd) for i in range(n)]
    return states, S.State(T, H, d, m).absorb(k, v, proj), q, k, v, proj


@pytest.mark.parametrize("n", [8, 9])
def test_eight_states_in_one_launch_and_nine_through_the_fold(gpulib, n, monkeypatch):
    from mlhot.ops import favor_merge, favor_query
    states, want, q, k, v, proj = _singles(n)
    calls = []
    real = gpulib.favor_summary_merge
    monkeypatch.setattr(gpulib, "favor_summary_merge", lambda bufs, *a, **kw: (calls.append(len(bufs)), real(bufs, *a, **kw))[1])
    merged = favor_merge(states)
    assert calls == ([8] if n == 8 else [8, 2])
    errs = _state_errors(merged, want, 266)
    got = favor_query(_dev(q), merged, None, proj.to(DEV))
    err = U.rel_err(got, R.merged(R.attention(q, k, v, proj)))
    print(f"merge of {n} one-shot states d=64 m=266: A {errs[0]:.2e}, a {errs[1]:.2e}, vs {errs[2]:.2e} of their scales, favor_query {err:.2e}")
    assert max(errs) <= U.RTOL and err <= U.RTOL
    assert merged.lens == (n, n) and merged.summary()[3].cpu().tolist() == [[n] * H] * 2
    assert merged.summary()[4].item() == max(s.summary()[4].item() for s in states)


# ---- 6. refusals on the device side --------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_as_it_was(gpulib):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_merge
    c = gpulib.c
    T, d, m = 2, 64, 266
    nb = gpulib.favor_summary_bytes(T, H, d, m)
    states = [torch.full((nb // 4,), 3.0, device=DEV) for _ in range(9)]
    out = torch.full((nb // 4,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    table = lambda ts: (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
    ARG, WORKSPACE, UNSUPPORTED = 1, 2, 4                                             # MLHOT_ERR_* (csrc/common.h)
    codes = {
        "out is input 1": (c.mlhot_favor_summary_merge(table([states[0], out, states[1]]), 3, None, T, H, d, m, p(out), nb, None), ARG),
        "out overlaps input 0": (c.mlhot_favor_summary_merge(table([out[4:]]), 1, None, T, H, d, m, p(out), nb, None), ARG),
        "n = 0": (c.mlhot_favor_summary_merge(table([]), 0, None, T, H, d, m, p(out), nb, None), UNSUPPORTED),
        "n = 9": (c.mlhot_favor_summary_merge(table(states), 9, None, T, H, d, m, p(out), nb, None), UNSUPPORTED),
        "d = 24": (c.mlhot_favor_summary_merge(table(states[:2]), 2, None, T, H, 24, 32, p(out), nb, None), UNSUPPORTED),
        "m = 1537": (c.mlhot_favor_summary_merge(table(states[:2]), 2, None, T, H, 16, 1537, p(out), nb, None), UNSUPPORTED),
        "state_bytes too large": (c.mlhot_favor_summary_merge(table(states[:2]), 2, None, T, H, d, m, p(out), nb + 16, None), WORKSPACE),
        "state_bytes too small": (c.mlhot_favor_summary_merge(table(states[:2]), 2, None, T, H, d, m, p(out), nb - 16, None), WORKSPACE),
    }
    torch.cuda.synchronize()
    for what, (got, want) in codes.items():
        assert got == want, (what, got, want)
    assert bool((out == 7.0).all()) and all(bool((s == 3.0).all()) for s in states)
    u8 = [s.view(torch.uint8) for s in states]
    with pytest.raises(MlhotError, match="out overlaps input state 0"):
        gpulib.favor_summary_merge(u8[:2], T, H, d, m, out=u8[0])
    with pytest.raises(MlhotError, match="takes 1 .. 8 states per call"):
        gpulib.favor_summary_merge(u8, T, H, d, m)
    assert all(bool((s == 3.0).all()) for s in states)
    g = torch.Generator().manual_seed(3)
    k = 0.25 * torch.randn(2, 4, H, 16, generator=g).to(DEV)
    from mlhot.ops import favor_absorb
    with pytest.raises(MlhotError, match=r"states\[1\] was built for"):
        favor_merge([favor_absorb(None, k, k, torch.randn(16, 16, generator=g).to(DEV)), favor_absorb(None, k, k, torch.randn(32, 16, generator=g).to(DEV))])
