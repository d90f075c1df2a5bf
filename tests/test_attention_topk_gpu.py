"""The top-k attention read-out on the MI355X: mlhot_favor_query_topk_fwd / _long_topk_fwd / _paged_topk_fwd through
mlhot.ops.favor_query(topk=) on random kh / vh / qh, no encoder.  Cases: tests/attention_topk_cases.py; the statement of the
definition: tests/attention_topk_ref.py.  Run with -m gpu.

Values are compared, indices only through the gather: the kernels rank the un-normalised S, and where two different S round to one
w a top-k over w may name the other slot.  Against float64 the bar is the read-out's own (tests/test_attention_readout_gpu.py:
U.rel_err <= U.RTOL), for wk against the float64 weight at idx and against the float64 j-th largest weight.

The keys entry (Nc <= 32) takes no lens: a ragged state's slots behind lens[t] are zero rows of F_k, and v is read there as
mlhot_favor_query_fwd reads it - poison goes into k alone, v is zero-filled.  The long and paged entries never read either."""
import functools

import pytest
import torch

from tests import attention_topk_cases as TC
from tests import attention_topk_ref as TR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H, D = TC.T, TC.H, TC.D
KEYS = {"cached": "favor_keys", "long": "favor_keys_long", "paged": "favor_keys_paged"}
LABEL = {"cached": "favor.querytopk", "long": "favor.lquerytopk", "paged": "favor.pquerytopk"}


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _state(form, k, p, lens, cap=None):
    """The key state of `form` on k [T, H, Nc, d] (CPU), optionally kept in `cap` slots"""
    from mlhot import ops
    kd = _dev(k)
    if cap is not None and cap > kd.shape[1]:
        kd = torch.cat([kd, torch.full((T, cap - kd.shape[1], H, D), float("nan"), device=DEV)], dim=1)
        lens = lens if lens is not None else (k.shape[2],) * T
    state = getattr(ops, KEYS[form])(kd, p.to(DEV), lens=lens)
    assert state.route == form
    return state


def _v(form, v, lens, cap=None):
    vd = _dev(TC.poisoned(v, lens, 0.0 if form == "cached" else float("nan")))
    if cap is not None and cap > vd.shape[1]:
        vd = torch.cat([vd, torch.full((T, cap - vd.shape[1], H, D), 0.0 if form == "cached" else float("nan"), device=DEV)], dim=1)
    return vd


@functools.lru_cache(maxsize=None)
def _setup(form, Nc, m, lens, cap=None):
    q, k, v, p, _ = TC.inputs(Nc, m)
    return _dev(q), _state(form, TC.poisoned(k, lens, float("nan")), p, lens, cap), _v(form, v, lens, cap), p.to(DEV)


@functools.lru_cache(maxsize=None)
def _w64(Nc, m, lens):
    q, k, _, p, _ = TC.inputs(Nc, m)
    from tests import attention_readout_ref as AR
    return AR.weights(q, k, p, lens)


def _check(gpulib, name, form, Nc, m, lens, cap=None):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup(form, Nc, m, lens, cap)
    slots = cap or Nc
    eff = lens if lens is not None or cap is None else (Nc,) * T
    w64 = _w64(Nc, m, lens)
    if cap:
        w64 = torch.cat([w64, torch.zeros(T, H, TC.NQ, cap - Nc, dtype=w64.dtype)], dim=-1)
    counts = TR.valid_counts(eff, T, slots)
    full = {kk: favor_query(qd, state, vd, pd, topk=kk) for kk in TC.KS}
    for Nq in TC.NQS:
        rows = qd[:, :Nq].contiguous()
        plain = favor_query(rows, state, vd, pd)
        out_w, w = favor_query(rows, state, vd, pd, weights=True)
        assert bool(torch.isfinite(plain).all()) and torch.equal(out_w, plain)
        for kk in TC.KS:
            labels, (out, idx, wk) = U.launch_labels(gpulib, lambda: favor_query(rows, state, vd, pd, topk=kk))
            assert labels == [LABEL[form]], labels
            assert idx.shape == (T, H, Nq, kk) and idx.is_contiguous() and wk.is_contiguous()
            assert torch.equal(out, plain), (Nq, kk)
            TR.check_shape_rules(idx, wk, eff, slots, kk)                           # NaN behind lens reaches nothing: wk > 0, finite
            assert torch.equal(wk, TR.gather_at(w, idx)), (Nq, kk)                  # the read-out's bits at idx
            for t, n in enumerate(counts):                                          # the VALUES of a top-k over w
                j = min(kk, n)
                assert torch.equal(wk[t, :, :, :j], torch.topk(w[t, :, :, :n], j, dim=-1).values), (Nq, kk, t)
            # the first Nq rows alone give the bits they have among all rows
            assert torch.equal(idx, full[kk][1][:, :, :Nq]) and torch.equal(wk, full[kk][2][:, :, :Nq]) and torch.equal(out, full[kk][0][:, :Nq])
            at = TR.gather_at(w64[:, :, :Nq], idx.cpu().long())
            jth = TR.topk_of(w64[:, :, :Nq], eff, kk)[1]
            e_at, e_jth = U.rel_err(wk, at), U.rel_err(wk, jth)
            line = f"attention top-k {name} Nq={Nq} k={kk}: against the float64 weight at idx {e_at:.2e}, against the float64 j-th largest {e_jth:.2e}"
            print(line)
            assert e_at <= U.RTOL and e_jth <= U.RTOL, line


@pytest.mark.parametrize("form,Nc,m,lens", TC.CASES, ids=[TC.case_id(c) for c in TC.CASES])
def test_topk_per_case(gpulib, form, Nc, m, lens):
    """out bit-equal to the plain entry; wk bit-equal to the read-out's w at idx and to torch.topk's values over the valid slots; idx
    distinct and valid, the padding exact; within U.RTOL of float64 both ways; row-invariant; NaN in the invalid rows of k (and v:
    long, paged) reaches nothing."""
    _check(gpulib, TC.case_id((form, Nc, m, lens)), form, Nc, m, lens)


def test_topk_513_shots_kept_in_1024_slots(gpulib):
    """The wide case, and capacity invariance: the same shots in 513 and in 1024 slots give the same bits."""
    from mlhot.ops import favor_query
    form, Nc, m, lens, cap = TC.WIDE
    _check(gpulib, f"{form}-{Nc}in{cap}-m{m}", form, Nc, m, lens, cap)
    a_set, b_set = _setup(form, Nc, m, lens), _setup(form, Nc, m, lens, cap)
    for kk in TC.KS:
        a, b = favor_query(*a_set, topk=kk), favor_query(*b_set, topk=kk)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kk


@pytest.mark.parametrize("form,Nc,cap", [("long", 40, 200), ("paged", 40, 300), ("paged", 300, 600)])
def test_same_shots_at_another_capacity_give_the_same_bits(gpulib, form, Nc, cap):
    from mlhot.ops import favor_query
    m, lens = 40, (Nc - 3, Nc)
    for kk in TC.KS:
        a, b = favor_query(*_setup(form, Nc, m, lens), topk=kk), favor_query(*_setup(form, Nc, m, lens, cap), topk=kk)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kk


@pytest.mark.parametrize("Nc", [1, 31, 32, 33, 255, 256])
def test_smaller_states_give_the_smaller_forms_bits(gpulib, Nc):
    """A paged state of at most 256 slots gives the long entry's bits, a long state of at most 32 the keys entry's."""
    from mlhot.ops import favor_query
    m = 40
    q, k, v, p, _ = TC.inputs(Nc, m)
    qd, vd, pd = _dev(q), _dev(v), p.to(DEV)
    for kk in TC.KS:
        res = {form: favor_query(qd, _state(form, k, p, None), vd, pd, topk=kk) for form in (("cached", "long", "paged") if Nc <= 32 else ("long", "paged"))}
        for form in res:
            assert all(torch.equal(x, y) for x, y in zip(res[form], res["long"])), (form, kk)


@pytest.mark.parametrize("form,Nc,twins", [("cached", 32, (5, 9)), ("long", 64, (5, 9, 40)), ("paged", 513, (5, 9, 40, 300))])
def test_equal_scores_rank_by_slot(gpulib, form, Nc, twins):
    """Identical key rows planted inside one 32-slot chunk (5, 9), across chunks of one page (5, 40) and across pages (5, 300):
    copies of query row 0 among keys scaled to a fifth, so that they lead that row - in float64 by a factor of at least 1.12 over
    the best other slot at these inputs (FAVOR+'s weight falls with |k|^2 / 2, a LONGER copy would lose).  Identical rows at
    different columns must give identical S bits; the twins then stand first in row 0's ranking, lower slot first, with one weight."""
    from mlhot.ops import favor_query
    m = 40
    q, k, v, p, _ = TC.inputs(Nc, m)
    k = 0.2 * k
    for c in twins:
        k[:, :, c] = q[:, :, 0]
    qd, state, vd, pd = _dev(q), _state(form, k, p, None), _dev(v), p.to(DEV)
    _, w = favor_query(qd, state, vd, pd, weights=True)
    for c in twins[1:]:
        assert torch.equal(w[:, :, 0, c], w[:, :, 0, twins[0]]), f"slots {twins[0]} and {c} hold one key row but S differs"
    for kk in (len(twins), 16):
        _, idx, wk = favor_query(qd, state, vd, pd, topk=kk)
        assert torch.equal(wk, TR.gather_at(w, idx))
        head = idx[:, :, 0, :len(twins)].cpu()
        assert bool((head == torch.tensor(twins, dtype=torch.int32)).all()), head.tolist()
        assert bool((wk[:, :, 0, :len(twins)] == wk[:, :, 0, :1]).all())
    _, idx1, _ = favor_query(qd, state, vd, pd, topk=1)
    assert bool((idx1[:, :, 0, 0] == twins[0]).all())


def test_bad_arguments_and_unsupported_shapes_write_nothing(gpulib):
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    q, v, proj = torch.zeros(1, 4, 2, 16, device=DEV), torch.zeros(1, 40, 2, 16, device=DEV), torch.zeros(16, 16, device=DEV)
    state, ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    out, idx, wk = torch.full((1, 4, 32), 7.0, device=DEV), torch.full((1, 2, 4, 3), 7, dtype=torch.int32, device=DEV), torch.full((1, 2, 4, 3), 7.0, device=DEV)
    c = gpulib.c
    rc = c.mlhot_favor_query_topk_fwd(p(q), p(state), p(v), p(proj), 1, 2, 4, 40, 16, 16, p(out), 3, p(idx), p(wk), p(ws), ws.numel(), None)
    assert rc != 0 and b"Nc <= 32" in c.mlhot_last_error()                         # MLHOT_ERR_UNSUPPORTED
    rc = c.mlhot_favor_query_long_topk_fwd(p(q), p(state), p(v), p(proj), None, 1, 2, 4, 300, 16, 16, p(out), 3, p(idx), p(wk), p(ws), ws.numel(), None)
    assert rc != 0 and b"Nc <= 256" in c.mlhot_last_error()
    rc = c.mlhot_favor_query_paged_topk_fwd(p(q), p(state), p(v), p(proj), None, 1, 2, 4, 5000, 16, 16, p(out), 3, p(idx), p(wk), p(ws), ws.numel(), None)
    assert rc != 0 and b"Nc <= 4096" in c.mlhot_last_error()
    for k, i, w_ in ((0, p(idx), p(wk)), (17, p(idx), p(wk)), (3, None, p(wk)), (3, p(idx), None)):
        rc = c.mlhot_favor_query_long_topk_fwd(p(q), p(state), p(v), p(proj), None, 1, 2, 4, 40, 16, 16, p(out), k, i, w_, p(ws), ws.numel(), None)
        assert rc != 0 and b"bad argument" in c.mlhot_last_error(), k                # MLHOT_ERR_ARG
    rc = c.mlhot_favor_query_long_topk_fwd(p(q), p(state), p(v), p(proj), None, 1, 2, 4, 40, 16, 16, p(out), 3, p(idx), p(wk), p(ws), 16, None)
    assert rc != 0 and b"workspace too small" in c.mlhot_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((idx == 7).all()) and bool((wk == 7.0).all())


def test_peak_memory_stays_far_below_w(gpulib):
    """T = 2, H = 8, Nq = 512, Nc = 4096, d = m = 16: w would be 128 MiB; the call's peak stays below a quarter of that - the bar of
    tests/test_attention_mass_gpu.py.  This path writes only out, idx and wk (1 MiB together)."""
    from mlhot.ops import favor_keys_paged, favor_query
    Tn, Hn, Nq, Nc, d, m, kk = 2, 8, 512, 4096, 16, 16, 8
    g = torch.Generator().manual_seed(11)
    qd = (0.5 * torch.randn(Tn, Nq, Hn, d, generator=g)).to(DEV)
    kd = (0.5 * torch.randn(Tn, Nc, Hn, d, generator=g)).to(DEV)
    vd = torch.randn(Tn, Nc, Hn, d, generator=g).to(DEV)
    pd = TC.proj(m).to(DEV)
    state = favor_keys_paged(kd, pd)
    w_bytes = Tn * Hn * Nq * Nc * 4
    assert w_bytes == 128 << 20
    plain = favor_query(qd, state, vd, pd)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, idx, wk = favor_query(qd, state, vd, pd, topk=kk)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"attention top-k memory: peak over the call {peak / 2 ** 20:.2f} MiB, w would be {w_bytes / 2 ** 20:.0f} MiB")
    operands = sum(t.numel() * t.element_size() for t in (qd, kd, vd, pd, state.buf, plain))
    assert operands + peak < w_bytes // 4
    assert peak <= 2 * (out.numel() + idx.numel() + wk.numel()) * 4 + (1 << 20)    # out, idx, wk and the token block, with allocator rounding
    assert torch.equal(out, plain)
    TR.check_shape_rules(idx, wk, None, Nc, kk)
    del out, idx, wk
    _, w = favor_query(qd[:, :64].contiguous(), state, vd, pd, weights=True)      # 16 MiB of w: the first 64 rows against torch.topk
    _, idx, wk = favor_query(qd[:, :64].contiguous(), state, vd, pd, topk=kk)
    assert torch.equal(wk, torch.topk(w, kk, dim=-1).values) and torch.equal(wk, TR.gather_at(w, idx))
