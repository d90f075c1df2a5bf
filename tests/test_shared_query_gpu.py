"""The shared-target query on the MI355X: mlhot_favor_query_shared_fwd / _long_shared_fwd through
mlhot.ops.favor_query(shared=True) on random kh / vh / qh, no encoder.  One set of query rows q [Nq, H, d] against T stored contexts:
out and w bit-equal to the per-task entries on the expanded query, whatever the task group; against float64 within the per-task
tests' own bars (tests/test_attention_readout_gpu.py, tests/test_favor_long_gpu.py: U.RTOL for values, AC.rowsum_bound for the row
sum of w); row invariance; exact zeros behind lens[t]; poison behind lens[t] reaches nothing; the envelope; the refusals.  Cases and
the float64 reference: tests/shared_query_cases.py.  Run with -m gpu."""
import ctypes as C
import functools

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import favor_cached_ref as R
from tests import shared_query_cases as SC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = SC.H
LABEL = {("cached", False): "favor.querys", ("cached", True): "favor.querysw", ("long", False): "favor.lquerys", ("long", True): "favor.lquerysw"}


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _rowsum_excess(w):
    return float((w.double().sum(dim=-1) - 1.0).abs().max())


@functools.lru_cache(maxsize=None)
def _setup(form, T, Nc, d, m, lens, poison=None):
    """(q [NQ, H, d] on the device, the key state, v [T, Nc, H, d], proj)"""
    from mlhot import ops
    q, kn, vp, p = SC.operands(form, T, Nc, d, m, lens, poison)
    pd = p.to(DEV)
    keys = ops.favor_keys if form == "cached" else ops.favor_keys_long
    state = keys(_dev(kn), pd, lens=None if lens is None else list(lens))
    assert state.route == form and state.dims == (T, Nc, H, d, m)
    return q.permute(1, 0, 2).contiguous().to(DEV), state, _dev(vp), pd


def _groups(T):
    return [T if g == "T" else g for g in SC.TASK_GROUPS]


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_shared_query_per_case(gpulib, case):
    """1. bits of the per-task entry on the expanded query; 2. float64; 3. every task group; 4. row invariance; 5. zeros behind lens[t]
    and rows of w that sum to 1."""
    from mlhot.ops import favor_query
    form, T, Nc, d, m, lens, nq = case
    qd, state, vd, pd = _setup(form, T, Nc, d, m, lens)
    qd = qd[:nq].contiguous()
    w64, out64 = SC.want(form, T, Nc, d, m, lens)
    # the whole call, on the parent's own path: the query rows expanded to every task
    qe = qd[None].expand(T, nq, H, d).contiguous()
    want_out, want_w = favor_query(qe, state, vd, pd, weights=True)
    assert torch.equal(favor_query(qe, state, vd, pd), want_out)
    labels, (out, w) = U.launch_labels(gpulib, lambda: favor_query(qd, state, vd, pd, weights=True, shared=True))
    assert labels == [LABEL[form, True]], labels                                        # ONE launch for all tasks
    assert out.shape == (T, nq, d * H) and w.shape == (T, H, nq, Nc) and out.is_contiguous() and w.is_contiguous()
    assert torch.equal(out, want_out) and torch.equal(w, want_w)                        # 1.
    labels, plain = U.launch_labels(gpulib, lambda: favor_query(qd, state, vd, pd, shared=True))
    assert labels == [LABEL[form, False]] and torch.equal(plain, want_out)              # w == NULL: no read-out, the same out
    for g in _groups(T):                                                                # 3.
        og, wg = favor_query(qd, state, vd, pd, weights=True, shared=True, task_group=g)
        assert torch.equal(og, want_out) and torch.equal(wg, want_w), g
        assert torch.equal(favor_query(qd, state, vd, pd, shared=True, task_group=g), want_out), g
    eo, ew, excess = U.rel_err(out, R.merged(out64[:, :, :nq])), U.rel_err(w, w64[:, :, :nq]), _rowsum_excess(w)
    line = (f"favor_query shared {SC.case_id(case)} Nq={nq}: out {eo:.2e}, w {ew:.2e} of their scales, |sum_n w - 1| {excess:.2e} "
            f"({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
    print(line)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0, line
    assert eo <= U.RTOL and ew <= U.RTOL, line                                          # 2.
    assert excess <= AC.rowsum_bound(Nc), line                                          # 5.
    if lens is not None:
        for t, L in enumerate(lens):
            assert bool((w[t, :, :, L:] == 0.0).all()) and float(w[t, :, :, :L].min()) > 0.0, (lens, t)
            assert U.rel_err(w[t, :, :, :L], w64[t, :, :nq, :L]) <= U.RTOL and U.rel_err(out[t], R.merged(out64[:, :, :nq])[t]) <= U.RTOL
    for n in [x for x in SC.NQS if x < nq]:                                             # the first n rows alone, every tile edge
        on, wn = favor_query(qd[:n].contiguous(), state, vd, pd, weights=True, shared=True)
        assert torch.equal(on, out[:, :n]) and torch.equal(wn, w[:, :, :n]), n
        assert torch.equal(on, favor_query(qe[:, :n].contiguous(), state, vd, pd)), n
    for n in (0, nq // 2, nq - 1):                                                      # 4. a row alone has the bits it has among all rows
        o1, w1 = favor_query(qd[n:n + 1].contiguous(), state, vd, pd, weights=True, shared=True)
        assert torch.equal(o1, out[:, n:n + 1]) and torch.equal(w1, w[:, :, n:n + 1]), n


@pytest.mark.parametrize("case", SC.POISON_CASES, ids=SC.case_id)
def test_poison_behind_lens_reaches_nothing(gpulib, case):
    """6. the rows of v behind lens[t] hold a finite poison other than 0 (k holds NaN there in every case): out and w are unchanged.  The
    cached entry reads those rows against an exactly zero column of S; the long entry never reads them, as its contract says."""
    from mlhot.ops import favor_query
    form, T, Nc, d, m, lens = case
    qd, state, vd, pd = _setup(form, T, Nc, d, m, lens)
    _, state_p, vp, _ = _setup(form, T, Nc, d, m, lens, SC.POISON[form])
    for t, L in enumerate(lens):
        if L < Nc:
            assert bool((vp[t, L:] == SC.POISON[form]).all())
    want_out, want_w = favor_query(qd, state, vd, pd, weights=True, shared=True)
    for g in _groups(T):
        out, w = favor_query(qd, state_p, vp, pd, weights=True, shared=True, task_group=g)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, want_out) and torch.equal(w, want_w), g
    if form == "long":                                                                  # never read: NaN and Inf are as good
        for bad in (float("nan"), float("inf")):
            vb = vd.clone()
            for t, L in enumerate(lens):
                vb[t, L:] = bad
            assert torch.equal(favor_query(qd, state, vb, pd, shared=True), want_out), bad


def test_nothing_is_written_outside_out_and_w(gpulib):
    """Nq 17: a full row tile and a tile of one row; Nc 65: three chunks, a row length that is no multiple of 4; w starts 3 floats into
    its buffer; T 5 in groups of 2: the last group holds one task."""
    form, T, Nc, d, m, lens = "long", 5, 65, 64, 266, (33, 65, 1, 32, 64)
    Nq, lead, guard = 17, 3, 4096
    qd, state, vd, pd = _setup(form, T, Nc, d, m, lens)
    rows = qd[:Nq].contiguous()
    want_out, want_w = gpulib.favor_query_shared_fwd(rows, state.buf, vd, pd, "long", lens=state.lens_dev, weights=True)
    n, no = T * H * Nq * Nc, T * Nq * d * H
    buf = torch.full((lead + guard + n + guard,), float("nan"), device=DEV)
    obuf = torch.full((guard + no + guard,), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    w, out = buf[lead + guard:lead + guard + n], obuf[guard:guard + no]
    assert w.data_ptr() % 16 != 0 and w.data_ptr() % 4 == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = gpulib.c.mlhot_favor_query_long_shared_fwd(p(rows), p(state.buf), p(vd), p(pd), p(state.lens_dev), T, H, Nq, Nc, d, m, 2, p(out), p(w), p(ws), 256, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert not bool(torch.isnan(w).any()) and not bool(torch.isnan(out).any())          # every element is overwritten
    assert bool(torch.isnan(buf[:lead + guard]).all()) and bool(torch.isnan(buf[lead + guard + n:]).all())
    assert bool(torch.isnan(obuf[:guard]).all()) and bool(torch.isnan(obuf[guard + no:]).all())
    assert torch.equal(w.view(T, H, Nq, Nc), want_w) and torch.equal(out.view(T, Nq, d * H), want_out)


@pytest.mark.parametrize("entry,Nc,d,m,says", [("cached", 15, 24, 32, "Nc <= 32"), ("cached", 33, 16, 16, "Nc <= 32"), ("cached", 15, 16, 8, "Nc <= 32"),
                                               ("long", 40, 24, 32, "Nc <= 256"), ("long", 257, 16, 16, "Nc <= 256"), ("long", 40, 272, 32, "Nc <= 256")])
def test_outside_the_envelope_nothing_is_written(gpulib, entry, Nc, d, m, says):
    """7. d % 16 != 0, Nc past the entry's limit, m and d outside: MLHOT_ERR_UNSUPPORTED, and the sentinels stand."""
    T, Nq = 2, 5
    g = torch.Generator().manual_seed(3)
    q = 0.25 * torch.randn(Nq, H, d, generator=g).to(DEV)
    v = 0.25 * torch.randn(T, Nc, H, d, generator=g).to(DEV)
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((1 << 16,), 7.0, device=DEV)
    out = torch.full((T, Nq, d * H), float("nan"), device=DEV)
    w = torch.full((T, H, Nq, Nc), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    c = gpulib.c
    if entry == "cached":
        assert c.mlhot_favor_query_shared_ws_bytes(T, H, Nq, Nc, d, m) == 0
        rc = c.mlhot_favor_query_shared_fwd(p(q), p(state), p(v), p(proj), T, H, Nq, Nc, d, m, 0, p(out), p(w), p(ws), 256, None)
    else:
        assert c.mlhot_favor_query_long_shared_ws_bytes(T, H, Nq, Nc, d, m) == 0
        rc = c.mlhot_favor_query_long_shared_fwd(p(q), p(state), p(v), p(proj), None, T, H, Nq, Nc, d, m, 0, p(out), p(w), p(ws), 256, None)
    assert rc == 4                                                                      # MLHOT_ERR_UNSUPPORTED
    name = "favor_query_shared_fwd" if entry == "cached" else "favor_query_long_shared_fwd"
    assert f"{name} serves {says}" in c.mlhot_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(w).all()) and bool((state == 7.0).all())


def test_bad_arguments_write_nothing(gpulib):
    d, m, Nq = 16, 16, 5
    qd, state, vd, pd = _setup("cached", 2, 31, d, m, None)
    out = torch.full((2, Nq, d * H), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rows = qd[:Nq].contiguous()
    c = gpulib.c
    assert c.mlhot_favor_query_shared_fwd(p(rows), p(state.buf), p(vd), p(pd), 2, H, Nq, 31, d, m, -1, p(out), None, p(ws), 256, None) == 1      # task_group < 0
    assert c.mlhot_favor_query_shared_fwd(p(rows), p(state.buf), p(vd), p(pd), 2, H, Nq, 31, d, m, 0, None, None, p(ws), 256, None) == 1
    assert c.mlhot_favor_query_shared_fwd(p(rows), p(state.buf), p(vd), p(pd), 2, H, Nq, 31, d, m, 0, p(out), None, p(ws), 16, None) != 0
    assert b"workspace too small" in c.mlhot_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_the_states_and_keywords_that_do_not_combine_refuse(gpulib):
    """8. "summary", "paged" and "plain" states, and mask / mass / topk with shared=True, raise MlhotError naming what was asked."""
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_keys, favor_keys_paged, favor_query
    T, d, m, Nq = 2, 16, 16, 5
    g = torch.Generator().manual_seed(3)
    q = 0.25 * torch.randn(Nq, H, d, generator=g).to(DEV)
    k33, k300, k15 = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (33, 300, 15))
    pd = AC.proj(d, m).to(DEV)
    plain, paged, cached = favor_keys(k33, pd), favor_keys_paged(k300, pd), favor_keys(k15, pd)
    assert (plain.route, paged.route, cached.route) == ("plain", "paged", "cached")
    summary = FavorKeyState("summary", (T, 15, H, d, m), buf=cached.buf, lens=(15, 15))
    for state, v in ((plain, k33), (paged, k300), (summary, k15)):
        for kw in ({}, {"weights": True}):
            with pytest.raises(MlhotError, match=f"shared=True serves .* this state's route is '{state.route}'"):
                favor_query(q, state, v, pd, shared=True, **kw)
    for kw, name in (({"mask": torch.ones(T, Nq, 15, dtype=torch.bool, device=DEV)}, "mask="), ({"mass": True}, "mass="), ({"topk": 3}, "topk=")):
        with pytest.raises(MlhotError, match=f"shared=True with {name}"):
            favor_query(q, cached, k15, pd, shared=True, **kw)
    with pytest.raises(MlhotError, match="without a task axis"):                        # per-task rows are not shared rows
        favor_query(q[None].expand(T, -1, -1, -1).contiguous(), cached, k15, pd, shared=True)
    out = favor_query(q, cached, k15, pd, shared=True)                                   # ... and the state still serves
    assert torch.equal(out, favor_query(q[None].expand(T, -1, -1, -1).contiguous(), cached, k15, pd))
