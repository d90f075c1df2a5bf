"""The kernel behind joined cached contexts on the MI355X: mlhot_rows_gather bit for bit against torch indexing
over its envelope - sources of different T_j and cap_j, plans that hold the fill, out-of-range sources and rows and a row named twice,
poisoned rows that nothing names - its refusals, which write nothing, and concat's finishing step: the key state on gathered rows
against the same keys op on rows gathered by torch.  -m gpu."""
import ctypes as C

import pytest
import torch

from tests import context_join_ref as JR
from tests import favor_summary_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = JR.H
ERR_ARG, ERR_UNSUPPORTED = 1, 4


def _raw(gpulib, srcs, rows, dsts, widths, plan, T, cap, nsrc=None, sets=None):
    """srcs[i][j]: set i of source j (tensors, or raw addresses)."""
    sets = len(dsts) if sets is None else sets
    nsrc = len(rows) if nsrc is None else nsrc
    ptr = lambda x: x if isinstance(x, int) or x is None else x.data_ptr()       # noqa: E731
    flat = [ptr(x) for per_set in srcs for x in per_set]
    return gpulib.c.mlhot_rows_gather((C.c_void_p * len(flat))(*flat), (C.c_int64 * len(rows))(*rows), nsrc, (C.c_void_p * len(dsts))(*[ptr(d) for d in dsts]),
                                      (C.c_int * len(widths))(*widths), sets, None if plan is None else C.c_void_p(ptr(plan)), T, cap, None)


def _sources(widths, nsrc, plan, g):
    """Per row set the nsrc sources [T_j, cap_j, W] on the device: random where the plan names a row, NaN / Inf everywhere else."""
    keep = JR.named(plan, nsrc)
    out = []
    for i, w in enumerate(widths):
        per_set = []
        for j, (tj, cj) in enumerate(JR.SRC_SHAPES[:nsrc]):
            x = torch.full((tj * cj, w), float("nan") if (i + j) % 2 == 0 else float("inf"))
            idx = sorted(keep[j])
            if idx:
                x[idx] = torch.randn(len(idx), w, generator=g)
            per_set.append(x.view(tj, cj, w).to(DEV))
        out.append(per_set)
    return out


def _check(gpulib, widths, nsrc, T, cap, seed):
    g = torch.Generator().manual_seed(seed)
    rows = [t * c for t, c in JR.SRC_SHAPES[:nsrc]]
    for rows_host in JR.kernel_plans(T, cap, nsrc, seed):
        plan = torch.tensor(rows_host, dtype=torch.int32).to(DEV)
        srcs = _sources(widths, nsrc, rows_host, g)
        dsts = [torch.full((T, cap, w), float("nan"), device=DEV) for w in widths]
        assert _raw(gpulib, srcs, rows, dsts, widths, plan, T, cap) == 0, gpulib.c.mlhot_last_error()
        for per_set, got in zip(srcs, dsts):
            want = JR.gathered(per_set, plan)
            assert bool(torch.isfinite(want).all())                                # what no entry names is in no expected row
            assert torch.equal(got, want), (widths, nsrc, T, cap)                  # ... and every row came back written: no NaN is left
        again = gpulib.rows_gather([[srcs[i][j] for i in range(len(widths))] for j in range(nsrc)], plan, T, cap)
        assert all(torch.equal(a, b) for a, b in zip(again, dsts))


@pytest.mark.parametrize("T", JR.TS)
@pytest.mark.parametrize("nsrc", JR.NSRCS)
@pytest.mark.parametrize("widths", JR.WIDTHS)
def test_rows_gather_is_torch_indexing(gpulib, widths, nsrc, T):
    for cap in JR.CAPS:
        _check(gpulib, widths, nsrc, T, cap, seed=sum(widths) + 10 * nsrc + T + cap)


@pytest.mark.parametrize("nsrc", (1, 8))
def test_rows_gather_at_4096_slots(gpulib, nsrc):
    _check(gpulib, (8,), nsrc, 3, 4096, seed=nsrc)
    _check(gpulib, (8, 8), nsrc, 1, 4096, seed=nsrc + 1)


def test_rows_gather_refusals_write_nothing(gpulib):
    T, cap = 2, 8
    plan = torch.zeros(T, cap, 2, dtype=torch.int32, device=DEV)
    x, x2 = torch.randn(T, cap, 16, device=DEV), torch.randn(T, cap, 16, device=DEV)
    keep = x.clone()
    y, y2 = torch.full((T, cap, 16), 7.0, device=DEV), torch.full((T, cap, 16), 7.0, device=DEV)
    n = T * cap
    assert _raw(gpulib, [[x]], [n], [y], [6], plan, T, cap) == ERR_UNSUPPORTED                               # W % 4 != 0
    assert _raw(gpulib, [[x]], [n], [y.view(-1)[1:]], [4], plan, 1, cap) == ERR_UNSUPPORTED                  # dst not 16-byte aligned
    assert _raw(gpulib, [[x.view(-1)[1:]]], [n - 1], [y], [4], plan, 1, cap) == ERR_UNSUPPORTED              # src not 16-byte aligned
    assert _raw(gpulib, [[x], [x], [x]], [n], [y, y2, y], [4, 4, 4], plan, 1, cap) == ERR_UNSUPPORTED        # 3 sets
    assert _raw(gpulib, [[x] * 9], [n] * 9, [y], [4], plan, 1, cap) == ERR_UNSUPPORTED                       # 9 sources
    assert _raw(gpulib, [[x]], [n], [y], [4], plan, 1, 4097) == ERR_UNSUPPORTED                              # cap
    assert _raw(gpulib, [[x]], [n], [y], [4], plan, 1, 0) == ERR_UNSUPPORTED
    assert _raw(gpulib, [[x]], [2 ** 31], [y], [4], plan, 1, cap) == ERR_UNSUPPORTED                         # rows_j >= 2^31
    assert _raw(gpulib, [[x]], [n], [x], [16], plan, T, cap) == ERR_ARG                                      # dst is src
    assert _raw(gpulib, [[x]], [n], [x.view(-1)[16:]], [16], plan, 1, cap) == ERR_ARG                        # dst overlaps src
    assert _raw(gpulib, [[x, y]], [n, n], [y], [16], plan, T, cap) == ERR_ARG                                # dst is the second source
    assert _raw(gpulib, [[x], [x2]], [n], [y, y], [16, 16], plan, T, cap) == ERR_ARG                         # dst 0 is dst 1
    assert _raw(gpulib, [[x], [y2]], [n], [y, y2], [16, 16], plan, T, cap) == ERR_ARG                        # dst 1 is set 1 of the source
    assert _raw(gpulib, [[None]], [n], [y], [16], plan, T, cap) == ERR_ARG                                   # NULL
    assert _raw(gpulib, [[x]], [n], [None], [16], plan, T, cap) == ERR_ARG
    assert _raw(gpulib, [[x]], [n], [y], [16], None, T, cap) == ERR_ARG
    assert _raw(gpulib, [[x, None]], [n, n], [y], [16], plan, T, cap) == ERR_ARG
    assert b"rows_gather" in gpulib.c.mlhot_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and bool((y == 7.0).all()) and bool((y2 == 7.0).all())
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError, match=r"sets=1 nsrc=1 cap=8 W=6"):
        gpulib.rows_gather([[torch.randn(T, cap, 6, device=DEV)]], plan, T, cap)


# ---- concat's finishing step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,na,nb", JR.KEY_JOINS)
@pytest.mark.parametrize("d,m", JR.KEY_SHAPES)
def test_keys_on_gathered_rows(gpulib, d, m, form, na, nb):
    """The key state concat builds - ragged.masked_keys on mlhot_rows_gather's rows under the ONE GatherPlan - is torch.equal to
    masked_keys called directly on rows gathered with torch index ops, and the gathered rows are the sources' rows."""
    from mlhot import ragged
    from mlhot.ops import favor_query
    T = JR.KEY_T
    g = torch.Generator().manual_seed(d + m + na)
    proj = S.proj_for(d, m).to(DEV)
    lens, caps = [(na, max(na // 2, 1)), (nb, nb - 1)], [na + 3, nb]
    srcs = []
    for (la, cap) in zip(lens, caps):
        k = 0.25 * torch.randn(T, cap, H, d, generator=g)
        for t, L in enumerate(la):
            k[t, L:] = float("nan")                                                   # the spare slots of a source are never read
        srcs.append(k.to(DEV))
    parts = [[(0, t), (1, t)] for t in range(T)]
    capacity = na + nb
    plan = ragged.GatherPlan(parts, lens, caps, capacity, DEV)
    kh, = gpulib.rows_gather([[k] for k in srcs], plan.rows, T, capacity)
    got = ragged.masked_keys(kh, proj, plan, form)
    kt = torch.zeros(T, capacity, H, d, device=DEV)
    for t in range(T):
        kt[t, :lens[0][t]] = srcs[0][t, :lens[0][t]]
        kt[t, lens[0][t]:lens[0][t] + lens[1][t]] = srcs[1][t, :lens[1][t]]
    assert torch.equal(kh, kt) and plan.total == tuple(a + b for a, b in zip(*lens))
    direct = ragged.masked_keys(kt, proj, plan, form)
    assert got.route == {"keys": "cached"}.get(form, form) and got.lens == direct.lens == plan.total
    assert all(torch.equal(a, b) for a, b in zip(got.features(), direct.features()))
    v = torch.randn(T, capacity, H, d, generator=g).to(DEV)
    q = (0.25 * torch.randn(T, 5, H, d, generator=g)).to(DEV)
    assert torch.equal(favor_query(q, got, v, proj), favor_query(q, direct, v, proj))
