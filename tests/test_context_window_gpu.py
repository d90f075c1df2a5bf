"""The kernels behind sliding-window cached contexts on the MI355X: mlhot_rows_compact bit for bit against
index_select / zeros over its envelope, key states rebuilt on compacted rows against the same keys op on rows compacted by torch and
against float64, and mlhot_favor_summary_retract against the float64 stream.  The retract bounds are relative to what the parent's
favor_absorb and favor_query show against float64 in the same test (tests/test_context_window_cpu.py keeps kappa <= 4).  -m gpu."""
import ctypes as C

import pytest
import torch

from tests import context_window_cases as WC
from tests import context_window_ref as WR
from tests import favor_cached_ref as CR
from tests import ragged_ref as RR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = WC.H
ERR_ARG, ERR_UNSUPPORTED = 1, 4


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


# ---- 1. rows_compact ----------------------------------------------------------------------------------------------------------------
def _raw(gpulib, srcs, dsts, widths, plan, T, cap):
    n = len(srcs)
    return gpulib.c.mlhot_rows_compact((C.c_void_p * n)(*[s.data_ptr() for s in srcs]), (C.c_void_p * n)(*[d.data_ptr() for d in dsts]),
                                       (C.c_int * n)(*widths), n, C.c_void_p(plan.data_ptr()), T, cap, None)


@pytest.mark.parametrize("sets", WC.ROW_SETS)
@pytest.mark.parametrize("cap,W", WC.ROW_SHAPES)
@pytest.mark.parametrize("T", WC.ROW_TS)
def test_rows_compact_is_index_select(gpulib, T, cap, W, sets):
    g = torch.Generator().manual_seed(T + cap + W + sets)
    widths = [W, 4 * ((W // 8) or 1), W + 4, 4][:sets]
    for kind in WC.PLANS:
        rows = WC.row_plan(kind, T, cap)
        plan = torch.tensor(rows, dtype=torch.int32).to(DEV)
        named = torch.zeros(T, cap, dtype=torch.bool)
        for t in range(T):
            named[t, [p for p in rows[t] if 0 <= p < cap]] = True
        srcs = []
        for i, w in enumerate(widths):
            x = torch.randn(T, cap, w, generator=g)
            x[~named] = float("nan") if i % 2 == 0 else float("inf")       # what no plan entry names must not reach dst
            srcs.append(x.to(DEV))
        dsts = [torch.full_like(x, float("nan")) for x in srcs]
        assert _raw(gpulib, srcs, dsts, widths, plan, T, cap) == 0, gpulib.c.mlhot_last_error()
        idx = plan.long().clamp(0, cap - 1)
        ok = (plan >= 0) & (plan < cap)
        for x, got in zip(srcs, dsts):
            want = torch.where(ok[:, :, None], torch.gather(x, 1, idx[:, :, None].expand(-1, -1, x.shape[2])), torch.zeros((), device=DEV))
            assert torch.equal(got, want), (kind, x.shape)
        again = gpulib.rows_compact(srcs, plan)
        assert all(torch.equal(a, b) for a, b in zip(again, dsts))


def test_rows_compact_refusals_write_nothing(gpulib):
    T, cap = 2, 8
    plan = torch.arange(cap, dtype=torch.int32).repeat(T, 1).to(DEV)
    x = torch.randn(T, cap, 16, device=DEV)
    keep = x.clone()
    assert _raw(gpulib, [x], [x], [16], plan, T, cap) == ERR_ARG                                  # dst is src
    assert _raw(gpulib, [x], [x.view(-1)[16:]], [16], plan, 1, cap) == ERR_ARG                    # dst overlaps src
    y = torch.full((T, cap, 16), 7.0, device=DEV)
    assert _raw(gpulib, [x, y], [y, torch.empty_like(x)], [16, 16], plan, T, cap) == ERR_ARG      # dst 0 is src 1
    assert _raw(gpulib, [x], [y], [6], plan, T, cap) == ERR_UNSUPPORTED                           # W % 4 != 0
    assert _raw(gpulib, [x], [y.view(-1)[1:]], [4], plan, 1, cap) == ERR_UNSUPPORTED              # dst not 16-byte aligned
    assert _raw(gpulib, [x] * 5, [y] * 5, [4] * 5, plan, 1, cap) == ERR_UNSUPPORTED               # 5 sets
    assert _raw(gpulib, [x], [y], [4], plan, 1, 4097) == ERR_UNSUPPORTED                          # cap
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and bool((y == 7.0).all())


# ---- 2. evicted key states -----------------------------------------------------------------------------------------------------------
def _keys_op(form):
    from mlhot import ops
    return {"keys": ops.favor_keys, "long": ops.favor_keys_long, "paged": ops.favor_keys_paged}[form]


@pytest.mark.parametrize("form,cap", WC.EVICT_FORMS)
@pytest.mark.parametrize("d,m", WC.SHAPES)
def test_keys_on_compacted_rows(gpulib, d, m, form, cap):
    from mlhot import ragged
    from mlhot.ops import favor_query
    k, proj, lens, drop = WC.evict_inputs(d, m, cap)
    T = WC.EVICT_T
    kd, pd = _dev(k), proj.to(DEV)
    old = _keys_op(form)(kd, pd, lens=lens)
    plan = ragged.KeepPlan(lens, drop, cap, DEV)
    kh, = gpulib.rows_compact([kd], plan.rows)
    got = ragged.masked_keys(kh, pd, plan, form)
    rows, total = ragged.keep_rows(lens, drop, cap)
    kt = WR.compact(torch.nan_to_num(k.permute(0, 2, 1, 3), nan=0.0), rows)                       # [T, cap, H, d] by torch on the host
    assert torch.equal(kh.cpu(), kt) and total == plan.total
    fresh = _keys_op(form)(kt.to(DEV), pd, lens=total)
    # the whole state, M included (F_k and M are all a key state holds; the bytes of its buffer behind them are never written)
    assert all(torch.equal(a, b) for a, b in zip(got.features(), fresh.features())) and got.lens == fresh.lens == total
    assert got.features()[1].item() <= old.features()[1].item() - 4.0                            # the dropped shot held M: it fell
    want_f, want_M = RR.key_features(kt.permute(0, 2, 1, 3).double(), proj.double(), total)
    F, M = got.features()
    eF = U.rel_err(F[..., :m], want_f)
    dd_scale = torch.einsum("tnhd,md->tnhm", d ** -0.25 * kt.double(), proj.double()).abs().max().item()
    eM = abs(M.item() - float(want_M)) / dd_scale
    print(f"evicted keys {form} cap={cap} d={d} m={m}: F_k {eF:.2e} of its scale, M off by {eM:.2e} of dd's scale")
    assert eF <= U.RTOL and eM <= U.RTOL
    g = torch.Generator().manual_seed(5)
    v = torch.randn(T, cap, H, d, generator=g).to(DEV)
    for Nq in (1, 16, 33):
        q = (0.25 * torch.randn(T, Nq, H, d, generator=g)).to(DEV)
        assert torch.equal(favor_query(q, got, v, pd), favor_query(q, fresh, v, pd))


# ---- 3. retract -------------------------------------------------------------------------------------------------------------------
def _per_th(x, want, scale):
    """max |x - want| / max |scale| per (task, head) -> [T, H]"""
    red = tuple(range(2, x.dim()))
    return ((x.double().cpu() - want).abs().amax(dim=red) / scale.abs().amax(dim=red)).clamp_min(0.0)


@pytest.mark.parametrize("regime", WC.REGIMES)
@pytest.mark.parametrize("N,R,which", WC.RETRACTS)
@pytest.mark.parametrize("d,m", WC.SHAPES)
def test_retract_against_the_float64_stream(gpulib, d, m, N, R, which, regime):
    from mlhot.ops import favor_absorb, favor_query, favor_retract
    T = WC.RETRACT_T
    q, k, v, proj = WC.retract_inputs(regime, d, m, N)
    lens, old, rest = WC.retract_split(N, R, which)
    n, nr = max(lens), max(len(r) for r in rest)
    pd, qd = proj.to(DEV), _dev(q)
    full64 = WR.absorbed(k, v, proj, [N] * T)
    rest64 = WR.absorbed(WC.gathered(k, rest, nr), WC.gathered(v, rest, nr), proj, [len(r) for r in rest], M=full64.M)
    own64 = WR.absorbed(WC.gathered(k, rest, nr), WC.gathered(v, rest, nr), proj, [len(r) for r in rest])
    kap = WR.kappa(full64, rest64, m)
    # the parent's own figures: favor_absorb's state on all N shots, favor_query on a freshly absorbed state of the rest
    full = favor_absorb(None, _dev(k), _dev(v), pd)
    A0, a0 = full.summary()[:2]
    absA, absa = _per_th(A0[:, :, :m], full64.A, full64.A), _per_th(a0[:, :, :m], full64.a, full64.a)
    fresh = favor_absorb(None, _dev(WC.gathered(k, rest, nr)), _dev(WC.gathered(v, rest, nr)), pd, lens=[len(r) for r in rest])
    qerr0 = U.rel_err(favor_query(qd, fresh, None, pd), CR.merged(own64.query(q, proj)))
    keep = full.buf.clone()
    # out of place, then in place through the binding: the same bits
    ko, vo = _dev(WC.gathered(k, old, n)), _dev(WC.gathered(v, old, n))
    got = favor_retract(full, ko, vo, pd, lens=None if all(L == n for L in lens) else lens)
    assert torch.equal(full.buf, keep) and got.lens == tuple(N - L for L in lens)
    buf = full.buf.clone()
    lens_dev = torch.tensor([[min(max(L - s, 0), 32) for L in lens] for s in range(0, n, 32)], dtype=torch.int32).to(DEV)
    for i, s in enumerate(range(0, n, 32)):
        gpulib.favor_summary_retract(ko[:, s:s + 32].contiguous(), vo[:, s:s + 32].contiguous(), pd, buf, lens=lens_dev[i], out=buf)
    assert torch.equal(buf, got.buf)
    A, a, vs, cnt, M = got.summary()
    assert M.item() == full.summary()[4].item()
    assert cnt.cpu().tolist() == [[N - L] * H for L in lens]
    assert all(bool(torch.isfinite(x).all()) for x in (A, a, vs)) and bool((a >= 0).all())
    assert bool((A[:, :, m:] == 0).all()) and bool((a[:, :, m:] == 0).all())
    retA, reta = _per_th(A[:, :, :m], rest64.A, full64.A), _per_th(a[:, :, :m], rest64.a, full64.a)
    qerr = U.rel_err(favor_query(qd, got, None, pd), CR.merged(rest64.query(q, proj)))
    print(f"retract {regime} d={d} m={m} {N}-{R} {which}: kappa {kap:.2f}; A {retA.max():.2e} (absorb {absA.max():.2e}), a {reta.max():.2e} "
          f"(absorb {absa.max():.2e}) of the state before; query {qerr:.2e} (fresh {qerr0:.2e}) of out's scale")
    assert bool((retA <= 4.0 * absA).all()), (retA, absA)
    assert bool((reta <= 4.0 * absa).all()), (reta, absa)
    assert qerr <= 4.0 * kap * qerr0


def test_retracting_a_shot_that_was_never_absorbed_stays_finite(gpulib):
    from mlhot.ops import favor_absorb, favor_retract
    d, m, N = 64, 266, 8
    q, k, v, proj = WC.retract_inputs("live", d, m, N)
    pd = proj.to(DEV)
    full = favor_absorb(None, _dev(k), _dev(v), pd)
    c, p = d ** -0.25, proj[0].double()
    alien = ((full.summary()[4].item() + 50.0) * p / (c * (p * p).sum())).float().expand(WC.RETRACT_T, H, 1, d).contiguous()      # dd 50 above M
    got = favor_retract(full, _dev(alien), _dev(v[:, :, :1].contiguous()), pd)
    A, a, vs, cnt, M = got.summary()
    assert all(bool(torch.isfinite(x).all()) for x in (A, a, vs, M)) and bool((a >= 0).all()) and cnt.cpu().tolist() == [[N - 1] * H] * WC.RETRACT_T
