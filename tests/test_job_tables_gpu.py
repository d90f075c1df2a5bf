"""csrc/mlp_chain.h's four C entries (mlhot_mlp_chain_fwd / _bwd, mlhot_linear_multi_fwd / _bwd) on the MI355X, through their C ABI on
windows of sentinel-filled buffers (tests/job_table_cases.py): every output and gradient against float64 at tests.util.RTOL, nothing
outside a logical window written, the launch labels, each table job bit-equal to the same job launched alone through mlhot_linear_fwd /
mlhot_linear_bwd and wherever it stands in a table, each chain weight gradient bit-equal to mlhot_linear_bwd's skinny weight gradient of
the chain's own g, every refusal without a launch or a write, and zero rows at the ops level.  Run with -m gpu.  Worst errors on record:
profiles/INDEX_job_tables.md."""
import pytest
import torch

from tests import job_table_cases as J
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(items):
    return [(i[0] if isinstance(i, tuple) else i).name for i in items]


def _err(lib):
    return lib.c.mlhot_last_error().decode()


def _compare(what, name, got, want, worst):
    """One output against float64: written everywhere (no sentinel left, finite), whole tensor / last row / last column at RTOL."""
    if got is None:
        assert want is None, f"{what}: {name} is NULL in the call but the reference has it"
        return
    assert want is not None and got.shape == want.shape, f"{what}: {name} shape"
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()) and not bool((got == J.SENTINEL).any()), f"{what}: {name} has unwritten elements"
    errs = [U.rel_err(got, want)]
    if got.dim() == 2:
        errs += [U.rel_err(got[-1], want[-1]), U.rel_err(got[:, -1], want[:, -1])]
    print(f"job_tables {what} {name}: " + " ".join(f"{e:.2e}" for e in errs))
    key = name.rstrip("0123456789")
    worst[key] = max(worst.get(key, 0.0), max(errs))
    assert max(errs) <= U.RTOL, f"{what}: {name} rel err {errs} > {U.RTOL}"


def _zeros(what, name, got):
    assert got is None or int(torch.count_nonzero(got)) == 0, f"{what}: {name} of an empty batch is not zero"


@pytest.mark.parametrize("c", J.CHAIN_CASES, ids=_ids(J.CHAIN_CASES))
def test_chain_case(gpulib, c):
    r = J.run_chain(gpulib, c, DEV)
    what = f"chain/{c.name}"
    assert r.rc_fwd == 0 and r.rc_bwd == 0, (r.rc_fwd, r.rc_bwd, _err(gpulib))
    assert not r.bad_fwd, f"{what}: the forward changed {r.bad_fwd} outside a logical window"
    assert not r.bad_bwd, f"{what}: the backward changed {r.bad_bwd} outside a logical window"
    assert r.labels_fwd == (["chain.fwd"] if c.M else []), r.labels_fwd
    assert sorted(r.labels_bwd) == (["chain.bwd.dgrad", "chain.bwd.wgrad"] if c.M else ["chain.bwd.wgrad"]), r.labels_bwd
    ref, worst = J.chain_reference(c, r.data), {}
    for k, l in enumerate(c.layers):
        _compare(what, f"y{k}", r.y[k], ref.y[k], worst)
        _compare(what, f"g{k}", r.g[k], ref.g[k], worst)
        _compare(what, f"dw{k}", r.dw[k], ref.dw[k], worst)
        _compare(what, f"db{k}", r.db[k], ref.db[k], worst)
        _compare(what, f"dside{k}", r.dside[k], ref.dside[k], worst)
        if c.M == 0:
            assert not bool((r.dw[k] == J.SENTINEL).any()) and (r.db[k] is None or not bool((r.db[k] == J.SENTINEL).any())), f"{what}: dw / db not written"
            _zeros(what, f"dw{k}", r.dw[k])
            _zeros(what, f"db{k}", r.db[k])
    _compare(what, "dx0", r.dx0, ref.dx0, worst)
    # the chain's weight gradients are linear_skinny.h's wgrad_body over the chain's own g: bit-equal to that body launched alone
    for k, col0, dw, db in J.chain_wgrad_alone(gpulib, c, r, DEV):
        assert J.same_bits(r.dw[k][:, col0:col0 + dw.shape[1]], dw), f"{what}: dw{k} columns {col0}.. differ from mlhot_linear_bwd's in bits"
        if db is not None:
            assert J.same_bits(r.db[k], db), f"{what}: db{k} differs from mlhot_linear_bwd's in bits"
    U.parity_log(f"job_tables {what}: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())) + "; weight gradients bit-equal to mlhot_linear_bwd's")


def _check_job(what, j, o, bwd, worst):
    ref = J.job_reference(j, o.data)
    _compare(what, "y", o.y, ref.y, worst)
    if bwd:
        for name in ("dx", "dx2", "dw", "db"):
            _compare(what, name, getattr(o, name), getattr(ref, name), worst)
        if j.M == 0:
            assert not bool((o.dw == J.SENTINEL).any()) and (o.db is None or not bool((o.db == J.SENTINEL).any())), f"{what}: dw / db not written"
            _zeros(what, "dw", o.dw)
            _zeros(what, "db", o.db)


def _same_job(what, a, b, bwd):
    for name in ("y",) + (("dx", "dx2", "dw", "db") if bwd else ()):
        assert J.same_bits(getattr(a, name), getattr(b, name)), f"{what}: {name} differs in bits"


@pytest.mark.parametrize("t", J.MULTI_CASES, ids=_ids(J.MULTI_CASES))
def test_multi_case(gpulib, t):
    n, what = len(t.jobs), f"multi/{t.name}"
    r = J.run_multi(gpulib, t.jobs, DEV, bwd=t.bwd)
    assert r.rc_fwd == 0 and (not t.bwd or r.rc_bwd == 0), (r.rc_fwd, r.rc_bwd, _err(gpulib))
    assert not r.bad_fwd, f"{what}: the forward changed {r.bad_fwd} outside a logical window"
    assert r.labels_fwd == (["linear_multi.fwd"] if any(j.M for j in t.jobs) else []), r.labels_fwd
    if t.bwd:
        assert not r.bad_bwd, f"{what}: the backward changed {r.bad_bwd} outside a logical window"
        assert r.labels_bwd == ["linear_multi.bwd"], r.labels_bwd
    worst = {}
    for i, (j, o) in enumerate(zip(t.jobs, r.jobs)):
        _check_job(f"{what}/{i}", j, o, t.bwd, worst)
    # a one-source job = the same sk:: bodies as mlhot_linear_fwd's skinny launch and mlhot_linear_bwd's combined one
    alone = 0
    for i, (j, o) in enumerate(zip(t.jobs, r.jobs)):
        if j.K2 or not j.dx:
            continue
        a = J.run_job_alone(gpulib, j, DEV)
        assert J.same_bits(o.y, a.y), f"{what}/{i}: y differs from mlhot_linear_fwd's in bits"
        if t.bwd:
            assert a.labels == ["linear_bwd"], a.labels            # the combined skinny launch (at M == 0 its weight-gradient half)
            for name in ("dx", "dw", "db"):
                assert J.same_bits(getattr(o, name), getattr(a, name)), f"{what}/{i}: {name} differs from mlhot_linear_bwd's in bits"
        alone += 1
    # whatever its position and neighbours: the reversed table, and every job as a table of its own
    if n > 1:
        rev = J.run_multi(gpulib, t.jobs[::-1], DEV, bwd=t.bwd)
        assert rev.rc_fwd == 0 and (not t.bwd or rev.rc_bwd == 0) and not rev.bad_fwd and not rev.bad_bwd
        for i, (o, p) in enumerate(zip(r.jobs, rev.jobs[::-1])):
            _same_job(f"{what}/{i} reversed", o, p, t.bwd)
        for i, j in enumerate(t.jobs):
            one = J.run_multi(gpulib, [j], DEV, bwd=t.bwd)
            assert one.rc_fwd == 0 and (not t.bwd or one.rc_bwd == 0) and not one.bad_fwd and not one.bad_bwd
            _same_job(f"{what}/{i} alone in a table", r.jobs[i], one.jobs[0], t.bwd)
    U.parity_log(f"job_tables {what}: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())) +
                 f"; {alone} one-source jobs bit-equal to mlhot_linear_fwd / _bwd" + (f"; {n} jobs bit-equal reversed and alone" if n > 1 else ""))


@pytest.mark.parametrize("c,stage", J.CHAIN_REFUSALS, ids=_ids(J.CHAIN_REFUSALS))
def test_chain_refusal(gpulib, c, stage):
    """An error return, nothing launched, every buffer as it was."""
    assert J.chain_refused(c, bwd=True) is not None
    r = J.run_chain(gpulib, c, DEV)
    if stage == "fwd":
        assert r.rc_fwd != 0 and r.labels_fwd == [] and not r.bad_fwd
        assert all(bool((y == J.SENTINEL).all()) for y in r.y), "a refused forward wrote a y"
    else:
        assert r.rc_fwd == 0, _err(gpulib)
    assert r.rc_bwd != 0 and r.labels_bwd == [], (r.rc_bwd, r.labels_bwd)
    assert r.bank.untouched(everything=True) == [], "a refused backward wrote"


@pytest.mark.parametrize("t,stage", J.MULTI_REFUSALS, ids=_ids(J.MULTI_REFUSALS))
def test_multi_refusal(gpulib, t, stage):
    assert J.multi_refused(t, bwd=True) is not None
    r = J.run_multi(gpulib, t.jobs, DEV)
    if stage == "fwd":
        assert r.rc_fwd != 0 and r.labels_fwd == [] and not r.bad_fwd
        assert all(bool((o.y == J.SENTINEL).all()) for o in r.jobs), "a refused forward wrote a y"
    else:
        assert r.rc_fwd == 0, _err(gpulib)
    assert r.rc_bwd != 0 and r.labels_bwd == [], (r.rc_bwd, r.labels_bwd)
    assert all(o.bank.untouched(everything=True) == [] for o in r.jobs), "a refused backward wrote"


@pytest.mark.parametrize("with_arena", [False, True], ids=["plain", "arena"])
def test_zero_rows_give_zero_weight_gradients(gpulib, with_arena):
    """mlp_chain(), Linear2Function and HeadStacksFunction over inputs without rows: every weight and bias gradient is exact zeros (the
    gradient of an empty sum - the kernels write them; the binding hands them uninitialised storage or a slot of the gradient arena,
    poisoned here), every input gradient is empty."""
    from mlhot import binding
    from mlhot.arena import GradArena
    from mlhot.ops import HeadStacksFunction, Linear2Function, linear2_ok, mlp_chain
    g = torch.Generator().manual_seed(3)
    par = lambda *s: torch.randn(*s, generator=g).to(DEV).requires_grad_()
    empty = lambda *s: torch.zeros(*s, device=DEV).requires_grad_()
    w1, b1, w2, b2 = par(12, 12), par(12), par(5, 12), par(5)               # chain: [side | x0] -> 12 -> 5
    w3, b3 = par(8, 12), par(8)                                              # Linear2: cat([xa, xb]) -> 8
    H, h = 2, 8
    sw, sb = [torch.randn(H * h, h, generator=g).to(DEV) for _ in range(2)], [torch.randn(H * h, generator=g).to(DEV) for _ in range(2)]
    heads = [[sw[i].view(H, h, h)[k].clone().requires_grad_() for k in range(H)] + [sb[i].view(H, h)[k].clone().requires_grad_() for k in range(H)]
             for i in range(2)]
    params = [w1, b1, w2, b2, w3, b3] + [p for hp in heads for p in hp]
    x0, side, xa, xb = empty(0, 8), empty(0, 4), empty(0, 8), empty(0, 4)
    xs = [empty(1, 0, h), empty(1, 0, h)]
    arena = GradArena([w1, b1, w2, b2, w3, b3]).refresh() if with_arena else None
    if arena is not None:
        arena.flat.fill_(float("nan"))
    binding.set_grad_arena(arena)
    try:
        y1 = mlp_chain(x0, [(w1, b1, "relu", side, True), (w2, b2, "tanh", None, False)])
        assert y1 is not None and y1.shape == (0, 5)
        assert linear2_ok(xa, xb, w3)
        y2 = Linear2Function.apply(xa, xb, w3, b3, "relu")
        outs = HeadStacksFunction.apply(H, 2, xs[0], sw[0], sb[0], xs[1], sw[1], sb[1], *[p for hp in heads for p in hp])
        assert y2.shape == (0, 8) and all(o.shape == (1, 0, H, h) for o in outs)
        poison = torch.full((1 << 16,), float("nan"), device=DEV)           # what the backward's torch.empty_like is likely to be handed
        del poison
        (y1.sum() + y2.sum() + sum(o.sum() for o in outs)).backward()
        torch.cuda.synchronize()
    finally:
        binding.set_grad_arena(None)
    for i, p in enumerate(params):
        assert p.grad is not None and p.grad.shape == p.shape, i
        assert int(torch.count_nonzero(p.grad)) == 0 and bool(torch.isfinite(p.grad).all()), f"parameter {i}: the gradient of an empty sum is not zero"
    for t in (x0, side, xa, xb, *xs):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.numel() == 0
