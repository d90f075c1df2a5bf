"""NT-Xent (csrc/nt_xent.h: mlhot_nt_xent_fwd / _bwd) against the float64 reference over the whole envelope of its kernels:
tests/ntx_cases.py has the cases, the reference and the way dz is judged (tests/test_ntx_cases_cpu.py shows that a wrong partial column
block is outside the gradient bar on every case that has one).  Bars: the loss at 1e-6 max(1, 0.07 / t) max(1, |ref|), dz at util.RTOL.
Run on the MI355X box:  pytest tests -m gpu.  Worst errors on record: profiles/INDEX_ntx_envelope.md."""
import ctypes as C
import json
import math

import pytest
import torch

from tests import ntx_cases as NC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1                   # csrc/common.h MLHOT_ERR_ARG
SENTINEL = -777.25
BAND = 1024                   # floats in front of and behind the workspace slice


def _P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _direct(gpulib, c, z=None):
    """nt_xent_fwd, then nt_xent_bwd with the case's upstream gradient -> (loss, dz, ws) on the CPU."""
    z = NC.inputs(c.name).to(DEV) if z is None else z
    loss, ws = gpulib.nt_xent_fwd(z, c.div, c.mod, c.t)
    dz = gpulib.nt_xent_bwd(z, c.div, c.mod, c.t, ws, torch.tensor(c.gscale, device=DEV))
    torch.cuda.synchronize()
    return loss.cpu(), dz.cpu(), ws.cpu()


def _judge(c, loss, dz, what):
    """Finite, the loss and dz within their bars of the float64 reference (exact zeros where the reference is exactly zero); one line
    per call in the parity log."""
    r = NC.reference(c)
    finite = math.isfinite(loss.item()) and bool(torch.isfinite(dz).all())
    loss_err = abs(loss.item() - r.loss.item())
    dz_err = NC.dz_err(c, dz, r.dz) if finite else float("inf")
    rec = dict(case=c.name, route=what, loss_err=loss_err, loss_bound=NC.loss_bound(c, r.loss), dz_err=dz_err, dz_bound=U.RTOL)
    U.parity_log("ntx_envelope " + json.dumps(rec))
    print(f"ntx_envelope {c.name} {what}: loss err {loss_err:.2e}/{rec['loss_bound']:.2e} dz err {dz_err:.2e}/{U.RTOL:.0e}")
    assert finite, (c.name, what)
    if c.zero:
        assert loss.item() == 0.0 and not dz.any(), (c.name, what, loss.item(), float(dz.abs().max()))
        return
    assert loss_err <= rec["loss_bound"], (c.name, what, loss.item(), r.loss.item())
    if c.gscale == 0.0:
        assert not dz.any(), (c.name, what, float(dz.abs().max()))
    assert dz_err <= U.RTOL, f"{c.name} {what}: dz rel err {dz_err:.3e} > {U.RTOL}"


@pytest.mark.parametrize("case", NC.CASES, ids=NC.CASE_IDS)
def test_ntx_parity_over_the_envelope(gpulib, case):
    """Every case through the binding's two entries; twice, with the bits of the first call (the reductions are fixed-order); cases
    whose labels equal another case's (mod >= N) carry that case's bits."""
    loss, dz, _ = _direct(gpulib, case)
    _judge(case, loss, dz, "direct")
    loss2, dz2, _ = _direct(gpulib, case)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2), f"{case.name}: two calls on the same input differ"
    if case.bits_of:
        loss0, dz0, _ = _direct(gpulib, NC.BY_NAME[case.bits_of])
        assert torch.equal(loss, loss0) and torch.equal(dz, dz0), f"{case.name}: not the bits of {case.bits_of}"


@pytest.mark.parametrize("case", NC.GSCALE_CASES, ids=[c.name for c in NC.GSCALE_CASES])
def test_ntx_upstream_gradient_through_autograd(gpulib, case):
    """trainer.losses.nt_xent with the loss scaled by gscale before backward(): the bits of the direct calls, and the same bars."""
    from trainer.losses import nt_xent
    z = NC.inputs(case.name).to(DEV).requires_grad_()
    loss = nt_xent(z, case.div, case.mod, case.t)
    (loss * case.gscale).backward()
    torch.cuda.synchronize()
    _judge(case, loss.detach().cpu(), z.grad.cpu(), "autograd")
    loss0, dz0, _ = _direct(gpulib, case)
    assert torch.equal(loss.detach().cpu(), loss0) and torch.equal(z.grad.cpu(), dz0)


# the bar of the saved statistics is 1e-5 whatever t is, and the fp32 error of s = cos / t (which is the relative error of E and W and
# the absolute error of negmax) grows as 1 / t: the cases below the shipped temperature 0.07 are judged by loss and dz alone
STAT_CASES = [c for c in NC.CASES if c.t >= 0.07]


@pytest.mark.parametrize("case", STAT_CASES, ids=[c.name for c in STAT_CASES])
def test_ntx_saved_statistics(gpulib, case):
    """What the forward leaves in ws for the backward, ws = rinv | negmax | E | W (N16 floats each): rinv and E row by row, negmax and W
    at tensor scale (both pass through or near zero), all at 1e-5 of the float64 reference's; anchors without negatives have negmax = -inf
    and W = 0."""
    c, r = case, NC.reference(case)
    _, _, ws = _direct(gpulib, c)
    n16 = (c.N + 15) // 16 * 16
    rinv, negmax, E, W = (ws[k * n16:k * n16 + c.N].double() for k in range(4))
    hn = r.has_neg
    assert bool((negmax[~hn] == float("-inf")).all()) and bool((W[~hn] == 0.0).all()), c.name
    assert bool(torch.isfinite(negmax[hn]).all())
    err = dict(rinv=float(((rinv - r.rinv).abs() / r.rinv).max()))
    if bool(hn.any()):
        err["negmax"] = NC.rel_err(negmax[hn], r.negmax[hn])
        err["E"] = float(((E[hn] - r.E[hn]).abs() / r.E[hn]).max())
        err["W"] = NC.rel_err(W[hn], r.W[hn]) if bool(r.W[hn].any()) else float(W[hn].abs().max())
    print(f"ntx_envelope {c.name} statistics: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    U.parity_log("ntx_envelope_stats " + json.dumps(dict(case=c.name, err=err)))
    for k, v in err.items():
        assert v <= NC.STAT_RTOL, (c.name, k, v)


# ---- the workspace contract, through the C entry points with buffers the test owns ------------------------------------------------
def _raw(gpulib, N, d, div, mod, t, z, fill):
    """mlhot_nt_xent_fwd then _bwd on a workspace that is a slice of exactly mlhot_nt_xent_ws_floats(N) floats inside a larger tensor,
    filled with `fill`; the floats around it hold SENTINEL.  -> (loss, dz, the whole tensor, the slice's bounds)"""
    n = gpulib.c.mlhot_nt_xent_ws_floats(N)
    big = torch.full((n + 2 * BAND,), SENTINEL, device=DEV)
    ws = big[BAND:BAND + n]
    ws.fill_(fill)
    loss, dz, one = torch.full((3,), SENTINEL, device=DEV), torch.full((N * d + 2 * BAND,), SENTINEL, device=DEV), torch.ones((), device=DEV)
    rc = gpulib.c.mlhot_nt_xent_fwd(_P(z), N, d, div, mod, t, _P(ws), _P(loss[1:]), _stream())
    assert rc == 0, gpulib.c.mlhot_last_error().decode()
    rc = gpulib.c.mlhot_nt_xent_bwd(_P(z), N, d, div, mod, t, _P(ws), _P(one), _P(dz[BAND:]), _stream())
    assert rc == 0, gpulib.c.mlhot_last_error().decode()
    torch.cuda.synchronize()
    return loss.cpu(), dz.cpu(), big.cpu(), (BAND, BAND + n)


@pytest.mark.parametrize("N,d,div,mod", [(1, 16, 1, 1), (16, 80, 1, 2), (17, 80, 1, 2), (2033, 240, 19, 107)])
def test_ntx_workspace_contract(gpulib, N, d, div, mod):
    """A workspace of exactly the reported size, filled with NaN and with 1e30: loss and dz carry the same bits either way (nothing is
    read before it is written: rows past N of the four statistics, partial sums past the last workgroup), are finite, and no float next
    to the workspace, the loss or dz changes."""
    assert gpulib.c.mlhot_nt_xent_ws_floats(N) == 4 * ((N + 15) // 16 * 16) + (N + 15) // 16 * 16 // 16 + 16
    g = torch.Generator().manual_seed(N * 1000 + d)
    z = (torch.randn(N, d, generator=g) * (1.0 + torch.rand(N, 1, generator=g))).to(DEV)
    keep = z.clone()
    runs = [_raw(gpulib, N, d, div, mod, 0.07, z, fill) for fill in (float("nan"), 1e30)]
    assert torch.equal(z, keep)
    for loss, dz, big, (lo, hi) in runs:
        assert bool((big[:lo] == SENTINEL).all()) and bool((big[hi:] == SENTINEL).all()), "a float next to the workspace changed"
        assert loss[0] == SENTINEL and loss[2] == SENTINEL and math.isfinite(loss[1].item())
        assert bool((dz[:BAND] == SENTINEL).all()) and bool((dz[BAND + N * d:] == SENTINEL).all()), "a float next to dz changed"
        assert bool(torch.isfinite(dz[BAND:BAND + N * d]).all())
    (l0, d0, _, _), (l1, d1, _, _) = runs
    assert l0[1].view(torch.int32) == l1[1].view(torch.int32) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)), \
        "the results depend on what the workspace held before the call"
    if N == 1:
        assert l0[1] == 0.0 and not d0[BAND:BAND + d].any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
REFUSED = [("N=0", dict(N=0)), ("N=2049", dict(N=2049)), ("d=8", dict(d=8)), ("d=24", dict(d=24)), ("d=264", dict(d=264)),
           ("div=0", dict(div=0)), ("mod=0", dict(mod=0)), ("t=0", dict(t=0.0)), ("t=-1", dict(t=-1.0)), ("t=nan", dict(t=float("nan")))]


@pytest.mark.parametrize("why,bad", REFUSED, ids=[w for w, _ in REFUSED])
def test_ntx_refusals(gpulib, why, bad):
    """Both entries return MLHOT_ERR_ARG, set mlhot_last_error and leave loss, dz and ws as they were; trainer.losses.nt_xent raises for
    the N and d cases without a launch."""
    a = dict(N=32, d=64, div=1, mod=4, t=0.07)
    a.update(bad)
    z = torch.ones(2049 * 264, device=DEV)                     # large enough for whatever shape the call names
    loss, dz, ws = (torch.full((n,), SENTINEL, device=DEV) for n in (4, 2049 * 264, gpulib.c.mlhot_nt_xent_ws_floats(2064)))
    one = torch.ones((), device=DEV)
    c = gpulib.c
    for name, call in (("fwd", lambda: c.mlhot_nt_xent_fwd(_P(z), a["N"], a["d"], a["div"], a["mod"], a["t"], _P(ws), _P(loss), _stream())),
                       ("bwd", lambda: c.mlhot_nt_xent_bwd(_P(z), a["N"], a["d"], a["div"], a["mod"], a["t"], _P(ws), _P(one), _P(dz), _stream()))):
        assert c.mlhot_set_option(b"no_such_option", 0) == ERR_ARG              # last_error now names another entry
        assert b"nt_xent" not in c.mlhot_last_error()
        rc = call()
        assert rc == ERR_ARG, (why, name, rc)
        assert b"nt_xent" in c.mlhot_last_error(), (why, name, c.mlhot_last_error())
    torch.cuda.synchronize()
    assert all(bool((t_ == SENTINEL).all()) for t_ in (loss, dz, ws)), f"{why}: a refused call wrote something"
    if "N" in bad or "d" in bad:
        from mlhot.binding import MlhotError
        from trainer.losses import nt_xent
        zz = torch.ones(a["N"], a["d"], device=DEV, requires_grad=True)
        gpulib.prof_begin(16)
        try:
            with pytest.raises(MlhotError):
                nt_xent(zz, 1, 4, 0.07)
        finally:
            launches = gpulib.prof_end()
        assert launches == []
