"""FAVOR+ (csrc/favor2.h's two-launch kernels and favor.h's operator chain) against the float64 reference over the whole envelope of
fv::applies() and just outside it: tests/favor_cases.py has the cases, the reference and the bound rule
    rel_err(kernel, reference in float64) <= RTOL + 2 x rel_err(reference in float32, reference in float64)
(tests/test_favor_cases_cpu.py shows that the right-hand side never exceeds 3e-4).  Run on the MI355X box:  pytest tests -m gpu"""
import ctypes as C
import json

import pytest
import torch

from tests import favor_cases as FC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_WORKSPACE = 2             # csrc/common.h MLHOT_ERR_WORKSPACE
BAND = 4096                   # bytes of 0x5A (at least) in front of and behind a buffer the test hands to the library
ROUTE_NAME = {1: "two_launch", 0: "chain"}

# (case, favor2 option): both implementations inside the envelope; outside it the chain is the only route, run once under the default
ROUTES = [(c, f2) for c in FC.CASES for f2 in ((1, 0) if c.route == "two_launch" else (1,))]
ROUTE_IDS = [f"{c.name}-{ROUTE_NAME[f2] if c.route == 'two_launch' else 'chain_only'}" for c, f2 in ROUTES]
STAGED = [(c, f2) for c, f2 in ROUTES if c in FC.STAGED]
STAGED_IDS = [i for (c, _), i in zip(ROUTES, ROUTE_IDS) if c in FC.STAGED]
ABI = [(c, f2) for c, f2 in ROUTES if c.route == "two_launch"]
ABI_IDS = [i for (c, _), i in zip(ROUTES, ROUTE_IDS) if c.route == "two_launch"]


@pytest.fixture
def favor2(gpulib):
    """Selects the FAVOR+ implementation for one test (1: favor2.h where it applies, 0: favor.h's chain) and puts the default back."""
    yield lambda value: gpulib.set_option("favor2", value)
    gpulib.set_option("favor2", 1)


def _run(gpulib, case, staged=False):
    """favor_fwd, then favor_bwd on the forward's own out and workspace -> {out, dq, dk, dv} on the CPU, reference layout."""
    qn, kn, vn, dout, proj = (t.to(DEV) for t in FC.kernel_layout(FC.inputs(case.name)))
    ex = None
    if staged:
        from mlhot.dist import StabiliserExchange
        ex = (StabiliserExchange(), torch.zeros(4, device=DEV))
    out, ws = gpulib.favor_fwd(qn, kn, vn, proj, exchange=ex)
    dq, dk, dv = gpulib.favor_bwd(qn, kn, vn, proj, out, dout, ws, exchange=ex)
    torch.cuda.synchronize()
    if staged:
        assert list(ex[0].calls) == ["fwd", "bwd"]
    return FC.reference_layout(case, *(t.cpu() for t in (out, dq, dk, dv)))


def _judge(case, got, what):
    """Finite, and within the bound of the float64 reference; one line per call in the parity log."""
    ref, e32, bound = FC.reference(case, torch.float64), FC.e32(case), FC.bounds(case)
    floor = FC.floors(case, ref)
    finite = {n: bool(torch.isfinite(got[n]).all()) for n in FC.NAMES}
    err = {n: U.rel_err(got[n], ref[n], floor[n]) if finite[n] else float("inf") for n in FC.NAMES}
    rec = dict(case=case.name, route=what, err=err, e32=e32, bound=bound)
    U.parity_log("favor_envelope " + json.dumps(rec))
    print(f"favor_envelope {case.name} {what}: " + " ".join(f"{n}={err[n]:.2e}/{bound[n]:.2e}" for n in FC.NAMES))
    assert all(finite.values()), (case.name, what, finite)
    for n in FC.NAMES:
        assert err[n] <= bound[n], f"{case.name} {what}: {n} rel err {err[n]:.3e} > {bound[n]:.3e} (e32 {e32[n]:.2e})"
    return err


@pytest.mark.parametrize("case,f2", ROUTES, ids=ROUTE_IDS)
def test_favor_parity_over_the_envelope(gpulib, favor2, case, f2):
    favor2(f2)
    got = _run(gpulib, case)
    _judge(case, got, ROUTE_NAME[f2] if case.route == "two_launch" else "chain_only")
    if case.variant == "dup":
        # ties: every key row holds the batch-global key maximum, query rows 0 and 1 are equal - the tie convention must not show
        assert torch.equal(got["out"][:, :, 0], got["out"][:, :, 1]), f"{case.name}: out of two equal queries differs"
        floor = FC.floors(case, FC.reference(case, torch.float64))["dq"]
        assert U.rel_err(got["dq"][:, :, 0], got["dq"][:, :, 1], floor) <= U.RTOL


@pytest.mark.parametrize("case,f2", STAGED, ids=STAGED_IDS)
def test_favor_staged_world_of_one_equals_the_plain_route(gpulib, favor2, case, f2):
    favor2(f2)
    plain, staged = _run(gpulib, case), _run(gpulib, case, staged=True)
    _judge(case, staged, "staged_" + (ROUTE_NAME[f2] if case.route == "two_launch" else "chain_only"))
    for n in FC.NAMES:
        assert torch.equal(plain[n], staged[n]), f"{case.name}: staged {n} differs from the plain route's bits"


# ---- the workspace contract, through the C entry points with buffers the test owns ------------------------------------------------
class _Banded:
    """`nbytes` bytes filled with `fill`, between two bands of 0x5A, in one allocation of the test's own."""

    def __init__(self, nbytes, fill):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 2 * BAND + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        self.start = BAND + (-(self.buf.data_ptr() + BAND)) % 256          # the library's arena wants a 256-byte aligned base
        self.mid = self.buf[self.start:self.start + nbytes]
        self.mid.fill_(fill)
        assert self.mid.data_ptr() % 256 == 0 and self.buf.numel() - (self.start + nbytes) >= BAND
        self.fill = fill

    def ptr(self):
        return C.c_void_p(self.mid.data_ptr())

    def bands_untouched(self):
        return bool((self.buf[:self.start] == 0x5A).all()) and bool((self.buf[self.start + self.nbytes:] == 0x5A).all())

    def untouched(self):
        return self.bands_untouched() and bool((self.mid == self.fill).all())

    def floats(self):
        return self.mid.view(torch.float32).cpu()


def _abi_call(gpulib, case, ws_fill, short=0):
    """mlhot_favor_fwd then mlhot_favor_bwd on a workspace of exactly mlhot_favor_ws_bytes() bytes filled with `ws_fill` (the calls are
    told `short` bytes less), outputs pre-filled with NaN.  Returns (rc_fwd, rc_bwd, ws, outputs {name: _Banded}, inputs_unchanged)."""
    c = case
    ins = [t.to(DEV) for t in FC.kernel_layout(FC.inputs(c.name))]
    keep = [t.clone() for t in ins]
    qn, kn, vn, dout, proj = ins
    wb = gpulib.c.mlhot_favor_ws_bytes(c.T, c.H, c.Nq, c.Nc, c.d, c.m)
    assert wb > 0
    ws = _Banded(wb, ws_fill)
    o = {n: _Banded(4 * t.numel(), 0xFF) for n, t in (("out", dout), ("dq", qn), ("dk", kn), ("dv", vn))}
    P = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    dims = (c.T, c.H, c.Nq, c.Nc, c.d, c.m)
    rc_f = gpulib.c.mlhot_favor_fwd(P(qn), P(kn), P(vn), P(proj), *dims, o["out"].ptr(), ws.ptr(), wb - short, stream)
    torch.cuda.synchronize()
    # the backward differentiates through the forward's out; after a refused forward it is handed the (NaN) buffer all the same
    rc_b = gpulib.c.mlhot_favor_bwd(P(qn), P(kn), P(vn), P(proj), *dims, o["out"].ptr(), P(dout), o["dq"].ptr(), o["dk"].ptr(), o["dv"].ptr(),
                                    ws.ptr(), wb - short, stream)
    torch.cuda.synchronize()
    return rc_f, rc_b, ws, o, all(torch.equal(a, b) for a, b in zip(ins, keep))


@pytest.mark.parametrize("case,f2", ABI, ids=ABI_IDS)
def test_favor_workspace_contract(gpulib, favor2, case, f2):
    """A workspace of exactly the reported size, poisoned (0xFF: NaN as float, huge as int): the results are finite and carry the bits
    of a run on a zero-filled workspace - nothing is read before it is written (features >= m, rows past Nq + Nc, the partial maxima of
    feature chunks past m) - and no byte outside the workspace or the outputs changes.  One byte less: MLHOT_ERR_WORKSPACE, nothing
    written."""
    favor2(f2)
    rc_f, rc_b, ws, o, kept = _abi_call(gpulib, case, 0xFF)
    assert (rc_f, rc_b) == (0, 0), gpulib.c.mlhot_last_error().decode()
    rc_f0, rc_b0, ws0, o0, kept0 = _abi_call(gpulib, case, 0x00)
    assert (rc_f0, rc_b0) == (0, 0), gpulib.c.mlhot_last_error().decode()
    assert kept and kept0, f"{case.name}: an input changed"
    for n in FC.NAMES:
        a, b = o[n].floats(), o0[n].floats()
        assert bool(torch.isfinite(a).all()), f"{case.name}: {n} on a poisoned workspace is not finite"
        assert torch.equal(a, b), f"{case.name}: {n} depends on what the workspace held before the call"
        assert o[n].bands_untouched() and o0[n].bands_untouched(), f"{case.name}: a byte next to {n} changed"
    assert ws.bands_untouched() and ws0.bands_untouched(), f"{case.name}: a byte next to the workspace changed"
    got = FC.reference_layout(case, *(o[n].floats().view(s) for n, s in (
        ("out", (case.T, case.Nq, case.d * case.H)), ("dq", (case.T, case.Nq, case.H, case.d)),
        ("dk", (case.T, case.Nc, case.H, case.d)), ("dv", (case.T, case.Nc, case.H, case.d)))))
    _judge(case, got, "abi_" + ROUTE_NAME[f2])
    rc_f, rc_b, ws, o, kept = _abi_call(gpulib, case, 0xFF, short=1)
    assert (rc_f, rc_b) == (ERR_WORKSPACE, ERR_WORKSPACE), (rc_f, rc_b)
    assert kept and ws.untouched() and all(o[n].untouched() for n in FC.NAMES), f"{case.name}: a refused call wrote something"
