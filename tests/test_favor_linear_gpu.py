"""FAVOR+ in linear form (csrc/favor_linear.h, option "favor_linear") on the MI355X: parity with the float64 reference over
tests/favor_linear_cases.py, repeatability, the launch labels of each route, the route function, the workspace contract and the staged
entries.  Run on the MI355X box:  pytest tests -m gpu"""
import ctypes as C

import pytest
import torch

from tests import favor_linear_cases as LC
from tests.test_favor_envelope_gpu import _Banded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_WORKSPACE = 2             # csrc/common.h MLHOT_ERR_WORKSPACE
SMALL = (2, 2, 16, 16, 64, 266)      # both sides <= 32: favor2.h's two launches whatever "favor_linear" says


class _linear:
    """`with _linear(gpulib, value):` sets the option for the block and puts the default (0) back."""

    def __init__(self, lib, value):
        self.lib, self.value = lib, value

    def __enter__(self):
        self.lib.set_option("favor_linear", self.value)

    def __exit__(self, *exc):
        self.lib.set_option("favor_linear", 0)


def _operands(case):
    return tuple(t.to(DEV) for t in LC.kernel_layout(LC.inputs(case.name)))


def _run(gpulib, case, staged=False):
    """favor_fwd, then favor_bwd on the forward's own out and workspace -> {out, dq, dk, dv} on the CPU, reference layout."""
    qn, kn, vn, dout, proj = _operands(case)
    ex = None
    if staged:
        from mlhot.dist import StabiliserExchange
        ex = (StabiliserExchange(), torch.zeros(4, device=DEV))
    out, ws = gpulib.favor_fwd(qn, kn, vn, proj, exchange=ex)
    dq, dk, dv = gpulib.favor_bwd(qn, kn, vn, proj, out, dout, ws, exchange=ex)
    torch.cuda.synchronize()
    return LC.reference_layout(case, *(t.cpu() for t in (out, dq, dk, dv)))


@pytest.mark.parametrize("name", LC.CASE_IDS)
def test_parity_with_float64(gpulib, name):
    """out, dq, dk, dv of the linear route inside RTOL + 2 e32 of the float64 reference on every case.  (Fails on a library without the
    option: set_option refuses the unknown name.)"""
    case = LC.BY_NAME[name]
    with _linear(gpulib, 1):
        got = _run(gpulib, case)
    LC.judge(case, got, "linear")
    if case.Nc == 1:          # with the centre Ctx is exactly 0
        assert not got["dq"].any() and not got["dk"].any(), f"{name}: dq / dk of a single key are not exact zeros"
    if case.variant == "dup":
        assert torch.equal(got["out"][:, :, 0], got["out"][:, :, 1]), f"{name}: out of two equal queries differs"


@pytest.mark.parametrize("case", LC.FUNCTION, ids=[c.name for c in LC.FUNCTION])
def test_parity_through_favor_function(gpulib, case):
    from mlhot.ops import FavorFunction
    qn, kn, vn, dout, proj = _operands(case)
    qn, kn, vn = (t.requires_grad_() for t in (qn, kn, vn))
    with _linear(gpulib, 1):
        out = FavorFunction.apply(qn, kn, vn, proj)
        out.backward(dout)
        torch.cuda.synchronize()
    got = LC.reference_layout(case, *(t.detach().cpu() for t in (out, qn.grad, kn.grad, vn.grad)))
    LC.judge(case, got, "linear_function")


def test_two_runs_have_the_same_bits(gpulib):
    case = LC.BY_NAME["T2_H2_Nq40_Nc70_d64_m266"]
    with _linear(gpulib, 1):
        a, b = _run(gpulib, case), _run(gpulib, case)
    for n in LC.NAMES:
        assert torch.equal(a[n], b[n]), n


def _labels(gpulib, dims, operands):
    qn, kn, vn, dout, proj = operands
    gpulib.prof_begin(256)
    try:
        out, ws = gpulib.favor_fwd(qn, kn, vn, proj)
        gpulib.favor_bwd(qn, kn, vn, proj, out, dout, ws)
    finally:
        recs = gpulib.prof_end()
    return [label for label, _ in recs]


def test_launch_labels_of_each_route(gpulib):
    case = LC.BY_NAME["T2_H2_Nq40_Nc70_d64_m266"]
    ops = _operands(case)
    T, H, Nq, Nc, d, m = SMALL
    g = torch.Generator().manual_seed(5)
    small = (torch.randn(T, Nq, H, d, generator=g).to(DEV), torch.randn(T, Nc, H, d, generator=g).to(DEV), torch.randn(T, Nc, H, d, generator=g).to(DEV),
             torch.randn(T, Nq, d * H, generator=g).to(DEV), LC.FC.projection(m, d).to(DEV))
    with _linear(gpulib, 1):
        on = _labels(gpulib, case.shape, ops)
        on_small = _labels(gpulib, SMALL, small)
    off = _labels(gpulib, case.shape, ops)
    print("favor_linear labels on:", on, "off:", off, "small:", on_small)
    lin = [x for x in on if x.startswith("favor.lin.")]
    assert {"favor.lin.ctx", "favor.lin.out", "favor.lin.bwd.dctx", "favor.lin.bwd.Gq", "favor.lin.bwd.Gk", "favor.lin.bwd.dv"} <= set(lin)
    assert "favor.S" not in on and "favor.bwd.dS" not in on
    assert "favor.S" in off and "favor.bwd.dS" in off and not [x for x in off if x.startswith("favor.lin.")]
    assert "favor.f1" in on_small and "favor.f2" in on_small and not [x for x in on_small if x.startswith("favor.lin.")]


def test_route_function_and_envelope(gpulib):
    from mlhot.ops import favor_route
    sup = gpulib.favor_linear_supported
    for c in LC.CASES:
        assert sup(*c.shape), c.name
        assert favor_route(*c.shape) == "chain", c.name
    assert not sup(*SMALL) and favor_route(*SMALL) == "two_launch"
    outside = [(1, 2, 6, 40, 40, 147), (1, 1, 5, 40, 64, 1537), (1, 2, 5, 40, 64, 15)]       # d 40, m 1537, m 15
    with _linear(gpulib, 1):
        for c in LC.CASES:
            assert favor_route(*c.shape) == "linear", c.name
        assert favor_route(*SMALL) == "two_launch"
        for shape in outside:
            assert not sup(*shape) and favor_route(*shape) == "chain", shape
    for shape in outside:
        assert not sup(*shape) and favor_route(*shape) == "chain", shape
    assert gpulib.c.mlhot_favor_linear_supported(*LC.CASES[0].shape) == 1 and gpulib.c.mlhot_favor_linear_supported(*SMALL) == 0


def _abi_call(gpulib, case, ws_fill, short=0):
    """tests/test_favor_envelope_gpu.py's method: mlhot_favor_fwd then mlhot_favor_bwd on a workspace of exactly mlhot_favor_ws_bytes()
    bytes filled with `ws_fill` (the calls are told `short` bytes less), outputs pre-filled with 0xFF."""
    c = case
    ins = list(_operands(c))
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
    rc_b = gpulib.c.mlhot_favor_bwd(P(qn), P(kn), P(vn), P(proj), *dims, o["out"].ptr(), P(dout), o["dq"].ptr(), o["dk"].ptr(), o["dv"].ptr(),
                                    ws.ptr(), wb - short, stream)
    torch.cuda.synchronize()
    return rc_f, rc_b, ws, o, all(torch.equal(a, b) for a, b in zip(ins, keep))


@pytest.mark.parametrize("name", ["T2_H2_Nq40_Nc70_d64_m266", "T1_H2_Nq5_Nc40_d64_m17", "T1_H2_Nq35_Nc1_d64_m266"])
def test_workspace_contract(gpulib, name):
    """A workspace of exactly the reported size poisoned with 0xFF gives the bits of a zero-filled one and no byte outside it or the
    outputs changes; one 256-byte block less: MLHOT_ERR_WORKSPACE, nothing written."""
    case = LC.BY_NAME[name]
    with _linear(gpulib, 1):
        rc_f, rc_b, ws, o, kept = _abi_call(gpulib, case, 0xFF)
        assert (rc_f, rc_b) == (0, 0), gpulib.c.mlhot_last_error().decode()
        rc_f0, rc_b0, ws0, o0, kept0 = _abi_call(gpulib, case, 0x00)
        assert (rc_f0, rc_b0) == (0, 0), gpulib.c.mlhot_last_error().decode()
        assert kept and kept0, f"{name}: an input changed"
        for n in LC.NAMES:
            a, b = o[n].floats(), o0[n].floats()
            assert bool(torch.isfinite(a).all()), f"{name}: {n} on a poisoned workspace is not finite"
            assert torch.equal(a, b), f"{name}: {n} depends on what the workspace held before the call"
            assert o[n].bands_untouched() and o0[n].bands_untouched(), f"{name}: a byte next to {n} changed"
        assert ws.bands_untouched() and ws0.bands_untouched(), f"{name}: a byte next to the workspace changed"
        got = LC.reference_layout(case, *(o[n].floats().view(s) for n, s in (
            ("out", (case.T, case.Nq, case.d * case.H)), ("dq", (case.T, case.Nq, case.H, case.d)),
            ("dk", (case.T, case.Nc, case.H, case.d)), ("dv", (case.T, case.Nc, case.H, case.d)))))
        LC.judge(case, got, "abi_linear")
        rc_f, rc_b, ws, o, kept = _abi_call(gpulib, case, 0xFF, short=256)
        assert (rc_f, rc_b) == (ERR_WORKSPACE, ERR_WORKSPACE), (rc_f, rc_b)
        assert kept and ws.untouched() and all(o[n].untouched() for n in LC.NAMES), f"{name}: a refused call wrote something"


def test_staged_entries_keep_their_route(gpulib):
    """mlhot_favor_fwd_staged / bwd_staged at a world of one give the same bits with the option on as with it off."""
    case = LC.STAGED
    off = _run(gpulib, case, staged=True)
    with _linear(gpulib, 1):
        on = _run(gpulib, case, staged=True)
    for n in LC.NAMES:
        assert torch.equal(on[n], off[n]), n
