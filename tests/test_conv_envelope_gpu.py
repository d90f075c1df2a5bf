"""The run-time-shaped convolution (csrc/conv_rt.h on ConvFwdRT / ConvDgradRT / ConvWgradRT and csrc/igemm.h, behind mlhot_conv2d_fwd /
_bwd / _bwd_scratch_bytes) against float64 over the whole envelope of its host decisions: tests/conv_cases.py has the cases with the
route each takes, the inputs and the reference; tests/test_conv_cases_cpu.py proves them on the host flavour first.
    exact pass  integer inputs: y, dx, dw, db carry the bits of the float64 reference (an index error shows on any element)
    real pass   rel_err(kernel, float64) <= tol + 2 x rel_err(torch float32 on the CPU, float64), tol = 1e-5 (y), 2e-5 (dx, dw, db)
Run on the MI355X box:  pytest tests -m gpu"""
import ctypes as C

import pytest
import torch

from tests import conv_cases as CC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 4096                   # bytes of 0x5A (at least) in front of and behind a buffer the test hands to the library
RELU_IDS = ["linear", "relu"]


def _log(line):
    U.parity_log(line)
    print(line)


@pytest.mark.parametrize("relu", [False, True], ids=RELU_IDS)
@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_conv_exact_pass(gpulib, name, relu):
    c = CC.BY_NAME[name]
    CC.judge(c, "exact", relu, CC.run(gpulib, c, "exact", relu, DEV), what="gpu", log=_log)


@pytest.mark.parametrize("relu", [False, True], ids=RELU_IDS)
@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_conv_real_pass(gpulib, name, relu):
    c = CC.BY_NAME[name]
    CC.judge(c, "real", relu, CC.run(gpulib, c, "real", relu, DEV), what="gpu", log=_log)


@pytest.mark.parametrize("case", CC.TWICE, ids=[c.name for c in CC.TWICE])
def test_split_k_runs_are_bit_equal(gpulib, case):
    """The slab reduction sums in a fixed order: two runs of a split-K weight gradient (256, 171 and 7 splits) give the same bits."""
    a, b = CC.run(gpulib, case, "real", True, DEV), CC.run(gpulib, case, "real", True, DEV)
    for n in CC.NAMES:
        assert torch.equal(CC.bits(a[n]), CC.bits(b[n])), f"{case.name}: {n} differs between two runs"


# ---- through the C entry points, with buffers the test owns -----------------------------------------------------------------------
class _Banded:
    """`nbytes` bytes filled with `fill`, between two bands of 0x5A, in one allocation of the test's own."""

    def __init__(self, nbytes, fill=0xFF):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 2 * BAND + 256,), 0x5A, dtype=torch.uint8, device=DEV)
        self.start = BAND + (-(self.buf.data_ptr() + BAND)) % 256
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


def _abi(gpulib, case, kind, relu, bias=True, give=("dx", "dw", "db"), short=0, scratch=True):
    """mlhot_conv2d_fwd into a NaN-filled, banded y, then mlhot_conv2d_bwd on that y into NaN-filled, banded dx / dw / db (only those
    named in `give` are passed, the others NULL) with a banded scratch of exactly mlhot_conv2d_bwd_scratch_bytes() bytes (the call is
    told `short` bytes less; scratch False: NULL and 0 bytes).  -> (rc_fwd, rc_bwd, {y, dx, dw, db, scratch: _Banded}, inputs kept)"""
    c, i = case, CC.inputs(case.name, kind)
    ins = [t.to(DEV) for t in (i.x, i.w, i.b, i.dy)]
    keep = [t.clone() for t in ins]
    x, w, b, dy = ins
    sb = gpulib.c.mlhot_conv2d_bwd_scratch_bytes(*c.shape)
    assert sb == 4 * c.wgrad[0] * c.Cout * (c.K + 1) + 256
    o = dict(y=_Banded(4 * dy.numel()), dx=_Banded(4 * x.numel()), dw=_Banded(4 * w.numel()), db=_Banded(4 * b.numel()), scratch=_Banded(sb))
    P = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    rc_f = gpulib.c.mlhot_conv2d_fwd(P(x), P(w), P(b) if bias else None, o["y"].ptr(), *c.shape, int(relu), stream)
    torch.cuda.synchronize()
    assert rc_f == 0, gpulib.c.mlhot_last_error().decode()
    out = {n: (o[n].ptr() if n in give else None) for n in ("dx", "dw", "db")}
    rc_b = gpulib.c.mlhot_conv2d_bwd(P(x), P(w), o["y"].ptr(), P(dy), *c.shape, int(relu), out["dx"], out["dw"], out["db"],
                                     o["scratch"].ptr() if scratch else None, sb - short if scratch else 0, stream)
    torch.cuda.synchronize()
    return rc_f, rc_b, o, all(torch.equal(a, k) for a, k in zip(ins, keep))


def _tensors(case, o, names=CC.NAMES):
    i = CC.inputs(case.name, "exact")
    shape = dict(y=i.dy.shape, dx=i.x.shape, dw=i.w.shape, db=i.b.shape)
    return {n: o[n].floats().view(shape[n]) for n in names}


@pytest.mark.parametrize("relu", [False, True], ids=RELU_IDS)
@pytest.mark.parametrize("case", CC.BANDED, ids=[c.name for c in CC.BANDED])
def test_conv_writes_every_output_and_nothing_else(gpulib, case, relu):
    """Outputs pre-filled with NaN between guard bands, scratch of exactly the reported size between guard bands: after the call no NaN
    is left in y, dx, dw, db (an input position no parity class writes, a class without a tap or behind the last output would keep
    it), every band is untouched, the inputs are, and the results are the exact pass's."""
    rc_f, rc_b, o, kept = _abi(gpulib, case, "exact", relu)
    assert rc_b == 0, gpulib.c.mlhot_last_error().decode()
    got = _tensors(case, o)
    for n in CC.NAMES:
        assert not bool(torch.isnan(got[n]).any()), f"{case.name}: {int(torch.isnan(got[n]).sum())} elements of {n} were never written"
    for n in CC.NAMES + ("scratch",):
        assert o[n].bands_untouched(), f"{case.name}: a byte next to {n} changed"
    assert kept, f"{case.name}: an input changed"
    CC.judge(case, "exact", relu, got, what="abi", log=_log)


NULLS = [CC.BY_NAME[n] for n in ("N2_C3_10x7_O4_k5_s2_p2", "N1_C2_20x30_O3_k3_s1_p1", "N1_C2_9x10_O3_k3_s4_p1")]


@pytest.mark.parametrize("case", NULLS, ids=[c.name for c in NULLS])
def test_conv_null_operands(gpulib, case):
    """b = NULL forward; then db = NULL, dx = NULL (the first layer), dw = db = NULL (the data gradient alone, which needs no scratch):
    every remaining output has the bits of the full call, a NaN-filled buffer whose pointer was not passed stays NaN."""
    rc_f, rc_b, full, _ = _abi(gpulib, case, "real", True)
    assert rc_b == 0, gpulib.c.mlhot_last_error().decode()
    want = _tensors(case, full)
    CC.judge(case, "real", True, want, what="abi full", log=_log)
    for give, scratch in ((("dx", "dw"), True), (("dw", "db"), True), (("dx",), True), (("dx",), False)):
        rc_f, rc_b, o, kept = _abi(gpulib, case, "real", True, give=give, scratch=scratch)
        assert rc_b == 0 and kept, (give, gpulib.c.mlhot_last_error().decode())
        got = _tensors(case, o)
        for n in ("dx", "dw", "db"):
            if n in give:
                assert torch.equal(CC.bits(got[n]), CC.bits(want[n])), f"{case.name}: {n} of the call with {give} differs from the full call's"
            else:
                assert o[n].untouched(), f"{case.name}: {n} was written though its pointer was not passed ({give})"
        assert all(o[n].bands_untouched() for n in o)
        if "dw" not in give:
            assert o["scratch"].untouched(), f"{case.name}: the data gradient alone wrote into the scratch"
    # no bias: y of the bias-less reference, and the gradients through it
    rc_f, rc_b, o, kept = _abi(gpulib, case, "real", True, bias=False, give=("dx", "dw"))
    assert rc_b == 0 and kept and o["db"].untouched()
    CC.judge(case, "real", True, _tensors(case, o, ("y", "dx", "dw")), bias=False, what="abi no bias", log=_log)
    rc_f, rc_b, o, kept = _abi(gpulib, case, "exact", True, bias=False, give=("dx", "dw"))
    assert rc_b == 0 and kept and o["db"].untouched()
    CC.judge(case, "exact", True, _tensors(case, o, ("y", "dx", "dw")), bias=False, what="abi no bias", log=_log)


@pytest.mark.parametrize("case", NULLS[:2], ids=[c.name for c in NULLS[:2]])
def test_conv_short_scratch_is_refused(gpulib, case):
    """One byte less than mlhot_conv2d_bwd_scratch_bytes(): MLHOT_ERR_WORKSPACE, named by mlhot_last_error, and dw, db, dx (which comes
    after the weight gradient) and the scratch keep what they held."""
    rc_f, rc_b, o, kept = _abi(gpulib, case, "real", True, short=1)
    assert rc_b == CC.ERR_WORKSPACE, rc_b
    assert b"conv2d_bwd: scratch too small" in gpulib.c.mlhot_last_error()
    assert kept and all(o[n].untouched() for n in ("dx", "dw", "db", "scratch")), f"{case.name}: a refused call wrote something"
    rc_f, rc_b, o, kept = _abi(gpulib, case, "real", True, scratch=False)
    assert rc_b == CC.ERR_WORKSPACE and all(o[n].untouched() for n in ("dx", "dw", "db"))


def test_conv_argument_refusals(gpulib):
    """What tests/test_conv_cases_cpu.py holds on the host flavour, on the product library: no bad shape reaches a launch."""
    CC.check_refusals(gpulib, DEV)


@pytest.mark.parametrize("bias,need_dx", [(False, False), (True, True)], ids=["no_bias_no_dx", "bias_dx"])
def test_conv2d_function_branches(gpulib, bias, need_dx):
    """mlhot.ops.Conv2dFunction with bias=None on an input that needs no gradient (need_dx / has_bias False: the first layer of a
    bias-less network), and with both, against the same reference."""
    from mlhot.ops import Conv2dFunction
    c = CC.BY_NAME["N2_C3_10x7_O4_k5_s2_p2"]
    for kind in CC.KINDS:
        i = CC.inputs(c.name, kind)
        x = i.x.to(DEV).requires_grad_(need_dx)
        w = i.w.to(DEV).requires_grad_()
        b = i.b.to(DEV).requires_grad_() if bias else None
        y = Conv2dFunction.apply(x, w, b, c.s, c.p, True)
        y.backward(i.dy.to(DEV))
        assert (x.grad is not None) == need_dx
        got = dict(y=y.detach().cpu(), dx=x.grad.cpu() if need_dx else None, dw=w.grad.cpu(), db=b.grad.cpu() if bias else None)
        CC.judge(c, kind, True, got, bias=bias, what=f"Conv2dFunction bias={int(bias)} dx={int(need_dx)}", log=_log)
