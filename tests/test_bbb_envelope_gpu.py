"""The Bayes-by-backprop sample kernels (mlhot_bbb_sample_fwd / _bwd, mlhot_bbb_sample_multi_fwd / _bwd) against the float64 reference
over the value and size edges of tests/bbb_cases.py: every output within 4 x the float32 reference expression's own error in term
scales (bbb_cases.BOUND; tests/test_bbb_cases_cpu.py measures it), exact zeros where no gradient arrives, the same bits on a second
run, nothing written outside the outputs, the two routes within the bound of each other.
Run on the MI355X box:  pytest tests -m gpu.  Worst errors on record: profiles/INDEX_b1_envelope.md."""
import json
import math

import pytest
import torch

from tests import bbb_cases as BC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1                   # csrc/common.h MLHOT_ERR_ARG


def _judge(c, out, what):
    items, kl, clean = out
    err = BC.errors(c, (items, kl))
    U.parity_log("b1_envelope " + json.dumps(dict(case=c.name, route=what, err=err)))
    print(f"b1_envelope {c.name} {what}: " + " ".join(f"{k}={v:.3e}/{BC.BOUND[k]:.2e}" for k, v in err.items()))
    assert clean, f"{c.name} {what}: a float outside the output slices changed"
    for k, v in err.items():
        assert v <= BC.BOUND[k], (c.name, what, k, v, BC.BOUND[k])
    for i in BC.exact_zero_items(c):
        assert not items[i].dmu.any() and not items[i].drho.any(), (c.name, what, i)


@pytest.mark.parametrize("case", BC.CASES, ids=BC.CASE_IDS)
def test_bbb_multi_over_the_table(gpulib, case):
    out = BC.run(gpulib, case, "multi", DEV)
    _judge(case, out, "multi")
    assert BC.same_bits(out, BC.run(gpulib, case, "multi", DEV)), f"{case.name}: two runs on the same input differ"


@pytest.mark.parametrize("case", BC.BOTH, ids=[c.name for c in BC.BOTH])
def test_bbb_single_tensor_over_the_table(gpulib, case):
    """The single-tensor route (run_foreach with its grid clamp, run_reduce1 over n KL terms), and the multi route on the same case
    within the bound of it: per element in term scales, both being within the bound of float64."""
    out = BC.run(gpulib, case, "single", DEV)
    _judge(case, out, "single")
    assert BC.same_bits(out, BC.run(gpulib, case, "single", DEV)), f"{case.name}: two runs on the same input differ"
    (a,), kl_a, _ = out
    (b,), kl_b, _ = BC.run(gpulib, case, "multi", DEV)
    r = BC.reference(case)
    s = r.scales[0]
    for k in ("w", "dmu", "drho"):
        e = BC.term_err(getattr(a, k), getattr(b, k).double(), getattr(s, k))
        assert e <= BC.BOUND[k], (case.name, "single against multi", k, e)
    assert abs(float(kl_a) - float(kl_b)) / r.kl_scale <= BC.BOUND["kl"], (case.name, float(kl_a), float(kl_b))


def test_bbb_overflow_pattern_is_the_float32_expressions(gpulib):
    """rho in {88, 89, 100}: expf overflows from 89 on.  Recorded behaviour, no float64 target: the inf / nan pattern of every output
    equals that of the reference's float32 expression in torch on the CPU (sigma = inf: w = +-inf or nan, kl = inf, d mu finite,
    d rho nan)."""
    c = BC.OVERFLOW
    ref, kl_ref = BC.expression(c, torch.float32)
    assert math.isinf(float(kl_ref))
    for route in ("single", "multi"):
        items, kl, clean = BC.run(gpulib, c, route, DEV)
        assert clean and BC.nonfinite_pattern(kl).item() == BC.nonfinite_pattern(kl_ref).item() == 1
        for f in ("w", "dmu", "drho") + (("klterm",) if route == "single" else ()):
            assert torch.equal(BC.nonfinite_pattern(getattr(items[0], f)), BC.nonfinite_pattern(getattr(ref[0], f))), (route, f)


def test_bbb_multi_refuses_a_33rd_item(gpulib):
    """MLHOT_ERR_ARG from both entries, mlhot_last_error names them, nothing is written; the binding raises as it does today."""
    from mlhot.binding import BbbItem, MlhotError
    n = 33
    t = torch.zeros(8, device=DEV)
    arr = (BbbItem * n)()
    for a in arr:
        a.mu = a.rho = a.eps = a.w = a.dmu = a.drho = t.data_ptr()
        a.n = 8
    kl, partial = torch.full((1,), 7.0, device=DEV), torch.full((64,), 7.0, device=DEV)
    s = BC._stream(DEV)
    assert gpulib.c.mlhot_bbb_sample_multi_fwd(arr, n, BC._P(partial), BC._P(kl), s) == ERR_ARG
    assert gpulib.c.mlhot_bbb_sample_multi_bwd(arr, n, BC._P(kl), s) == ERR_ARG
    assert b"bbb_sample_multi" in gpulib.c.mlhot_last_error()
    torch.cuda.synchronize()
    assert kl.item() == 7.0 and not t.any() and bool((partial == 7.0).all())
    ts = [torch.zeros(8, device=DEV) for _ in range(33)]
    with pytest.raises(MlhotError):
        gpulib.bbb_sample_multi_fwd(ts, ts, ts)
