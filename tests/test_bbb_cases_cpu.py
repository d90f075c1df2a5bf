"""No GPU: the case table of tests/bbb_cases.py proven here - it holds what the issue of the B1 envelope lists, its float32 reference
expression stays under a quarter of every bound (that is where the bounds come from), and the hostsim build of the four entries
(mlhot_bbb_sample_fwd / _bwd, mlhot_bbb_sample_multi_fwd / _bwd) passes the same table under the same bounds.  The GPU run of the
table is tests/test_bbb_envelope_gpu.py; figures on record: profiles/INDEX_b1_envelope.md."""
import math

import pytest
import torch

from tests import bbb_cases as BC

ERR_ARG = 1                   # csrc/common.h MLHOT_ERR_ARG


def test_the_table_holds_every_edge():
    names = set(BC.CASE_IDS)
    assert all(f"one_n{n}" in names for n in (1, 255, 256, 257, 1023, 1024, 1025, 3073, 4095, 4096, 4097, 256 * 16 * 256 + 1))
    assert all(BC.BY_NAME[f"one_n{n}"].both for n in BC.SINGLE_SIZES)
    assert {c.dkl for c in BC.CASES} == {0.0, 1e-7, 0.3, 1.0} and {c.dkl for c in BC.BOTH} == {0.0, 1e-7, 0.3, 1.0}
    counts = {len(c.items) for c in BC.CASES}
    assert {1, 2, 32} <= counts and max(counts) == 32
    m32 = BC.BY_NAME["multi32_dkl1"]
    assert {it.n for it in m32.items} == {1, 255, 256, 257, 1023, 1024, 1025, 2049} and m32.items[-1].n == 1
    assert {(it.dw, it.two) for it in m32.items} == {(d, t) for d in (True, False) for t in ("none", "dw2", "nodw2")}
    mixed = [it.n for it in BC.BY_NAME["multi_mixed_chunks"].items]
    assert mixed[0] <= 1024 < mixed[1] and mixed[2] <= 1024 and mixed[-1] == 1          # one chunk, several, one chunk; the last item one element
    assert [it.n for it in BC.BY_NAME["multi2_1024_1"].items] == [1024, 1]                # a chunk boundary that is an item boundary
    assert BC.workgroups(BC.BY_NAME["multi_1025_workgroups"]) == 1025
    big = BC.BY_NAME["multi_4097_workgroups"]
    assert BC.workgroups(big) == 4097 and len(big.items) == 1 and big.items[0].n == 4096 * 1024 + 1
    assert any(BC.exact_zero_items(c) for c in BC.CASES if len(c.items) == 1) and len(BC.exact_zero_items(BC.BY_NAME["multi32_dkl0"])) >= 4


def test_the_value_cross_is_walked_whole():
    """Every (rho, mu, eps) triple of the cross is an element of every item of at least 385 elements; sigma = 0.1 is met to float32
    rounding; every term of every scale is finite in float32 (the smallest sigma is 6.1e-6: 0.01 / sigma^3 = 4e13)."""
    assert len(BC.RHOS) == 11 and abs(math.log1p(math.exp(BC.RHO_EDGE)) - 0.1) < 1e-15
    x = BC.inputs(BC.BY_NAME["one_n1025"])[0]
    seen = {(float(r), float(m), float(e)) for r, m, e in zip(x.rho[:BC.CROSS], x.mu[:BC.CROSS], x.eps[:BC.CROSS])}
    want = {(float(torch.tensor(r, dtype=torch.float32)), float(torch.tensor(m, dtype=torch.float32)), e) for r in BC.RHOS for m in BC.MUS for e in BC.EPSS}
    assert seen == want and len(want) == 385
    for c in BC.CASES:
        if c.name in BC.LARGEST:
            continue
        s, skl = BC.scales(c)
        fmax = torch.finfo(torch.float32).max
        assert all(float(getattr(i, k).max()) < fmax for i in s for k in ("w", "w2", "klterm", "dmu", "drho")) and skl < fmax, c.name
        for x in BC.inputs(c):
            assert float(x.rho.min()) >= -12.0 and float(x.rho.max()) <= 12.0 and float(x.mu.abs().max()) <= 3.0 and float(x.eps.abs().max()) <= 4.0


def test_the_bounds_are_four_times_the_measured_reference_error():
    assert set(BC.BOUND) == set(BC.KINDS) and all(BC.BOUND[k] == 4.0 * BC.REF32_WORST[k] for k in BC.KINDS)


@pytest.mark.parametrize("case", BC.CASES, ids=BC.CASE_IDS)
def test_the_float32_reference_stays_under_a_quarter_of_the_bounds(case):
    """The reference's own float32 expression (torch on the CPU, autograd) against float64, in term scales."""
    err = BC.errors(case, BC.expression(case, torch.float32))
    print(f"bbb_cases {case.name} float32 expression: " + " ".join(f"{k}={v:.3e}" for k, v in err.items()))
    assert set(err) == set(BC.KINDS)
    for k, v in err.items():
        assert v <= BC.BOUND[k] / 4.0, (case.name, k, v, BC.BOUND[k] / 4.0)


def test_gradients_by_autograd_equal_the_hand_derived_formula_in_float64():
    """The formulas in the comment of BbbSampleBwd, in float64, against the reference's autograd: 1e-12 of the term scale."""
    c = BC.BY_NAME["multi32_dkl1"]
    r = BC.reference(c)
    for x, want, s in zip(BC.inputs(c), r.items, r.scales):
        mu, rho, eps = x.mu.double(), x.rho.double(), x.eps.double()
        sigma = torch.log1p(torch.exp(rho))
        zero = torch.zeros_like(mu)
        dw, dw2 = (zero if x.dw is None else x.dw.double()), (zero if x.dw2 is None else x.dw2.double())
        eps2 = zero if x.eps2 is None else x.eps2.double()
        dmu = dw + dw2 + c.dkl * mu / sigma ** 2
        drho = (dw * eps + dw2 * eps2 + c.dkl * (1 / sigma - 0.01 / sigma ** 3 - mu ** 2 / sigma ** 3)) * torch.sigmoid(rho)
        assert BC.term_err(dmu, want.dmu, s.dmu) <= 1e-12 and BC.term_err(drho, want.drho, s.drho) <= 1e-12


def _judge(c, out, what):
    items, kl, clean = out
    err = BC.errors(c, (items, kl))
    print(f"bbb_cases {c.name} {what}: " + " ".join(f"{k}={v:.3e}/{BC.BOUND[k]:.2e}" for k, v in err.items()))
    assert clean, f"{c.name} {what}: a float outside the output slices changed"
    for k, v in err.items():
        assert v <= BC.BOUND[k], (c.name, what, k, v, BC.BOUND[k])
    for i in BC.exact_zero_items(c):
        assert not items[i].dmu.any() and not items[i].drho.any(), (c.name, what, i)
    return err


HOSTSIM_CASES = [c for c in BC.CASES if c.name not in ("multi_1025_workgroups", "multi_4097_workgroups")]      # the two largest: seconds each


@pytest.mark.parametrize("case", HOSTSIM_CASES, ids=[c.name for c in HOSTSIM_CASES])
def test_hostsim_over_the_table(hostsim, case):
    multi = BC.run(hostsim, case, "multi", "cpu")
    _judge(case, multi, "hostsim multi")
    assert BC.same_bits(multi, BC.run(hostsim, case, "multi", "cpu"))
    if case.both:
        single = BC.run(hostsim, case, "single", "cpu")
        _judge(case, single, "hostsim single")
        assert BC.same_bits(single, BC.run(hostsim, case, "single", "cpu"))


def test_hostsim_overflow_pattern_is_the_float32_expressions(hostsim):
    """rho in {88, 89, 100}: expf overflows from 89 on.  No float64 target: the inf / nan pattern of every output equals that of the
    reference's float32 expression in torch on the CPU (sigma = inf: w = +-inf or nan, kl = inf, d mu finite, d rho nan)."""
    c = BC.OVERFLOW
    ref, kl_ref = BC.expression(c, torch.float32)
    assert math.isinf(float(kl_ref)) and bool(torch.isnan(ref[0].drho[1::3]).all()) and bool(torch.isfinite(ref[0].drho[0::3]).all())
    for route in ("single", "multi"):
        items, kl, clean = BC.run(hostsim, c, route, "cpu")
        assert clean and BC.nonfinite_pattern(kl).item() == BC.nonfinite_pattern(kl_ref).item() == 1
        for f in ("w", "dmu", "drho") + (("klterm",) if route == "single" else ()):
            assert torch.equal(BC.nonfinite_pattern(getattr(items[0], f)), BC.nonfinite_pattern(getattr(ref[0], f))), (route, f)


def test_hostsim_refuses_a_33rd_item(hostsim):
    from mlhot.binding import BbbItem
    n = 33
    t = torch.zeros(8)
    arr = (BbbItem * n)()
    for a in arr:
        a.mu = a.rho = a.eps = a.w = a.dmu = a.drho = t.data_ptr()
        a.n = 8
    kl, partial = torch.full((1,), 7.0), torch.full((64,), 7.0)
    assert hostsim.c.mlhot_bbb_sample_multi_fwd(arr, n, BC._P(partial), BC._P(kl), None) == ERR_ARG
    assert hostsim.c.mlhot_bbb_sample_multi_bwd(arr, n, BC._P(kl), None) == ERR_ARG
    assert b"bbb_sample_multi" in hostsim.c.mlhot_last_error()
    assert kl.item() == 7.0 and not t.any() and bool((partial == 7.0).all())
