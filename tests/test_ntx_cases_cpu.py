"""tests/ntx_cases.py checked on the CPU: the vectorised float64 reference against the pair-by-pair definition, the table's inputs
against the condition that makes the GPU test able to see a wrong partial column block, and a float64 model of that defect against the
GPU test's gradient bar.  No GPU."""
import pytest
import torch

from oracle import ref_cpu as O
from tests import ntx_cases as NC
from tests import util as U

PARTIAL = [c for c in NC.CASES if c.d % 64 and not c.zero]
# the partial column block's wrong rows are the tile rows >= (d % 64) / 4 = 4 at d = 80: a case of 3 rows has none of them
NO_ROW_IN_THE_BLOCK = ["N3_d80_mod2"]


def test_the_table_covers_what_it_says():
    by = {}
    for c in NC.CASES:
        by.setdefault((c.N, c.div, c.mod, c.t, c.gscale, c.recipe), set()).add(c.d)
    assert by[(37, 1, 5, 0.07, 1.0, "randn")] >= {16, 32, 48, 64, 80, 112, 128, 144, 192, 208, 240, 256}
    assert all({16, 80, 240} <= by[(N, 1, 5, 0.07, 1.0, "randn")] for N in (16, 17))
    assert {c.N for c in NC.CASES if c.d == 80 and c.mod == 2} == {2, 3, 15, 16, 17, 31, 32, 33, 64, 65}
    assert [c.name for c in NC.CASES if c.zero] == ["N2_mod1_exact_zero", "N2_mod2_exact_zero"]
    assert sorted(c.N for c in NC.CASES if c.N > 65) == [2033, 2048]
    assert U.RTOL == 1e-4 and NC.rel_err(torch.tensor([1.0, 2.5]), torch.tensor([1.0, 2.0])) == U.rel_err(torch.tensor([1.0, 2.5]), torch.tensor([1.0, 2.0]))
    for c in NC.CASES:
        assert 1 <= c.N <= 2048 and 16 <= c.d <= 256 and c.d % 16 == 0 and c.div >= 1 and c.mod >= 1 and c.t > 0
        assert 4 * (16 * (c.d + 4) + 16 * ((c.N + 15) // 16 * 16 + 4) + (c.N + 15) // 16 * 16 + 64) <= 160 * 1024      # ntx::lds_bytes
        r = NC.reference(c)
        assert (r.pairs == 0) == c.zero, c.name
        if c.zero:
            assert r.loss.item() == 0.0 and not r.dz.any()
        elif c.gscale != 0.0:
            assert r.dz.abs().max().item() > 0.0, c.name
        if c.bits_of:
            assert torch.equal(NC.labels(c), NC.labels(NC.BY_NAME[c.bits_of])) and torch.equal(NC.inputs(c.name), NC.inputs(c.bits_of))
    lab = NC.labels(NC.BY_NAME["lab_wrap"]).tolist()
    assert lab[:10] == [0, 0, 1, 1, 2, 2, 3, 3, 0, 0]
    assert sorted(NC.labels(NC.BY_NAME["lab_unequal"]).bincount().tolist()) == [10, 15, 20]
    assert NC.labels(NC.BY_NAME["lab_all_but_one"]).bincount().tolist() == [44, 1]
    z = NC.inputs("deg_tiny_row")
    assert 0.0 < z[NC.DEGENERATE_ROW].double().norm().item() < NC.NORM_FLOOR
    for recipe, (a, b) in NC.TWIN_ROWS.items():
        c = NC.BY_NAME["deg_" + recipe]
        assert torch.equal(NC.inputs(c.name)[a], NC.inputs(c.name)[b])
        assert (NC.labels(c)[a] == NC.labels(c)[b]) == (recipe == "twins_same_label")
    n = NC.inputs("deg_six_decades").double().norm(dim=1)
    assert n.max() / n.min() >= 1e6


@pytest.mark.parametrize("case", NC.SMALL, ids=[c.name for c in NC.SMALL])
def test_oracle_against_the_pair_by_pair_definition(case):
    """ref (O(N^2) tensor arithmetic) against oracle.ref_cpu.nt_xent (one autograd node per pair) in float64: the loss to 1e-12
    relative, gscale x the autograd gradient to 1e-10 (zero / 1e-20 rows against their own scale)."""
    c = case
    r = NC.reference(c)
    z = NC.inputs(c.name).double().requires_grad_()
    want = O.nt_xent(z, NC.labels(c).tolist(), c.t)
    (want * c.gscale).backward()
    assert abs(r.loss.item() - want.item()) <= 1e-12 * abs(want.item()), (r.loss.item(), want.item())
    if c.zero or c.gscale == 0.0:
        assert not r.dz.any() and not z.grad.any()
    else:
        assert NC.dz_err(c, r.dz, z.grad) <= 1e-10
    # the two-step form the defect model is built on (dL/dzn, then the normalisation's backward) is the same gradient
    clean = NC._norm_backward(NC.inputs(c.name).double(), r.rinv[:, None], r.dzn)
    assert NC.dz_err(c, clean, r.dz) <= 1e-10 or c.zero or c.gscale == 0.0


@pytest.mark.parametrize("case", PARTIAL, ids=[c.name for c in PARTIAL])
def test_partial_block_is_live_and_the_gradient_bar_sees_the_defect(case):
    """For every case with d % 64 != 0 and a gradient: the reference gradient on the partial column block (columns >= 64 floor(d / 64),
    tile rows >= (d % 64) / 4) reaches 1e-2 of the whole gradient's largest entry - a condition on the inputs - and a backward that
    loses those anchors' rows of the product (ntx_cases.defect_model) is outside the GPU test's bar, dz_err <= util.RTOL."""
    c = case
    pb = NC.partial_block(c)
    if c.name in NO_ROW_IN_THE_BLOCK:
        assert pb is None and c.N <= (c.d % 64) // 4
        return
    assert pb is not None
    r = NC.reference(c)
    if c.gscale == 0.0:
        assert not r.dz.any()              # nothing to see: the GPU test asks for exact zeros here
        return
    rows, c0 = pb
    share = r.dz[rows, c0:].abs().max().item() / r.dz.abs().max().item()
    err = NC.dz_err(c, NC.defect_model(c), r.dz)
    print(f"ntx_cases {c.name}: partial block share {share:.2e}, defect model dz_err {err:.2e}")
    assert share >= 1e-2, (c.name, share)
    assert err > U.RTOL, (c.name, err)


def test_lds_limit_references_are_finite_and_consistent():
    """The two cases above 65 rows have no pair-by-pair check: their dz from ref and from the two-step form agree, and stay unchanged
    between calls (the reference is computed once and shared)."""
    for name in ("lds_2048_256", "lds_2033_240"):
        c = NC.BY_NAME[name]
        r = NC.reference(c)
        assert r is NC.reference(c)
        assert bool(torch.isfinite(r.dz).all()) and r.loss.item() > 0.0
        clean = NC._norm_backward(NC.inputs(name).double(), r.rinv[:, None], r.dzn)
        assert NC.dz_err(c, clean, r.dz) <= 1e-10
