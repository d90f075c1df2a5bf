"""The aggregators' and the losses' functors in the host flavour of the library, called directly (tests/agg_loss_cases.py has the
cases, the inputs and the references): the twin of tests/test_agg_loss_envelope_gpu.py - the same cases and assertions wherever the
host flavour exports the entry.  It proves the functors' arithmetic and the references before the device run; the launch geometry
(run_foreach's clamp, reduce1_block's three regimes) is the device twin's.  The first tests check the INPUTS: conditions that make
float64 and fp32 select alike, each with no exception allowed."""
import pytest
import torch

from tests import agg_loss_cases as G

DEV = "cpu"
SELECTING = [c for c in G.LOSS_KINDS if c[0] in ("quaternion", "degree")]


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=G.ids)
def test_mean_inputs_sum_exactly_in_fp32(shape):
    """Every partial sum over the shots (in shot order, as both kernels add) survives the round trip through fp32."""
    rs, dr = G.mean_inputs(shape)
    sums = rs.double().cumsum(dim=1)
    assert torch.equal(sums.float().double(), sums)
    assert torch.equal((dr * 64).round(), dr * 64) and float(dr.abs().max()) <= 4.0 and float(rs.abs().max()) <= 4.0


@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=G.ids)
def test_max_inputs_tie_and_select_alike_in_fp32_and_float64(shape):
    rs, _ = G.max_inputs(shape)
    rows32, arg32 = G.first_greater_scan(rs)
    rows64, arg64 = G.first_greater_scan(rs.double())
    assert torch.equal(arg32, arg64) and torch.equal(rows32.double(), rows64)
    assert torch.equal(rows32[-1], rs.max(dim=1).values)
    if shape[1] >= 3:
        assert G.max_tie_fraction(rs) >= 0.5, G.max_tie_fraction(rs)
    if rs.numel() >= 64:
        neg_zero = (rs.view(torch.int32) == torch.tensor(-0.0).view(torch.int32)).any()
        assert bool(neg_zero) and bool((rs == 0.75).any()) and bool((rs == -1.5).any())


def _selecting_inputs():
    for case in SELECTING:
        for rows in G.LOSS_ROWS:
            yield case, rows, 1
        for rows in G.PREFIX_ROWS:
            for P in G.PREFIX_P:
                yield case, rows, P


def test_quaternion_inputs_select_alike_in_fp32_and_float64():
    """The branch of the minimum and every sign agree between torch fp32 and float64; |p - q| >= 0.5 and |sgn g_j - u_j| >= 0.02 in
    every row; both branches occur wherever there are two rows, every scale wherever there are three."""
    for case, rows, P in _selecting_inputs():
        if case[0] != "quaternion":
            continue
        mu, gt = G.loss_inputs(case, rows, P)
        b32, s32, gap32, m32 = G.quaternion_choices(mu, gt)
        b64, s64, gap64, m64 = G.quaternion_choices(mu.double(), gt.double())
        assert torch.equal(b32, b64) and torch.equal(s32.double(), s64), (rows, P)
        assert float(min(gap32.min(), gap64.min())) >= 0.5 and float(min(m32.min(), m64.min())) >= 0.02, (rows, P)
        if rows >= 2:
            assert bool(b64.any()) and bool((~b64).any())
        if rows >= 3:
            norms = mu.double().pow(2).sum(-1).sqrt()
            assert all(bool(((norms / s - 1).abs() < 1e-6).any()) for s in G.QUAT_SCALES)


def test_degree_inputs_select_alike_in_fp32_and_float64():
    """The fold and the winning wrap candidate agree between torch fp32 and float64 with a margin of >= 1 degree in every row;
    |cos a| <= 0.98; from 12 rows on every fold class (m[1] > 0, < 0, +0.0, -0.0) meets every winning candidate."""
    for case, rows, P in _selecting_inputs():
        if case[0] != "degree":
            continue
        mu, gt = G.loss_inputs(case, rows, P)
        assert gt.shape == (rows, case[2]) and float(mu[..., 0].abs().max()) <= 0.98
        f32, w32, m32 = G.degree_choices(mu, gt)
        f64, w64, m64 = G.degree_choices(mu.double(), gt.double())
        assert torch.equal(f32, f64) and torch.equal(w32, w64), (rows, P)
        assert float(min(m32.min(), m64.min())) >= 1.0, (rows, P)
        if rows >= 12:
            m1 = mu[0, :, 1]
            neg_zero = (m1.view(torch.int32) == torch.tensor(-0.0).view(torch.int32))
            klass = torch.where(neg_zero, 3, torch.where(m1 == 0, 2, torch.where(m1 < 0, 1, 0)))
            assert {(int(k), int(w)) for k, w in zip(klass, w64[0])} == {(k, w) for k in range(4) for w in range(3)}
            assert not bool(f64[0][klass >= 2].any()) and bool(f64[0][klass == 1].all())


def test_distractor_inputs_keep_their_distance():
    for rows in G.LOSS_ROWS:
        mu, gt = G.loss_inputs(("distractor", 2, 2), rows)
        assert float((mu.double() - gt.double()).pow(2).sum(-1).sqrt().min()) >= 1e-3
    mu, gt = G.loss_inputs(("distractor", 2, 2), 1025, equal_row=1024)
    assert int((mu[0] == gt).all(dim=-1).sum()) == 1


def test_baco_regimes_reach_their_regions():
    """The threshold regime has shots on both sides of softplus's threshold; in the deep regimes fp32 softplus is below the resolution
    of the 1e-5 floor or exactly 0 (var == 1e-5f) and expf(-lv) overflows."""
    import torch.nn.functional as F
    floor = torch.tensor(1e-5, dtype=torch.float32)
    for shape in G.BACO_SHAPES:
        lv = G.baco_inputs(shape, "threshold")[1]
        assert all(bool((lv == torch.tensor(v, dtype=torch.float32)).any()) for v in G.THRESHOLD_LV) and bool((lv.abs() < 3).any())
        assert bool((lv == 20.0).any()) and bool(((lv > 20.0) & (lv < 20.00001)).any())
        lv = G.baco_inputs(shape, "deep")[1]
        assert all(bool((lv == v).any()) for v in G.DEEP_LV) and bool((lv > -5).any())
        assert bool(((floor + F.softplus(lv)) == floor).any()) and bool(torch.isinf(torch.exp(-lv)).any())
        lv = G.baco_inputs(shape, "all_deep")[1]
        assert bool(((floor + F.softplus(lv)) == floor).all())


# ---- aggregators ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=G.ids)
def test_mean_bitwise(hostsim, shape):
    G.need(hostsim, "mlhot_agg_prefix_fwd")
    G.check_mean(hostsim, shape, DEV)


@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=G.ids)
def test_max_ties_bitwise(hostsim, shape):
    G.need(hostsim, "mlhot_agg_prefix_fwd")
    G.check_max(hostsim, shape, DEV)


@pytest.mark.parametrize("regime", G.BACO_REGIMES)
@pytest.mark.parametrize("shape", G.BACO_SHAPES, ids=G.ids)
def test_baco_vs_float64_per_column(hostsim, shape, regime):
    G.need(hostsim, "mlhot_agg_prefix_fwd")
    G.check_baco(hostsim, shape, regime, DEV)


@pytest.mark.parametrize("regime", G.BACO_REGIMES)
@pytest.mark.parametrize("shape", G.BACO_SHAPES, ids=G.ids)
def test_baco_prefix_rows_have_the_bits_of_agg_fwd(hostsim, shape, regime):
    G.need(hostsim, "mlhot_agg_prefix_fwd")
    G.check_prefix_rows_equal_agg_fwd(hostsim, "baco", shape, regime, DEV)


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_prefix_rows_have_the_bits_of_agg_fwd(hostsim, mode):
    G.need(hostsim, "mlhot_agg_prefix_fwd")
    G.check_prefix_rows_equal_agg_fwd(hostsim, mode, G.PREFIX_SHAPE, "-", DEV)


def test_agg_refusals(hostsim):
    G.need(hostsim, "mlhot_agg_fwd")
    G.check_agg_refusals(hostsim, DEV)


# ---- losses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", G.LOSS_ROWS)
@pytest.mark.parametrize("case", G.LOSS_KINDS, ids=G.ids)
def test_loss_value_and_gradient_vs_float64(hostsim, case, rows):
    G.need(hostsim, "mlhot_loss_fwd")
    G.check_loss(hostsim, case, rows, DEV)


@pytest.mark.parametrize("P", G.PREFIX_P)
@pytest.mark.parametrize("rows", G.PREFIX_ROWS)
@pytest.mark.parametrize("case", G.LOSS_KINDS, ids=G.ids)
def test_loss_prefix_vs_float64_and_loss_fwd(hostsim, case, rows, P):
    G.need(hostsim, "mlhot_loss_prefix_fwd")
    G.check_loss_prefix(hostsim, case, rows, P, DEV)


def test_distractor_row_with_mu_equal_gt(hostsim):
    G.need(hostsim, "mlhot_loss_fwd")
    G.check_distractor_equal_row(hostsim, DEV)


@pytest.mark.parametrize("rows", G.PLUS_ROWS)
@pytest.mark.parametrize("case", G.TRAIN_KINDS, ids=G.ids)
def test_loss_plus_has_the_bits_of_loss_and_axpy(hostsim, case, rows):
    G.need(hostsim, "mlhot_loss_plus_fwd")
    G.check_loss_plus(hostsim, case, rows, DEV)


def test_loss_refusals(hostsim):
    G.need(hostsim, "mlhot_loss_fwd")
    G.check_loss_refusals(hostsim, DEV)
