"""tests/conv_cases.py is fit to judge a kernel, shown on the host flavour of the library (the same ConvFwdRT / ConvDgradRT /
ConvWgradRT functors' A / B / store in a plain loop) before a GPU is involved: every case takes the route the table states, the table
reaches every edge of conv_rt.h's and igemm.h's host decisions, the exact pass returns the float64 reference's bits, the real pass is
inside the bound, and the bound's own conditions hold (integer range; 2 x e32 <= tol, so the bound never more than doubles).

Measured here over the table (both ReLU settings): the largest e32 = rel_err(torch float32 on the CPU, float64) is 7.0e-07 for y,
3.4e-07 for dx, 7.9e-07 for dw and 2.2e-07 for db, so the largest bounds tol + 2 e32 are 1.14e-05 (y), 2.07e-05 (dx), 2.16e-05 (dw) and
2.04e-05 (db); the host flavour itself (one fma chain per k chunk of the requested split, the chunks summed in order, as the device
does) is at most 8.5e-07 (y), 8.2e-07 (dx), 4.5e-07 (dw), 9.3e-07 (db) off the float64 reference on the real inputs, and no ReLU decision
of it differs from the float64 sign."""
import os
import re

import pytest
import torch

from tests import conv_cases as CC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "what-matters-for-meta-learning_amd", "csrc")


def test_cases_take_the_route_the_table_names(hostsim):
    """The literals of the table against route(), route()'s constants against the sources, and the requested split against the one
    number the library exposes: (mlhot_conv2d_bwd_scratch_bytes - 256) / (4 Cout (Cin k k + 1))."""
    conv_rt, igemm = open(os.path.join(CSRC, "conv_rt.h")).read(), open(os.path.join(CSRC, "igemm.h")).read()
    assert re.search(r"#define MLHOT_CONV_BK (\d+)", conv_rt).group(1) == str(CC.CONV_BK)
    assert re.search(r"#define MLHOT_CONV_BM (\d+)", conv_rt).group(1) == "128"
    assert conv_rt.count("if (wgs64 < 128) return run_igemm<P, 16, 64, CONV_BK, 1, 4>") == 1
    assert conv_rt.count("const int rc = wgs64 < 128 ? run_igemm_batch<ConvDgradRT, 16, 64, CONV_BK, 1, 4>") == 1
    assert conv_rt.count("if (batch.n == 4) MLHOT_TRY(flush());") == 1 and "IgemmBatch { P p[4]; int n; }" in igemm
    assert "long want = (512 + tiles - 1) / tiles;" in conv_rt and "long maxs = pos / 64;" in conv_rt and "if (want > 256) want = 256;" in conv_rt
    assert "k_chunk = (k_chunk + BK - 1) / BK * BK;" in igemm and "nsplit = (p.K + k_chunk - 1) / k_chunk;" in igemm
    for c in CC.CASES:
        r = CC.route(c.shape)
        assert (c.fwd, c.dgrad, c.wgrad) == (r.fwd, r.dgrad, r.wgrad), (c.name, r.fwd, r.dgrad, r.wgrad)
        sb = hostsim.c.mlhot_conv2d_bwd_scratch_bytes(*c.shape)
        per_split = 4 * c.Cout * (c.K + 1)
        assert (sb - 256) % per_split == 0 and (sb - 256) // per_split == c.wgrad[0], (c.name, sb)


def test_table_reaches_every_edge():
    """Asserted over the table, so that a later edit cannot silently drop an edge."""
    R = {c.name: CC.route(c.shape) for c in CC.CASES}
    cases = CC.CASES
    some = lambda f: any(f(c, R[c.name]) for c in cases)
    # forward: both tiles, the two shapes next to the switch, K below / at / above one k tile, a second N tile on either side
    assert {c.fwd for c in cases} >= {(16, 127), (128, 128)}
    assert some(lambda c, r: c.fwd[0] == 128 and c.pos % 128 != 0)
    assert {1, 27, 75} <= {c.K for c in cases} and some(lambda c, r: c.K % 32 == 0)
    assert some(lambda c, r: c.Cout == 65 and c.fwd == (16, 126)) and some(lambda c, r: c.Cout == 65 and c.fwd == (128, 128))
    # data gradient: a second N tile on either tile, every batch pattern, both sides of the switch decided by the sum alone
    assert some(lambda c, r: c.Cin > 64 and c.dgrad[3] == ((1, 16),)) and some(lambda c, r: c.Cin > 64 and c.dgrad[3] == ((1, 128),))
    patterns = {c.dgrad[3] for c in cases}
    assert {((1, 16),), ((1, 128),), ((4, 16),), ((4, 128),), ((4, 128), (4, 128), (1, 16)), ((4, 16),) * 4} <= patterns
    for total, tile in ((128, 128), (124, 16)):
        assert some(lambda c, r: c.dgrad[3] == ((4, tile),) and sum(k.wgs for k in r.classes) == total and max(k.wgs for k in r.classes) < 128)
    assert some(lambda c, r: c.dgrad[1] > 0 and c.k > 1) and some(lambda c, r: c.dgrad[1] > 0 and c.k == 1) and some(lambda c, r: c.dgrad[2] > 0)
    assert some(lambda c, r: c.s == 4) and {2, 4} <= {c.k for c in cases} and some(lambda c, r: c.p >= c.k) and some(lambda c, r: c.H < c.s)
    assert some(lambda c, r: (c.H + 2 * c.p - c.k) % c.s != 0)
    # p = 0 and the last input row and column lie behind the last tap of the last output
    assert some(lambda c, r: c.p == 0 and (c.HO - 1) * c.s + c.k - 1 < c.H - 1 and (c.WO - 1) * c.s + c.k - 1 < c.W - 1)
    for s in (2, 3):
        assert some(lambda c, r: c.s == s and c.H > c.W) and some(lambda c, r: c.s == s and c.H < c.W)
    # weight gradient: the split at pos = 63, 64, 127, 128; 9 -> 9 and 9 -> 7 with a partial last chunk; the cap; 171; tiles bind
    split_at = {c.pos: c.wgrad for c in cases if c.pos in (63, 64, 127, 128, 576, 600)}
    assert split_at == {63: (1, 1), 64: (1, 1), 127: (1, 1), 128: (2, 2), 576: (9, 9), 600: (9, 7)}
    assert some(lambda c, r: c.pos == 600 and r.k_chunk == 96 and r.last_chunk == 24)
    assert some(lambda c, r: c.wgrad == (256, 256) and c.pos // 64 >= 256 and r.tiles == 1)
    assert some(lambda c, r: c.wgrad == (255, 171)) and some(lambda c, r: c.wgrad[1] > 8 and c.wgrad[1] % 8 != 0)
    assert some(lambda c, r: c.wgrad[1] > 1 and r.last_chunk < r.k_chunk) and some(lambda c, r: c.wgrad[0] != c.wgrad[1])
    assert some(lambda c, r: c.Cout > 64 and c.wgrad[0] > 1) and some(lambda c, r: c.Cout > 64 and c.wgrad[0] == 1)
    assert some(lambda c, r: r.tiles > 1 and c.wgrad[0] == -(-512 // r.tiles) < min(c.pos // 64, 256))
    assert some(lambda c, r: r.bias_col == 63) and some(lambda c, r: r.bias_col == 0 and c.k == 1) and some(lambda c, r: r.bias_col == 0 and c.k == 4)
    assert all(c in cases for c in CC.TWICE + CC.BANDED) and [c.wgrad[1] for c in CC.TWICE] == [256, 171, 7]
    # small: the host flavour's triple loop stays well under a second per GEMM
    assert all(c.pos * c.Cout * (c.K + 1) <= 10.5e6 for c in cases)


@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_bound_conditions(name):
    """Exact pass: 9 x (the longest reduction of the three GEMMs) + 3 < 2^24 and the inputs are the integers the rule is about.  Real
    pass: 2 x e32 <= tol for y, dx, dw, db and both ReLU settings."""
    c = CC.BY_NAME[name]
    assert 9 * CC.route(c.shape).max_K + 3 < 2 ** 24
    i = CC.inputs(name, "exact")
    for t in (i.x, i.w, i.b, i.dy):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max().item() <= 3
    for relu in (False, True):
        e, b = CC.e32(c, relu), CC.bounds(c, relu)
        print(f"conv_cases {name} relu={int(relu)} e32: " + " ".join(f"{n}={e[n]:.2e}" for n in CC.NAMES)
              + " bound: " + " ".join(f"{n}={b[n]:.2e}" for n in CC.NAMES))
        for n in CC.NAMES:
            assert 2.0 * e[n] <= CC.TOL[n], (name, relu, n, e[n])


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_exact_pass_on_hostsim(hostsim, name, relu):
    c = CC.BY_NAME[name]
    CC.judge(c, "exact", relu, CC.run(hostsim, c, "exact", relu), what="hostsim", log=print)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_real_pass_on_hostsim(hostsim, name, relu):
    c = CC.BY_NAME[name]
    CC.judge(c, "real", relu, CC.run(hostsim, c, "real", relu), what="hostsim", log=print)


@pytest.mark.parametrize("name", ["N1_C2_6x8_O3_k3_s2_p0", "N1_C2_20x30_O3_k3_s1_p1"])
def test_optional_operands_on_hostsim(hostsim, name):
    """No bias (b and db NULL) and no data gradient (dx NULL), exact pass: what is left equals the reference of that call."""
    c = CC.BY_NAME[name]
    for relu in (False, True):
        got = CC.run(hostsim, c, "exact", relu, bias=False)
        assert got["db"] is None
        CC.judge(c, "exact", relu, got, bias=False, what="hostsim no bias", log=print)
        got = CC.run(hostsim, c, "exact", relu, need_dx=False)
        assert got["dx"] is None
        CC.judge(c, "exact", relu, got, what="hostsim no dx", log=print)


def test_argument_refusals_on_hostsim(hostsim):
    CC.check_refusals(hostsim, "cpu")
