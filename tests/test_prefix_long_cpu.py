"""The prefix sweep beyond 32 context shots without a GPU: the float64 restatement of the chunked walk
(tests/prefix_long_ref.py) against the per-prefix definition on every input of the GPU tests, the denominators those tests will
divide by, ks validation, lens saturation, split ks, and what the host build says."""
import ctypes as C
import math

import pytest
import torch

from tests import favor_cached_ref as R
from tests import prefix_long_ref as L
from tests import prefix_ref as PR

TIGHT = 1e-12            # float64 restatement against float64 definition, of out's scale


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def _check_denominators(den, what):
    assert bool(torch.isfinite(den).all()) and den.min().item() > 0.0, f"{what}: a float64 denominator is zero or not finite"


# ---- 1. the restatement equals the definition on every input the GPU tests use -----------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("Nc", L.NCS)
@pytest.mark.parametrize("d,m", L.SHAPES)
def test_streamed_equals_the_per_prefix_definition(d, m, Nc, kind):
    c = L.case(kind, d, m, Nc)
    out, den = L.reference(kind, d, m, Nc)
    _check_denominators(den, f"{kind} d={d} m={m} Nc={Nc}")
    assert bool(torch.isfinite(out).all())
    ks = L.ks_sets(Nc)["all"]
    want, wden = L.direct(c["q"], c["k"], c["v"], c["proj"], ks)
    _check_denominators(wden, f"{kind} d={d} m={m} Nc={Nc} (definition)")
    err = _rel(out[[k - 1 for k in ks]], want)
    assert err <= TIGHT, f"{kind} d={d} m={m} Nc={Nc}: {err:.2e}"
    # ... and the definition is the existing reference on the sliced context
    for k in {1, Nc, min(33, Nc)}:
        plain = R.attention(c["q"], c["k"][:, :, :k], c["v"][:, :, :k], c["proj"])
        assert _rel(want[ks.index(k)], plain) <= TIGHT, (kind, d, m, Nc, k)


def test_the_definition_is_prefix_refs_on_a_small_case():
    c = L.case("peak_last", 16, 16, 65)
    want = torch.from_numpy(PR.favor_prefixes_np(c["q"], c["k"], c["v"], c["proj"]))
    got, _ = L.direct(c["q"], c["k"], c["v"], c["proj"], range(1, 66))
    assert _rel(got, want) <= TIGHT
    run = torch.cummax(L.shot_maxima(c["k"], c["proj"]), dim=0).values
    assert _rel(run, torch.from_numpy(PR.favor_stabilisers_np(c["k"], c["proj"]))) <= TIGHT
    assert run[L.peak_shot(65)] - run[L.peak_shot(65) - 1] > 40.0            # the rescale path runs: the stabiliser jumps in the last chunk


# ---- 2. lens: saturation, the stabiliser over every task's valid shots -------------------------------------------------------------
@pytest.mark.parametrize("Nc,lens", [(Nc, lens) for Nc, many in L.LENS.items() for lens in many])
@pytest.mark.parametrize("d,m", L.SHAPES[:2])
def test_lens_saturate_and_the_walk_agrees(d, m, Nc, lens):
    c = L.case("live", d, m, Nc)
    ks = L.ks_sets(Nc)["all"]
    out, den = L.streamed(c["q"], c["k"], c["v"], c["proj"], ks, lens)
    _check_denominators(den, f"lens {lens}")
    want, _ = L.direct(c["q"], c["k"], c["v"], c["proj"], ks, lens)
    assert _rel(out, want) <= TIGHT
    dd = torch.einsum("thnd,md->thnm", d ** -0.25 * c["k"].double(), c["proj"].double())
    for t, n in enumerate(lens):
        if n < Nc:        # behind lens[t] only the stabiliser moves: the task's output is its first lens[t] shots under M_k
            k = Nc
            Mk = max(dd[u, :, :min(k, lens[u])].max().item() for u in range(L.T))
            fk = m ** -0.5 * (torch.exp(dd[t, :, :n] - (c["k"][t, :, :n].double() ** 2).sum(-1, keepdim=True) * 0.5 * d ** -0.5 - Mk) + L.EPS)
            Sm = torch.einsum("hqm,hnm->hqn", R.query_features(c["q"], c["proj"])[t], fk)
            sat = torch.einsum("hqn,hne->hqe", Sm, c["v"][t, :, :n].double()) / Sm.sum(-1, keepdim=True)
            assert _rel(out[k - 1, t], sat) <= TIGHT
    # rows behind lens[t] do not matter
    k2, v2 = c["k"].clone(), c["v"].clone()
    for t, n in enumerate(lens):
        k2[t, :, n:], v2[t, :, n:] = 1e3, -1e3
    again, _ = L.streamed(c["q"], k2, v2, c["proj"], ks, lens)
    assert torch.equal(again, out)


# ---- 3. splitting ks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["live", "peak_last"])
def test_splitting_ks_is_consistent(kind):
    c = L.case(kind, 64, 266, 97)
    ks = L.ks_sets(97)["all"]
    whole, _ = L.streamed(c["q"], c["k"], c["v"], c["proj"], ks)
    parts = [L.streamed(c["q"], c["k"], c["v"], c["proj"], ks[i:i + 64])[0] for i in (0, 64)]
    assert torch.equal(torch.cat(parts), whole)
    some = L.ks_sets(97)["edges"]
    assert torch.equal(L.streamed(c["q"], c["k"], c["v"], c["proj"], some)[0], whole[[k - 1 for k in some]])


# ---- 4. ks and lens validation (host work: nothing touches a GPU) ---------------------------------------------------------------------
def test_ks_validation():
    from mlhot.binding import MlhotError
    from mlhot.ops import PREFIX_LONG_MAX_K, prefix_sizes
    assert PREFIX_LONG_MAX_K == 64
    assert prefix_sizes(None, 5, "x") == (1, 2, 3, 4, 5)
    assert prefix_sizes(torch.tensor([1, 33, 40]), 40, "x") == (1, 33, 40)
    for bad in ([], [0, 1], [1, 41], [3, 3], [4, 2], [1.0, 2], [True, 2], 7, torch.tensor([1.0]), torch.tensor([[1, 2]])):
        with pytest.raises(MlhotError, match="x: ks must"):
            prefix_sizes(bad, 40, "x")
    with pytest.raises(ValueError, match="ks must"):
        prefix_sizes([2, 1], 40, "x", exc=ValueError)


def test_the_op_refuses_on_the_host_before_it_needs_a_gpu():
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_prefixes_long
    q, k, proj = torch.zeros(2, 3, 8, 16), torch.zeros(2, 40, 8, 16), torch.zeros(16, 16)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_prefixes_long(q.requires_grad_(), k, k, proj)
    with pytest.raises(MlhotError):                     # CPU tensors: the op is GPU only
        favor_prefixes_long(q.detach(), k, k, proj)


# ---- 5. the host build ---------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_three_entries_and_they_are_unsupported(hostsim):
    c = hostsim.c
    assert hostsim.missing == set()
    assert c.mlhot_favor_prefix_long_supported(2, 8, 5, 40, 64, 266, 4) == 0
    assert c.mlhot_favor_prefix_long_workspace_bytes(2, 8, 5, 40, 64, 266, 4) == 0
    assert not hostsim.favor_prefix_long_supported(2, 8, 5, 40, 64, 266, 4)
    q, k = torch.zeros(2, 5, 8, 64), torch.zeros(2, 40, 8, 64)
    proj, out, ws = torch.zeros(266, 64), torch.full((4, 2, 5, 512), 7.0), torch.zeros(1 << 10)
    ks = (C.c_int32 * 4)(1, 32, 33, 40)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = c.mlhot_favor_prefix_long_fwd(p(q), p(k), p(k), p(proj), ks, 4, None, 2, 8, 5, 40, 64, 266, p(out), p(ws), 4 * ws.numel(), None)
    assert rc == 4 and bool((out == 7.0).all())                                   # MLHOT_ERR_UNSUPPORTED, nothing written
    from mlhot.binding import MlhotError
    with pytest.raises(MlhotError, match="favor_prefix_long_fwd serves"):
        hostsim.favor_prefix_long_fwd(q, k, k, proj, [1, 32, 33, 40])


def test_ks_sets_and_the_peak_sit_where_the_tests_say():
    assert L.ks_sets(97)["edges"] == [1, 31, 32, 33, 63, 64, 65, 95, 96, 97]
    assert L.ks_sets(31)["1_32_33_Nc"] == [1, 31] and L.ks_sets(65)["1_32_33_Nc"] == [1, 32, 33, 65]
    assert [L.peak_shot(n) for n in (1, 32, 33, 64, 65, 97)] == [0, 1, 32, 33, 64, 96]
    assert math.isinf(L.shot_maxima(L.case("live", 16, 16, 33)["k"], L.case("live", 16, 16, 33)["proj"], (1, 1))[5].item())
