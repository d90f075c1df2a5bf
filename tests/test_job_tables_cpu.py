"""The case table of tests/job_table_cases.py, checked without a GPU: the float64 reference against plain double
torch.nn.functional.linear over an explicit cat, the restated argument checks of csrc/mlp_chain.h (check_chain, chain_backward,
check_multi) on every case and refusal, the block totals restated from the header comments, the coverage the table promises, and
the ReLU condition on every case's inputs (no pre-activation on a tie, so that no case needs a flip allowance)."""
import pytest
import torch
import torch.nn.functional as F

from tests import job_table_cases as J

CHAIN_IDS = [c.name for c in J.CHAIN_CASES]
MULTI_IDS = [t.name for t in J.MULTI_CASES]


def _close(a, b):
    return a.shape == b.shape and (a.numel() == 0 or float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())))


@pytest.mark.parametrize("c", J.CHAIN_CASES, ids=CHAIN_IDS)
def test_chain_reference_is_plain_linear_over_cat(c):
    d = J.chain_data(c)
    ref = J.chain_reference(c, d)
    leaves = dict(x0=d.x0.double().requires_grad_(True))
    h = leaves["x0"]
    for k, l in enumerate(c.layers):
        w = leaves[f"w{k}"] = d.w[k].double().requires_grad_(True)
        b = None
        if l.b:
            b = leaves[f"b{k}"] = d.b[k].double().requires_grad_(True)
        parts = [h]
        if l.side_w:
            s = leaves[f"side{k}"] = d.side[k].double().requires_grad_(True)
            parts = [s, h] if l.side_first else [h, s]
        pre = F.linear(torch.cat(parts, dim=-1), w, b)
        h = {"none": lambda t: t, "relu": F.relu, "tanh": torch.tanh}[l.act](pre)
        assert h.shape == (c.M, l.N) and _close(ref.y[k], h.detach()) and _close(ref.pre[k], pre.detach())
    (h * d.dy.double()).sum().backward()
    grad = lambda name: leaves[name].grad if leaves[name].grad is not None else torch.zeros_like(leaves[name])
    for k, l in enumerate(c.layers):
        assert _close(ref.dw[k], grad(f"w{k}"))
        assert (ref.db[k] is None) == (not l.b) and (not l.b or _close(ref.db[k], grad(f"b{k}")))
        want = l.side_w and l.dside
        assert (ref.dside[k] is not None) == bool(want)
        if want:
            assert _close(ref.dside[k], grad(f"side{k}") + (d.dside_prior[k].double() if l.dside_acc else 0.0))
    assert (ref.dx0 is not None) == c.dx0
    if c.dx0:
        assert _close(ref.dx0, grad("x0") + (d.dx0_prior.double() if c.dx0_acc else 0.0))


@pytest.mark.parametrize("t", J.MULTI_CASES, ids=MULTI_IDS)
def test_job_reference_is_plain_linear_over_cat(t):
    for j in t.jobs:
        d = J.job_data(j)
        ref = J.job_reference(j, d)
        x, x2, w, b = (v.double().requires_grad_(True) for v in (d.x, d.x2, d.w, d.b))
        pre = F.linear(torch.cat([x, x2], dim=-1), w, b if j.b else None)
        y = {"none": lambda v: v, "relu": F.relu, "tanh": torch.tanh}[j.act](pre)
        (y * d.dy.double()).sum().backward()
        grad = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
        assert y.shape == (j.M, j.N) and _close(ref.y, y.detach()) and _close(ref.dw, grad(w))
        assert (ref.db is None) == (not j.b) and (not j.b or _close(ref.db, grad(b)))
        assert (ref.dx is not None) == j.dx and (not j.dx or _close(ref.dx, grad(x) + (d.dx_prior.double() if j.acc else 0.0)))
        want2 = bool(j.K2 and j.dx2)
        assert (ref.dx2 is not None) == want2 and (not want2 or _close(ref.dx2, grad(x2) + (d.dx2_prior.double() if j.acc else 0.0)))


def test_relu_pre_activations_are_off_the_tie():
    """A condition on the inputs (the seeds of the case table), met by every case: the kernels' fp32 ReLU decisions then equal the
    reference's, and no comparison needs an allowance for a flipped decision."""
    for c in J.CHAIN_CASES:
        ref = J.chain_reference(c, J.chain_data(c))
        for k, l in enumerate(c.layers):
            assert l.act != "relu" or J.relu_margin_ok(ref.pre[k]), f"chain/{c.name} layer {k}: choose another seed"
    for t in J.MULTI_CASES:
        for i, j in enumerate(t.jobs):
            assert j.act != "relu" or J.relu_margin_ok(J.job_reference(j, J.job_data(j)).pre), f"multi/{t.name} job {i}: choose another seed"


def test_every_case_is_accepted_and_every_refusal_refused():
    for c in J.CHAIN_CASES:
        assert J.chain_refused(c, bwd=False) is None and J.chain_refused(c, bwd=True) is None, c.name
    for c, stage in J.CHAIN_REFUSALS:
        assert J.chain_refused(c, bwd=True) is not None, c.name
        assert (J.chain_refused(c, bwd=False) is not None) == (stage == "fwd"), c.name
    for t in J.MULTI_CASES:
        assert J.multi_refused(t, bwd=False) is None and (not t.bwd or J.multi_refused(t, bwd=True) is None), t.name
    for t, stage in J.MULTI_REFUSALS:
        assert J.multi_refused(t, bwd=True) is not None, t.name
        assert (J.multi_refused(t, bwd=False) is not None) == (stage == "fwd"), t.name
    # one refusal per rule, each for its own reason
    reasons = {c.name: J.chain_refused(c, bwd=True) for c, _ in J.CHAIN_REFUSALS}
    assert reasons["ref_M513"] == reasons["ref_5layers"] == reasons["ref_x0_unaligned"] == "bad argument"
    assert reasons["ref_inner_N6"] == "inner layer 0" and reasons["ref_K_mismatch"] == "layer 1 width" and reasons["ref_ldy_short"] == "layer 1"
    assert reasons["ref_ldg6"] == reasons["ref_ldg_short"] == "layer 0 g" and reasons["ref_lddy_short"] == "lddy"


def test_every_stride_is_larger_than_its_width():
    for c in J.CHAIN_CASES:
        if c.name == "tight":
            continue
        n_last = c.layers[-1].N
        assert c.ld["x0"] > c.K0 and c.off["x0"] == 4 and c.ld["dy"] > n_last and c.ld["dx0"] > c.K0 and c.ld["dx0"] % 2 == 1 and c.ld["dy"] % 2 == 1
        for k, l in enumerate(c.layers):
            assert c.ld[("y", k)] > l.N and c.ld[("y", k)] % 2 == 1 and c.ld[("g", k)] > l.N and c.ld[("g", k)] % 4 == 0 and c.ld[("side", k)] % 4 == 0
            assert not l.side_w or (c.ld[("side", k)] > l.side_w and c.ld[("dside", k)] % 2 == 1)
    for t in J.MULTI_CASES:
        for j in t.jobs:
            if t.name == "tight":
                continue
            assert j.ld["x"] > j.K1 and j.ld["y"] > j.N and j.ld["dy"] > j.N and j.ld["dx"] > j.K1 and j.off["x"] == 4 and j.off["dx"] == 4
            assert not j.K2 or (j.ld["x2"] > j.K2 and j.ld["dx2"] > j.K2)


def test_block_totals():
    """Restated from the header comments: chain_fwd / chain_dgrad = ceil(M / 16) workgroups; a weight-gradient job = ceil(N / 16) *
    ceil(K / 64) blocks, one job per layer and one per side, at most MAXJ; a table job = gdx * ceil(N / 16) forward blocks, gdx * ceil(K /
    16) + ceil(N / 16) * ceil(K / 64) backward blocks, gdx = ceil(M / 32)."""
    by = {c.name: c for c in J.CHAIN_CASES}
    assert all(len(J.chain_wgrad_jobs(c)) <= J.MAXJ for c in J.CHAIN_CASES)
    assert J.chain_wgrad_jobs(by["four_sides"]) == [(4, 8), (4, 8), (8, 12), (12, 12), (12, 16), (4, 16), (16, 5), (12, 5)]       # MAXJ, exactly
    assert J.chain_blocks(by["four_sides"]) == (2, 8)
    assert J.chain_blocks(by["one_M17_K260_N256_relu"]) == (2, 16 * 5)
    assert J.chain_blocks(by["one_M512_K8_N4"]) == (32, 1)
    assert J.chain_blocks(by["side1_first_w256"]) == (3, 1 + 1 + 4 + 1)
    assert J.chain_blocks(by["M0"]) == (0, 1 + 1 + 1 + 1 + 1)                     # no rows: the weight-gradient table still has its blocks
    tb = {t.name: t for t in J.MULTI_CASES}
    assert J.multi_blocks(tb["one_M1_K4_N4"], False) == [(0, 1)] and J.multi_blocks(tb["one_M1_K4_N4"], True) == [(0, 2)]
    # eight_shapes, forward: gdx 1 1 1 2 2 2 3 16 x column tiles 1 8 8 9 1 1 2 1
    assert J.multi_blocks(tb["eight_shapes"], False) == [(0, 1), (1, 8), (9, 8), (17, 18), (35, 2), (37, 2), (39, 6), (45, 16)]
    # ... backward: gdx * ceil(K / 16) + ceil(N / 16) * ceil(K / 64)
    assert [b for _, b in J.multi_blocks(tb["eight_shapes"], True)] == [1 + 1, 2 + 8, 4 + 8, 34 + 45, 66 + 9, 2 + 1, 3 + 2, 16 + 1]
    for name, kept_fwd in (("empty_first", 2), ("empty_middle", 2), ("empty_last", 2), ("empty_all", 0)):
        fwd, bwd = J.multi_blocks(tb[name], False), J.multi_blocks(tb[name], True)
        assert len(fwd) == kept_fwd and len(bwd) == 3 and all(b > 0 for _, b in bwd)
    for t in J.MULTI_CASES:
        firsts = [f for f, _ in J.multi_blocks(t, True)]
        assert firsts == sorted(set(firsts)), t.name                      # the lookup's `first` column is strictly increasing


def test_the_table_reaches_what_it_promises():
    cs = [c for c in J.CHAIN_CASES]
    assert {c.M for c in cs} >= {0, 1, 15, 16, 17, 33, 512}
    assert {c.layers[-1].N for c in cs} >= {1, 2, 3, 5, 17, 255, 256}
    assert {l.N for c in cs for l in c.layers[:-1]} >= {4, 12, 20, 128, 132, 144, 256}
    assert {l.K for c in cs for l in c.layers} >= {4, 8, 252, 256, 260, 512}
    assert {len(c.layers) for c in cs} == {1, 2, 3, 4}
    assert {(k, l.side_first) for c in cs for k, l in enumerate(c.layers) if l.side_w} == {(k, f) for k in range(4) for f in (0, 1)}
    assert {l.side_w for c in cs for l in c.layers} >= {0, 4, 12, 256}
    assert {(l.act, k + 1 == len(c.layers)) for c in cs for k, l in enumerate(c.layers) if len(c.layers) > 1} == {(a, e) for a in J.ACT_CODE for e in (False, True)}
    assert any(not c.dx0 and not any(l.side_w for l in c.layers) for c in cs)
    assert any(l.side_w and not l.dside for c in cs for l in c.layers) and any(not l.b for c in cs for l in c.layers)
    assert any(c.dx0_acc for c in cs) and any(l.dside_acc for c in cs for l in c.layers)
    for c in cs:                                                            # a width of its own for every layer
        widths = [c.K0] + [l.N for l in c.layers]
        assert len(set(widths[1:])) == len(widths) - 1 and all(a != b for a, b in zip(widths, widths[1:])), c.name
    js = [j for t in J.MULTI_CASES for j in t.jobs]
    bj = [j for t in J.MULTI_CASES if t.bwd for j in t.jobs]
    assert {len(t.jobs) for t in J.MULTI_CASES} >= {1, 2, 8}
    assert {j.M for j in js} >= {0, 1, 31, 32, 33, 63, 64, 65, 512} and {j.K for j in js} >= {4, 20, 64, 260, 516}
    assert {j.N for j in bj} >= {4, 124, 128, 132} and any(j.N % 4 for j in js)
    assert {(j.K1, j.K2, j.dx, j.dx2) for j in bj if j.K2} >= {(K1, K2, m["dx"], m["dx2"]) for K1, K2 in J.SEAMS for m in J.MODES}
    assert any(j.acc and j.K2 and j.dx2 for j in bj) and any(j.acc and not j.K2 for j in bj) and any(not j.b for j in bj)
    for t in J.MULTI_CASES:                                                 # distinct shapes inside a table
        shapes = [(j.M, j.K, j.N, j.K2) for j in t.jobs]
        assert len(set(shapes)) == len(shapes), t.name
