"""tests/tail_cases.py without a GPU: the table against the arithmetic it claims, and every case through the host flavour of the
library (the operator chain of csrc/np_vanilla.h: all it has) against the float64 oracle under the library's own routing.  This
validates the table, the parameter builder, the oracle and the refusals at these widths before any GPU time is spent on them
(tests/test_tail_envelope_gpu.py)."""
import pytest

from tests import tail_cases as TC

NAMES = [c.name for c in TC.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_expected_family_follows_from_the_lds_arithmetic(name):
    c = TC.BY_NAME[name]
    assert TC.route(c) == c.family, (name, TC.lds_bytes(c))


def test_edge_pairs_stand_on_both_sides_of_their_bound():
    """Each `fits` / `does not` pair differs in one width, the fitting one is the LAST that fits in the kernels' 16-column
    granularity, and the launch that decides is the one the table names."""
    def worst(name):
        need = TC.lds_bytes(TC.BY_NAME[name])
        k = max(need, key=need.get)
        return k, need[k]
    for fits, over, launch in (("attn_m416", "attn_m417", "tail.bwd.B"), ("attn_dw128_fused", "attn_dw128_m225", "tail.bwd.B"),
                               ("attn_wide_hidden_fits", "attn_wide_hidden", "tail.bwd.A"), ("cnp_wide_hidden_fits", "cnp_wide_hidden", "tail.bwd.cnp")):
        (kf, bf), (ko, bo) = worst(fits), worst(over)
        assert kf == ko == launch and bf <= TC.LDS_LIMIT < bo, (fits, over, kf, bf, ko, bo)
    # the issue's table: phase B' at dim_w 64 / m 266, 416, 417 and dim_w 128 / m 621; the forward's phase B at dim_w 128 / m 621 fits
    b = TC.BY_NAME["attn_distinct"]
    assert [TC.attention_lds(b._replace(m_feat=m))["tail.bwd.B"] for m in (266, 416, 417)] == [125312, 162176, 166272]
    dw128 = TC.attention_lds(TC.BY_NAME["attn_dw128"])
    assert dw128["tail.bwd.B"] == 264576 and dw128["tail.B"] == 131648 <= TC.LDS_LIMIT
    # dim_w 192: only the key-head block's tile count keeps it off the fused kernels
    c = TC.BY_NAME["attn_dw192_m32"]
    assert max(TC.attention_lds(c).values()) <= TC.LDS_LIMIT and c.dim_w > TC.KEYHEAD_MAX_DW and c.dim_w % 64 == 0


def test_every_width_of_the_distinct_cases_differs():
    """attn_distinct / cnp_distinct_mean: the model's widths differ from each other.  Their row strides do not (80 = dim_w + dim_w / 4 =
    hidden[0] and 112 = dim_w + dim_z = hidden[1]; 88 = dim_w + dim_z = hidden[1]): the *_rows cases keep those apart as well."""
    a = TC.BY_NAME["attn_distinct"]
    widths = [a.dim_w, a.dim_z, *a.hidden, a.dec_hidden, a.m_feat, a.label_dim, a.y_dim]
    assert len(set(widths)) == len(widths), widths
    a = TC.BY_NAME["attn_distinct_rows"]
    widths = [a.dim_w, a.dim_w // 4, a.dim_w + a.dim_w // 4, a.dim_z, a.dim_w + a.dim_z, *a.hidden, a.dec_hidden, a.m_feat, a.label_dim, a.y_dim]
    assert len(set(widths)) == len(widths), widths
    p = TC.BY_NAME["cnp_distinct_mean"]
    widths = [p.dim_w, p.dim_r, p.dim_z, *p.hidden, p.dec_hidden, p.label_dim, p.y_dim]
    assert len(set(widths)) == len(widths), widths
    p = TC.BY_NAME["cnp_distinct_rows"]
    widths = [p.dim_w, p.dim_w // 4, p.dim_w + p.dim_w // 4, p.dim_r, p.dim_z, p.dim_w + p.dim_z, *p.hidden, p.dec_hidden, p.label_dim, p.y_dim]
    assert len(set(widths)) == len(widths), widths
    b = TC.BY_NAME["baco_distinct"]
    assert len({b.dim_w, b.dim_r, b.dim_z}) == 3
    assert len(TC.BY_NAME["hidden1"].hidden) == 1 and len(TC.BY_NAME["hidden_max"].hidden) == TC.MAX_HIDDEN


@pytest.mark.parametrize("name", NAMES)
def test_host_chain_vs_float64_oracle(hostsim, name):
    c = TC.BY_NAME[name]
    got = TC.run(hostsim, c, "cpu")
    ref = TC.oracle(c, got["routes"])
    TC.compare(c, got, ref, "host chain")
    if TC.qk_live(c):
        # a condition on the INPUTS: the float64 oracle alone, under its OWN routing, has first-class query / key gradients
        share = TC.qk_share(TC.oracle(c)["grads"])
        assert share > TC.QK_MIN, f"{name}: attention not sharp enough: query / key gradients at {share:.1e} of the largest - change the seed"


@pytest.mark.parametrize("name,case,code,word", TC.REFUSALS, ids=[r[0] for r in TC.REFUSALS])
def test_refusals_name_the_width(hostsim, name, case, code, word):
    rc, msg = TC.refusal(hostsim, case)
    assert rc == code and word in msg, (rc, msg)


def test_flat_layout_at_distinct_widths_is_dense_and_ordered(hostsim):
    """mlhot_np_grads_flat_layout at widths that all differ: every gradient gets a 4-float aligned range of its own size, no two
    overlap, and the total is their end (an offset computed from the wrong width would overlap or overrun)."""
    for name in ("attn_distinct", "cnp_distinct_mean", "baco_distinct", "hidden_max"):
        c = TC.BY_NAME[name]
        total, offs = hostsim.np_grads_layout(TC.dims_of(hostsim, c))
        p = TC.params(name)
        spans = sorted((offs[k], offs[k] + p[k].numel(), k) for k in offs)
        assert set(offs) == {k for k in p if "projection" not in k}
        assert all(lo % 4 == 0 for lo, _, _ in spans)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), name
        assert spans[-1][1] <= total <= spans[-1][1] + 3
