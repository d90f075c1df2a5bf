"""Per-target context masks on the MI355X, ops level: mlhot_favor_query_masked_fwd and
mlhot_favor_query_long_masked_fwd through mlhot.ops.favor_query(mask=) - all ones bit-equal to the unmasked entry, every pattern
against float64, the dominant-shot leave-one-out, row and group invariance, w's zeros and row sums, out with w bit-equal to out
without, the empty row, the envelope and the NULL mask.  Shapes, patterns and float64 references: tests/context_mask_cases.py.
Run with -m gpu.

The bars are those of the unmasked tests of the same kernels (tests/test_attention_readout_gpu.py, tests/test_favor_long_gpu.py):
U.RTOL of the tensor's scale for out and w, Nc 2^-23 for the row sum of w.  A masked sum is a sub-sum of the same terms: no extra
margin.  The worst figures of a run are in profiles/INDEX_context_mask.md."""
import ctypes as C

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import context_mask_cases as CC
from tests import context_mask_ref as CM
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H, NQ = CC.T, CC.H, CC.NQ


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _state(route, kd, pd, lens):
    from mlhot.ops import favor_keys, favor_keys_long
    state = favor_keys_long(kd, pd, lens=list(lens)) if route == "long" else favor_keys(kd, pd, lens=None if lens is None else list(lens))
    assert state.route == route
    return state


def _setup(shape):
    route, Nc, lens, d, m = shape
    q, k, v, p = CC.inputs(Nc, d, m)
    qd, vd, pd = _dev(q), _dev(v), p.to(DEV)
    return qd, _state(route, _dev(k), pd, lens), vd, pd


def _check_w(w, mk, lens, Nc, line):
    """masked columns exactly 0, kept entries >= 0, rows that keep a valid slot sum to 1, the others are zeros, nothing is NaN"""
    from tests import ragged_ref as RR
    keep = (mk & RR.valid_mask(lens, Nc)[:, None, None, :]).to(w.device)[:, :, None].expand_as(w)
    assert bool(torch.isfinite(w).all()), line
    assert bool((w[~keep] == 0.0).all()) and float(w.min()) >= 0.0, line
    live = keep.any(dim=-1)
    sums = w.double().sum(dim=-1)
    excess = float((sums[live] - 1.0).abs().max()) if bool(live.any()) else 0.0
    assert excess <= AC.rowsum_bound(Nc), (line, excess)
    assert not bool(sums[~live].any()), line
    return excess


# ---- 1. all ones: the unmasked entry's bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.SHAPES, ids=str)
def test_all_ones_is_bit_equal_to_the_unmasked_entry(gpulib, shape):
    from mlhot.ops import favor_query
    route, Nc, lens, d, m = shape
    qd, state, vd, pd = _setup(shape)
    label = "favor.lquerym" if route == "long" else "favor.querym"
    for Nq in CC.NQS:
        rows = qd[:, :Nq].contiguous()
        want_out, want_w = favor_query(rows, state, vd, pd, weights=True)
        for G in (1, 2, Nc):
            ones = torch.ones(T, G, Nq, Nc, dtype=torch.bool, device=DEV)
            labels, (out, w) = U.launch_labels(gpulib, lambda: favor_query(rows, state, vd, pd, weights=True, mask=ones))
            assert labels == [label + "w"]                               # ONE launch for any Nq and G
            assert out.shape == (T, G, Nq, d * H) and w.shape == (T, G, H, Nq, Nc) and out.is_contiguous() and w.is_contiguous()
            for g in range(G):
                assert torch.equal(out[:, g], want_out) and torch.equal(w[:, g], want_w), (Nq, G, g)
            labels, plain = U.launch_labels(gpulib, lambda: favor_query(rows, state, vd, pd, mask=ones))
            assert labels == [label] and torch.equal(plain, out)
    assert U.launch_labels(gpulib, lambda: favor_query(qd, state, vd, pd))[0] == ["favor.lquery" if route == "long" else "favor.query"]


# ---- 2. every pattern against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.SHAPES, ids=str)
def test_masked_read_outs_against_float64(gpulib, shape):
    from mlhot.ops import favor_query
    from mlhot.ragged import pack_mask
    route, Nc, lens, d, m = shape
    qd, state, vd, pd = _setup(shape)
    for pattern in CC.patterns(Nc):
        mk, out64, w64 = CC.want(shape, pattern)
        out, w = favor_query(qd, state, vd, pd, weights=True, mask=mk.to(DEV))
        assert torch.equal(out, favor_query(qd, state, vd, pd, mask=pack_mask(mk, Nc).to(DEV))), pattern      # without w, from packed words
        eo, ew = U.rel_err(out, CM.merged(out64)), U.rel_err(w, w64)
        line = f"favor_query mask {route} Nc={Nc} lens={lens} d={d} m={m} {pattern} G={mk.shape[1]}: out {eo:.2e}, w {ew:.2e} of their scales"
        excess = _check_w(w, mk, CC.lens_of(shape), Nc, line)
        print(f"{line}, |sum_n w - 1| {excess:.2e} ({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
        assert bool(torch.isfinite(out).all()), line
        assert eo <= U.RTOL and ew <= U.RTOL, line
        dead = ~(mk & (torch.arange(Nc)[None, :] < torch.tensor(CC.lens_of(shape))[:, None])[:, None, None, :]).any(dim=-1)       # [T, G, Nq]
        assert not bool(out[dead.to(DEV)].any()), line                   # a row that keeps no valid slot: exact zeros


def test_leave_one_out_over_a_dominant_shot(gpulib):
    """One shot holds more than 0.999 of the weight; the group that drops it keeps the other three, 1e-4 of it each.  Summing the
    kept columns keeps the bound; "the full sum minus the dropped column" would leave three digits."""
    from mlhot.ops import favor_keys, favor_query
    q, k, v, p, mk, out64, w64, full = CC.dominant()
    Nc, slot = CC.DOMINANT["Nc"], CC.DOMINANT["slot"]
    assert float(full[..., slot].min()) > 0.999
    qd, vd, pd = _dev(q), _dev(v), p.to(DEV)
    out, w = favor_query(qd, favor_keys(_dev(k), pd), vd, pd, weights=True, mask=mk.to(DEV))
    _check_w(w, mk, (Nc,) * T, Nc, "dominant")
    for g in range(Nc):                                               # each group on its own scale
        eo, ew = U.rel_err(out[:, g], CM.merged(out64)[:, g]), U.rel_err(w[:, g], w64[:, g])
        print(f"favor_query mask, dominant shot {slot} of {Nc}, group without slot {g}: out {eo:.2e}, w {ew:.2e} of their scales")
        assert eo <= U.RTOL and ew <= U.RTOL, g


# ---- 3. row and group invariance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.SHAPES, ids=str)
def test_rows_and_groups_do_not_depend_on_the_launch(gpulib, shape):
    from mlhot.ops import favor_query
    route, Nc, lens, d, m = shape
    qd, state, vd, pd = _setup(shape)
    mk = torch.cat([CC.mask("random", Nc, CC.lens_of(shape)), CC.mask("causal", Nc, CC.lens_of(shape))], dim=1).to(DEV)      # G = 3
    full_out, full_w = favor_query(qd, state, vd, pd, weights=True, mask=mk)

    def same(rows, mask, gsel, nsel):
        out, w = favor_query(rows.contiguous(), state, vd, pd, weights=True, mask=mask.contiguous())
        return torch.equal(out, full_out[:, gsel][:, :, nsel]) and torch.equal(w, full_w[:, gsel][:, :, :, nsel])
    every = slice(None)
    perm = torch.randperm(NQ, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert same(qd[:, perm], mk[:, :, perm], every, perm)                                      # rows permuted
    for start, L in ((0, 1), (0, 16), (5, 12), (16, 1)):                                       # chunked
        assert same(qd[:, start:start + L], mk[:, :, start:start + L], every, slice(start, start + L)), (start, L)
    big = 3.0 * torch.randn(T, 40, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)   # padded with other rows and other masks
    bigm = torch.rand(T, 3, 40, Nc, device=DEV) < 0.5
    big[:, 11:11 + NQ], bigm[:, :, 11:11 + NQ] = qd, mk
    out, w = favor_query(big, state, vd, pd, weights=True, mask=bigm)
    assert torch.equal(out[:, :, 11:11 + NQ], full_out) and torch.equal(w[:, :, :, 11:11 + NQ], full_w)
    for gs in ([2, 0, 1], [1], [0, 2], [2, 2, 1, 0, 0]):                                        # groups permuted, G changed
        assert same(qd, mk[:, gs], gs, every), gs


# ---- 4. the empty row, the envelope, the NULL mask ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [CC.SHAPES[1], CC.SHAPES[5]], ids=str)
def test_a_row_without_a_kept_slot_is_exact_zeros(gpulib, shape):
    from mlhot.ops import favor_query
    route, Nc, lens, d, m = shape
    qd, state, vd, pd = _setup(shape)
    mk = CC.mask("random", Nc, CC.lens_of(shape)).to(DEV)
    mk[0, 0, 3], mk[1, 1, 16], mk[1, 0, :] = False, False, False
    out, w = favor_query(qd, state, vd, pd, weights=True, mask=mk)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all())
    for t, g, n in ((0, 0, 3), (1, 1, 16), (1, 0, 5)):
        assert not bool(out[t, g, n].any()) and not bool(w[t, g, :, n].any())
    ones = torch.ones_like(mk)
    ref_out, ref_w = favor_query(qd, state, vd, pd, weights=True, mask=torch.where(mk.any(dim=-1, keepdim=True), mk, ones))
    live = mk.any(dim=-1)                                              # the rows beside an empty one are untouched by it
    assert torch.equal(out[live], ref_out[live])


def _raw(gpulib, long, args):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    q, state, v, proj, lens, mask, G, Tn, Hn, Nq, Nc, d, m, out, w, ws = args
    if long:
        return gpulib.c.mlhot_favor_query_long_masked_fwd(p(q), p(state), p(v), p(proj), p(lens), p(mask), G, Tn, Hn, Nq, Nc, d, m, p(out), p(w), p(ws), 256, None)
    return gpulib.c.mlhot_favor_query_masked_fwd(p(q), p(state), p(v), p(proj), p(mask), G, Tn, Hn, Nq, Nc, d, m, p(out), p(w), p(ws), 256, None)


@pytest.mark.parametrize("long,Nc,d,m", [(False, 33, 16, 16), (False, 4, 24, 32), (False, 4, 16, 8), (True, 257, 16, 16), (True, 40, 24, 32)])
def test_outside_the_envelope_nothing_is_written(gpulib, long, Nc, d, m):
    Nq, G = 5, 2
    g = torch.Generator().manual_seed(3)
    q, v = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (Nq, Nc))
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((4096,), 7.0, device=DEV)
    out = torch.full((T, G, Nq, d * H), float("nan"), device=DEV)
    w = torch.full((T, G, H, Nq, Nc), float("nan"), device=DEV)
    mask = torch.full((T, G, Nq, (Nc + 31) // 32), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    assert _raw(gpulib, long, (q, state, v, proj, None, mask, G, T, H, Nq, Nc, d, m, out, w, ws)) == 4           # MLHOT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(w).all()) and bool((state == 7.0).all())
    assert ("favor_query_long_masked_fwd serves Nc <= 256" if long else "favor_query_masked_fwd serves Nc <= 32") in gpulib.c.mlhot_last_error().decode()


@pytest.mark.parametrize("shape", [CC.SHAPES[0], CC.SHAPES[4]], ids=str)
def test_a_null_mask_and_no_group_are_argument_errors(gpulib, shape):
    route, Nc, lens, d, m = shape
    qd, state, vd, pd = _setup(shape)
    Nq = 5
    rows = qd[:, :Nq].contiguous()
    out = torch.full((T, 1, Nq, d * H), float("nan"), device=DEV)
    mask = torch.full((T, 1, Nq, (Nc + 31) // 32), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    for mk, G in ((None, 1), (mask, 0)):
        assert _raw(gpulib, route == "long", (rows, state.buf, vd, pd, state.lens_dev, mk, G, T, H, Nq, Nc, d, m, out, None, ws)) == 1      # MLHOT_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
