"""The paged per-shot key state on the MI355X: mlhot_favor_keys_paged_fwd / mlhot_favor_query_paged_fwd /
mlhot_favor_query_paged_masked_fwd either side of every 256-slot page edge - out, w and F_k against float64, out with w bit-equal to
out without, the bit-for-bit tie to the long entries at one page, capacity and row invariance, ragged states with poisoned rows,
masks that drop a whole page or keep only the last partial one, the dominant-shot leave-one-out, the envelope.  Inputs and float64
references: tests/favor_paged_cases.py.  Run with -m gpu.

The bars are the project's U.RTOL for values and Nc 2^-23 for the row sum of w (tests/attention_readout_cases.rowsum_bound), as for
the long entries: the paged walk runs the same chains, only longer."""
import ctypes as C

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import context_mask_ref as CM
from tests import favor_cached_ref as R
from tests import favor_paged_cases as PC
from tests import ragged_ref as RR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = PC.T, PC.H


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _rowsum_excess(w):
    return float((w.double().sum(dim=-1) - 1.0).abs().max())


def _setup(kind, d, m, Nc):
    from mlhot.ops import favor_keys_paged
    q, k, v, proj = PC.inputs(kind, d, m, Nc)
    qd, vd, pd = _dev(q), _dev(v), proj.to(DEV)
    state = favor_keys_paged(_dev(k), pd)
    assert state.route == "paged" and state.lens is None and state.dims == (T, Nc, H, d, m)
    return qd, state, vd, pd


# ---- 1. values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,m,Nc", PC.cases())
def test_out_and_weights_against_float64(gpulib, kind, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup(kind, d, m, Nc)
    k = PC.inputs(kind, d, m, Nc)[1]
    w64, out64 = PC.want(kind, d, m, Nc)
    fk, M = state.features()
    fk64, M64 = R.key_features(k, pd.cpu())
    ferr = U.rel_err(fk[..., :m], fk64)
    print(f"favor_keys_paged {kind} d={d} m={m} Nc={Nc}: F_k {ferr:.2e} of its scale, M {float(M):.6f} against {float(M64):.6f}")
    assert ferr <= U.RTOL and abs(float(M) - float(M64)) <= U.RTOL * max(1.0, abs(float(M64)))
    assert not bool(fk[..., m:].any())                               # features >= m are zeros
    for Nq in [n for n in PC.NQS if (d, m) != PC.DM_BIG or n <= PC.NQ_BIG]:
        rows = qd[:, :Nq].contiguous()
        out, w = favor_query(rows, state, vd, pd, weights=True)
        assert w.shape == (T, H, Nq, Nc) and w.is_contiguous() and out.shape == (T, Nq, d * H)
        assert torch.equal(out, favor_query(rows, state, vd, pd)), Nq             # out with w is out without
        eo, ew, excess = U.rel_err(out, R.merged(out64[:, :, :Nq])), U.rel_err(w, w64[:, :, :Nq]), _rowsum_excess(w)
        line = (f"favor_query paged {kind} d={d} m={m} Nc={Nc} Nq={Nq}: out {eo:.2e}, w {ew:.2e} of their scales, |sum_n w - 1| {excess:.2e} "
                f"({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
        print(line)
        assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0, line
        assert eo <= U.RTOL and ew <= U.RTOL, line
        assert excess <= AC.rowsum_bound(Nc), line


def test_the_launches(gpulib):
    from mlhot.ops import favor_keys_paged, favor_query
    q, k, v, proj = PC.inputs("live", 16, 16, 513)
    qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
    labels, state = U.launch_labels(gpulib, lambda: favor_keys_paged(kd, pd))
    assert labels == ["favor.pkeys1", "favor.pkeys2"]
    ones = torch.ones(T, 3, PC.NQ, 513, dtype=torch.bool, device=DEV)
    for kw, label in (({}, "favor.pquery"), ({"weights": True}, "favor.pqueryw"), ({"mask": ones}, "favor.pquerym"),
                      ({"mask": ones, "weights": True}, "favor.pquerymw")):
        assert U.launch_labels(gpulib, lambda: favor_query(qd, state, vd, pd, **kw))[0] == [label]            # one launch for any Nq and G


# ---- 2. the tie to the long entries at one page -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", PC.TIE_NCS)
@pytest.mark.parametrize("d,m", PC.DM)
def test_one_page_has_the_long_entries_bits(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys_long, favor_keys_paged, favor_query
    lens = (Nc, max(1, Nc - 7))
    mk = torch.rand(T, 3, PC.NQ, Nc, generator=torch.Generator().manual_seed(Nc)) < 0.5
    mk[:, 0] = True
    mk = mk.to(DEV)
    for kind in PC.KINDS:
        q, k, v, proj = PC.inputs(kind, d, m, Nc)
        qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
        for ln in (None, list(lens)):
            long, paged = favor_keys_long(kd, pd, lens=ln), favor_keys_paged(kd, pd, lens=ln)
            assert long.route == "long" and paged.route == "paged"
            for a, b in zip(paged.features(), long.features()):
                assert torch.equal(a, b), (kind, ln)
            out, w = favor_query(qd, paged, vd, pd, weights=True)
            want_out, want_w = favor_query(qd, long, vd, pd, weights=True)
            assert torch.equal(out, want_out) and torch.equal(w, want_w), (kind, ln)
            assert torch.equal(favor_query(qd, paged, vd, pd), want_out), (kind, ln)
            out, w = favor_query(qd, paged, vd, pd, weights=True, mask=mk)          # mlhot_favor_query_long_masked_fwd's bits
            want_out, want_w = favor_query(qd, long, vd, pd, weights=True, mask=mk)
            assert torch.equal(out, want_out) and torch.equal(w, want_w), (kind, ln)
            assert torch.equal(favor_query(qd, paged, vd, pd, mask=mk), want_out), (kind, ln)


# ---- 3. capacity invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(300, 300), (300, 257)])
@pytest.mark.parametrize("d,m", PC.DM)
def test_the_same_shots_at_another_capacity_give_the_same_bits(gpulib, d, m, lens):
    from mlhot.ops import favor_keys_paged, favor_query
    q, k, v, proj = PC.inputs("live", d, m, 300)
    qd, pd = _dev(q), proj.to(DEV)
    got = {}
    for cap in (300, 320, 1024):
        kc = torch.full((T, H, cap, d), float("nan"))
        vc = torch.full((T, H, cap, d), -1e30)
        for t, L in enumerate(lens):
            kc[t, :, :L], vc[t, :, :L] = k[t, :, :L], v[t, :, :L]
        state = favor_keys_paged(_dev(kc), pd, lens=list(lens))
        out, w = favor_query(qd, state, _dev(vc), pd, weights=True)
        assert bool((w[..., 300:] == 0.0).all()) and bool(torch.isfinite(out).all())
        mk = torch.zeros(T, 2, PC.NQ, cap, dtype=torch.bool, device=DEV)
        mk[..., :300] = (torch.rand(T, 2, PC.NQ, 300, generator=torch.Generator().manual_seed(8)) < 0.5).to(DEV)
        mk[..., 0], mk[..., 300:] = True, True                        # the bits behind the shots do not count
        mout, mw = favor_query(qd, state, _dev(vc), pd, weights=True, mask=mk)
        got[cap] = (out, w[..., :300].contiguous(), state.features()[0][:, :, :300].contiguous(), state.features()[1].clone(), mout,
                    mw[..., :300].contiguous())
    for cap in (320, 1024):
        for a, b in zip(got[cap], got[300]):
            assert torch.equal(a, b), cap
    if lens == (300, 300):                                             # ... and full tasks need no lens at all
        state = favor_keys_paged(_dev(k), pd)
        out, w = favor_query(qd, state, _dev(v), pd, weights=True)
        assert torch.equal(out, got[300][0]) and torch.equal(w, got[300][1]) and torch.equal(state.features()[0], got[300][2])


# ---- 4. row invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", [257, 513])
@pytest.mark.parametrize("d,m", PC.DM)
def test_rows_do_not_depend_on_the_launch(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup("live", d, m, Nc)
    mk = PC.mask("random", Nc, (Nc, Nc)).to(DEV)
    full_out, full_w = favor_query(qd, state, vd, pd, weights=True)
    full_mout, full_mw = favor_query(qd, state, vd, pd, weights=True, mask=mk)
    assert full_w.shape == (T, H, PC.NQ, Nc) and bool(torch.isfinite(full_w).all())

    def same(rows, sel):
        out, w = favor_query(rows.contiguous(), state, vd, pd, weights=True)
        mout, mw = favor_query(rows.contiguous(), state, vd, pd, weights=True, mask=mk[:, :, sel].contiguous())
        return (torch.equal(out, full_out[:, sel]) and torch.equal(w, full_w[:, :, sel]) and torch.equal(mout, full_mout[:, :, sel])
                and torch.equal(mw, full_mw[:, :, :, sel]))
    for n in (0, 15, 16, 36):                                          # a row alone
        assert same(qd[:, n:n + 1], slice(n, n + 1)), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17)):
        assert same(qd[:, start:start + L], slice(start, start + L)), (start, L)
    perm = torch.randperm(PC.NQ, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert same(qd[:, perm], perm)
    big = 3.0 * torch.randn(T, 100, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)           # other rows, another regime
    big[:, 37:37 + PC.NQ] = qd
    bigm = torch.rand(T, 3, 100, Nc, device=DEV) < 0.5
    bigm[:, :, 37:37 + PC.NQ] = mk
    out, w = favor_query(big, state, vd, pd, weights=True)
    assert torch.equal(out[:, 37:37 + PC.NQ], full_out) and torch.equal(w[:, :, 37:37 + PC.NQ], full_w)
    mout, mw = favor_query(big, state, vd, pd, weights=True, mask=bigm)
    assert torch.equal(mout[:, :, 37:37 + PC.NQ], full_mout) and torch.equal(mw[:, :, :, 37:37 + PC.NQ], full_mw)
    for gs in ([2, 0, 1], [1], [2, 2, 0]):                             # groups permuted, G changed
        mout, mw = favor_query(qd, state, vd, pd, weights=True, mask=mk[:, gs].contiguous())
        assert torch.equal(mout, full_mout[:, gs]) and torch.equal(mw, full_mw[:, gs]), gs


# ---- 5. ragged states ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", PC.RAGGED_NCS)
@pytest.mark.parametrize("d,m", PC.DM)
def test_ragged_tasks_with_poisoned_rows(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys_paged, favor_query
    for lens in PC.ragged_lens(Nc):
        q, kn, vp, proj, w64, out64, fk64, M64 = PC.ragged("live", d, m, Nc, lens)
        qd, vd, pd = _dev(q), _dev(vp), proj.to(DEV)
        state = favor_keys_paged(_dev(kn), pd, lens=list(lens))
        assert state.lens == tuple(lens) and state.lens_dev.dtype == torch.int32
        fk, M = state.features()
        out, w = favor_query(qd, state, vd, pd, weights=True)
        assert torch.equal(out, favor_query(qd, state, vd, pd))
        assert bool(torch.isfinite(fk).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all())
        for t, L in enumerate(lens):
            assert not bool(fk[t, :, L:].any()) and bool((w[t, :, :, L:] == 0.0).all()), (lens, t)          # exact zeros
            assert float(w[t, :, :, :L].min()) > 0.0, (lens, t)
        ferr, eo, ew, excess = U.rel_err(fk[..., :m], fk64), U.rel_err(out, R.merged(out64)), U.rel_err(w, w64), _rowsum_excess(w)
        print(f"favor paged, ragged lens={lens} d={d} m={m} Nc={Nc}: F_k {ferr:.2e}, out {eo:.2e}, w {ew:.2e} of their scales, "
              f"|sum_n w - 1| {excess:.2e} ({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
        assert ferr <= U.RTOL and eo <= U.RTOL and ew <= U.RTOL and excess <= AC.rowsum_bound(Nc)
        assert abs(float(M) - float(M64)) <= U.RTOL * max(1.0, abs(float(M64)))
        for t, L in enumerate(lens):                                   # ... and on the valid part of every task on its own
            assert U.rel_err(w[t, :, :, :L], w64[t, :, :, :L]) <= U.RTOL and U.rel_err(out[t], R.merged(out64)[t]) <= U.RTOL
        ones = torch.ones(T, 2, PC.NQ, Nc, dtype=torch.bool, device=DEV)                                   # the masked entry on the same poison
        mout, mw = favor_query(qd, state, vd, pd, weights=True, mask=ones)
        for g in range(2):
            assert torch.equal(mout[:, g], out) and torch.equal(mw[:, g], w), (lens, g)


def test_the_state_is_written_whatever_the_buffer_held(gpulib):
    d, m, Nc, lens = 64, 266, 300, (1, 257)
    k, proj = PC.inputs("live", d, m, Nc)[1], PC.inputs("live", d, m, Nc)[3]
    kd, pd = _dev(k), proj.to(DEV)
    for ld in (None, torch.tensor(lens, dtype=torch.int32, device=DEV)):
        fresh = gpulib.favor_keys_paged_fwd(kd, pd, ld)
        nb = gpulib.favor_keys_paged_bytes(T, H, Nc, d, m)
        buf = torch.full((nb // 4,), float("nan"), device=DEV).view(torch.uint8)
        assert gpulib.favor_keys_paged_fwd(kd, pd, ld, out=buf) is buf
        fk, M = gpulib.favor_state_views(buf, T, H, Nc, m)
        assert bool(torch.isfinite(fk).all()) and bool(torch.isfinite(M).all())
        want_fk, want_M = gpulib.favor_state_views(fresh, T, H, Nc, m)
        assert torch.equal(fk, want_fk) and torch.equal(M, want_M)


# ---- 6. masks ------------------------------------------------------------------------------------------------------------------------
def _mask_setup(Nc, d, m):
    from mlhot.ops import favor_keys_paged
    q, k, v, p = PC.mask_inputs(Nc, d, m)
    pd = p.to(DEV)
    return _dev(q), favor_keys_paged(_dev(k), pd, lens=list(PC.mask_lens(Nc))), _dev(v), pd


def _check_w(w, mk, lens, Nc, line):
    """masked columns exactly 0, kept entries >= 0, rows that keep a valid slot sum to 1, the others are zeros, nothing is NaN"""
    keep = (mk & RR.valid_mask(lens, Nc)[:, None, None, :]).to(w.device)[:, :, None].expand_as(w)
    assert bool(torch.isfinite(w).all()), line
    assert bool((w[~keep] == 0.0).all()) and float(w.min()) >= 0.0, line
    live = keep.any(dim=-1)
    sums = w.double().sum(dim=-1)
    excess = float((sums[live] - 1.0).abs().max()) if bool(live.any()) else 0.0
    assert excess <= AC.rowsum_bound(Nc), (line, excess)
    assert not bool(sums[~live].any()), line
    return excess


@pytest.mark.parametrize("Nc", PC.MASK_NCS)
@pytest.mark.parametrize("d,m", PC.DM)
def test_all_ones_is_bit_equal_to_the_unmasked_entry(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _mask_setup(Nc, d, m)
    for Nq in PC.NQS:
        rows = qd[:, :Nq].contiguous()
        want_out, want_w = favor_query(rows, state, vd, pd, weights=True)
        for G in (1, 3):
            ones = torch.ones(T, G, Nq, Nc, dtype=torch.bool, device=DEV)
            out, w = favor_query(rows, state, vd, pd, weights=True, mask=ones)
            assert out.shape == (T, G, Nq, d * H) and w.shape == (T, G, H, Nq, Nc) and out.is_contiguous() and w.is_contiguous()
            for g in range(G):
                assert torch.equal(out[:, g], want_out) and torch.equal(w[:, g], want_w), (Nq, G, g)
            assert torch.equal(favor_query(rows, state, vd, pd, mask=ones), out)                      # out without w
            if G == 1:
                o3, w3 = favor_query(rows, state, vd, pd, weights=True, mask=ones[:, 0])              # a 3-D mask
                assert torch.equal(o3[:, 0], want_out) and torch.equal(w3[:, 0], want_w)


@pytest.mark.parametrize("Nc", PC.MASK_NCS)
@pytest.mark.parametrize("d,m", PC.DM)
def test_masked_read_outs_against_float64(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    from mlhot.ragged import pack_mask
    qd, state, vd, pd = _mask_setup(Nc, d, m)
    lens = PC.mask_lens(Nc)
    for pattern in PC.MASK_PATTERNS:
        mk, out64, w64 = PC.mask_want(Nc, d, m, pattern)
        out, w = favor_query(qd, state, vd, pd, weights=True, mask=mk.to(DEV))
        assert torch.equal(out, favor_query(qd, state, vd, pd, mask=pack_mask(mk, Nc).to(DEV))), pattern      # without w, from packed words
        for g in range(mk.shape[1]):                                   # a 4-D mask is its G 3-D calls, bit for bit
            og, wg = favor_query(qd, state, vd, pd, weights=True, mask=mk[:, g].to(DEV))
            assert torch.equal(og[:, 0], out[:, g]) and torch.equal(wg[:, 0], w[:, g]), (pattern, g)
        line = f"favor_query mask paged Nc={Nc} lens={lens} d={d} m={m} {pattern}"
        excess = _check_w(w, mk, lens, Nc, line)
        assert bool(torch.isfinite(out).all()), line
        for g in range(mk.shape[1]):                                   # each group on its own scale
            eo, ew = U.rel_err(out[:, g], CM.merged(out64)[:, g]), U.rel_err(w[:, g], w64[:, g])
            print(f"{line} group {g}: out {eo:.2e}, w {ew:.2e} of their scales, |sum_n w - 1| {excess:.2e}")
            assert eo <= U.RTOL and ew <= U.RTOL, (line, g)
        dead = ~(mk & RR.valid_mask(lens, Nc)[:, None, None, :]).any(dim=-1)                           # [T, G, Nq]
        assert not bool(out[dead.to(DEV)].any()), line                 # a row that keeps no valid slot: exact zeros


@pytest.mark.parametrize("Nc", PC.MASK_NCS)
def test_a_row_without_a_kept_slot_is_exact_zeros(gpulib, Nc):
    from mlhot.ops import favor_query
    d, m = 64, 266
    qd, state, vd, pd = _mask_setup(Nc, d, m)
    mk = PC.mask("random", Nc, PC.mask_lens(Nc)).to(DEV)
    mk[0, 0, 3], mk[1, 1, 16], mk[1, 0, :] = False, False, False
    mk[1, 2, 20, :270] = False                                         # keeps only slots behind the task's shots: nothing valid
    out, w = favor_query(qd, state, vd, pd, weights=True, mask=mk)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all())
    for t, g, n in ((0, 0, 3), (1, 1, 16), (1, 0, 5), (1, 2, 20)):
        assert not bool(out[t, g, n].any()) and not bool(w[t, g, :, n].any())
    assert torch.equal(out, favor_query(qd, state, vd, pd, mask=mk))
    filled = torch.where(mk.any(dim=-1, keepdim=True), mk, torch.ones_like(mk))
    filled[1, 2, 20] = True
    ref_out, _ = favor_query(qd, state, vd, pd, weights=True, mask=filled)
    live = mk.any(dim=-1)
    live[1, 2, 20] = False
    assert torch.equal(out[live], ref_out[live])                       # the rows beside an empty one are untouched by it


def test_leave_one_out_over_a_dominant_shot(gpulib):
    """One shot on the second page holds nearly all the weight; the group that drops it keeps the other 299, each at the feature
    floor.  Summing the kept columns keeps the bar; "the full sum minus the dropped column" would lose the digits to cancellation."""
    from mlhot.ops import favor_keys_paged, favor_query
    q, k, v, p, mk, out64, w64, full = PC.dominant()
    Nc, slot, drop = PC.DOMINANT["Nc"], PC.DOMINANT["slot"], PC.DOMINANT["drop"]
    assert float(full[..., slot].min()) > 0.9
    qd, vd, pd = _dev(q), _dev(v), p.to(DEV)
    out, w = favor_query(qd, favor_keys_paged(_dev(k), pd), vd, pd, weights=True, mask=mk.to(DEV))
    _check_w(w, mk, (Nc,) * T, Nc, "dominant")
    for g, s in enumerate(drop):                                       # each group on its own scale
        eo, ew = U.rel_err(out[:, g], CM.merged(out64)[:, g]), U.rel_err(w[:, g], w64[:, g])
        print(f"favor_query mask paged, dominant shot {slot} of {Nc}, group without slot {s}: out {eo:.2e}, w {ew:.2e} of their scales")
        assert eo <= U.RTOL and ew <= U.RTOL, g


# ---- 7. the envelope -----------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("Nc,d,m", [(4097, 16, 16), (300, 24, 32), (300, 16, 8)])
def test_outside_the_envelope_nothing_is_written(gpulib, Nc, d, m):
    Nq, G = 5, 2
    g = torch.Generator().manual_seed(3)
    q, k = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (Nq, Nc))
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((1 << 16,), 7.0, device=DEV)
    out = torch.full((T, G, Nq, d * H), float("nan"), device=DEV)
    w = torch.full((T, G, H, Nq, Nc), float("nan"), device=DEV)
    mask = torch.full((T, G, Nq, (Nc + 31) // 32), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    c = gpulib.c
    assert not gpulib.favor_paged_supported(T, H, Nc, d, m) and gpulib.favor_keys_paged_bytes(T, H, Nc, d, m) == 0
    assert c.mlhot_favor_query_paged_bytes(T, H, Nq, Nc, d, m, 0) == 0 and c.mlhot_favor_query_paged_bytes(T, H, Nq, Nc, d, m, G) == 0
    calls = {
        "favor_keys_paged_fwd": lambda: c.mlhot_favor_keys_paged_fwd(_p(k), _p(proj), None, T, H, Nc, d, m, _p(state), state.numel() * 4, None),
        "favor_query_paged_fwd": lambda: c.mlhot_favor_query_paged_fwd(_p(q), _p(state), _p(k), _p(proj), None, T, H, Nq, Nc, d, m, _p(out), _p(w), _p(ws),
                                                                       ws.numel(), None),
        "favor_query_paged_masked_fwd": lambda: c.mlhot_favor_query_paged_masked_fwd(_p(q), _p(state), _p(k), _p(proj), None, _p(mask), G, T, H, Nq, Nc, d, m,
                                                                                     _p(out), _p(w), _p(ws), ws.numel(), None),
    }
    for name, call in calls.items():
        assert call() == 4, name                                       # MLHOT_ERR_UNSUPPORTED
        msg = c.mlhot_last_error().decode()
        assert f"{name} serves Nc <= 4096" in msg and f"Nc={Nc} d={d} m={m}" in msg, msg
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(w).all()) and bool((state == 7.0).all()) and not bool(ws.any())


def test_the_envelope_ends_at_4096_slots_and_the_other_forms_keep_theirs(gpulib):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_keys_paged
    assert gpulib.favor_paged_supported(T, H, 4096, 256, 1536) and gpulib.favor_paged_supported(T, H, 1, 16, 16)
    assert not gpulib.favor_paged_supported(T, H, 4097, 256, 1536)
    assert gpulib.favor_long_supported(T, H, 256, 16, 16) and not gpulib.favor_long_supported(T, H, 257, 16, 16)
    ntile = 3
    assert gpulib.c.mlhot_favor_query_paged_bytes(T, H, 37, 513, 16, 16, 0) == 256
    assert gpulib.c.mlhot_favor_query_paged_bytes(T, H, 37, 513, 16, 16, 5) >= T * H * ntile * 5 * 16 * 4
    proj = torch.randn(16, 16).to(DEV)
    with pytest.raises(MlhotError, match="favor_keys_paged serves Nc <= 4096.*Nc=4097"):
        favor_keys_paged(torch.zeros(T, 4097, H, 16, device=DEV), proj)
    with pytest.raises(MlhotError, match=r"lens must lie in 1\.\.300"):
        favor_keys_paged(torch.zeros(T, 300, H, 16, device=DEV), proj, lens=[0, 300])


def test_a_null_mask_no_group_and_a_short_workspace_are_refused(gpulib):
    Nc, d, m, Nq, G = 513, 16, 16, 5, 3
    qd, state, vd, pd = _setup("live", d, m, Nc)
    rows = qd[:, :Nq].contiguous()
    out = torch.full((T, G, Nq, d * H), float("nan"), device=DEV)
    mask = torch.full((T, G, Nq, (Nc + 31) // 32), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    call = lambda mk, g, nws: gpulib.c.mlhot_favor_query_paged_masked_fwd(_p(rows), _p(state.buf), _p(vd), _p(pd), None, _p(mk), g, T, H, Nq, Nc, d, m,
                                                                          _p(out), None, _p(ws), nws, None)
    assert call(None, 1, ws.numel()) == 1 and call(mask, 0, ws.numel()) == 1                        # MLHOT_ERR_ARG
    assert call(mask, G, 256) == 2 and "workspace too small" in gpulib.c.mlhot_last_error().decode()  # MLHOT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(mask, G, ws.numel()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0], gpulib.favor_query_paged_fwd(rows, state.buf, vd, pd))


def test_nothing_is_written_outside_w_and_out(gpulib):
    """Nq 17: a full row tile and a tile of one row; Nc 513: three pages, a row length that is no multiple of 4; w starts 3 floats
    into its buffer.  Unmasked and masked (G 2) entries."""
    d, m, Nc, Nq, lead, guard, G = 64, 266, 513, 17, 3, 4096, 2
    qd, state, vd, pd = _setup("live", d, m, Nc)
    rows = qd[:, :Nq].contiguous()
    want_out, want_w = gpulib.favor_query_paged_fwd(rows, state.buf, vd, pd, weights=True)
    mask = torch.full((T, G, Nq, (Nc + 31) // 32), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for groups in (0, G):
        n, no = T * max(groups, 1) * H * Nq * Nc, T * max(groups, 1) * Nq * d * H
        buf = torch.full((lead + guard + n + guard,), float("nan"), device=DEV)
        obuf = torch.full((guard + no + guard,), float("nan"), device=DEV)
        w, out = buf[lead + guard:lead + guard + n], obuf[guard:guard + no]
        if groups:
            rc = gpulib.c.mlhot_favor_query_paged_masked_fwd(_p(rows), _p(state.buf), _p(vd), _p(pd), None, _p(mask), G, T, H, Nq, Nc, d, m, _p(out), _p(w),
                                                             _p(ws), ws.numel(), None)
        else:
            rc = gpulib.c.mlhot_favor_query_paged_fwd(_p(rows), _p(state.buf), _p(vd), _p(pd), None, T, H, Nq, Nc, d, m, _p(out), _p(w), _p(ws), ws.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0
        assert bool(torch.isnan(buf[:lead + guard]).all()) and bool(torch.isnan(buf[lead + guard + n:]).all())
        assert bool(torch.isnan(obuf[:guard]).all()) and bool(torch.isnan(obuf[guard + no:]).all())
        if groups:
            for g in range(G):
                assert torch.equal(w.view(T, G, H, Nq, Nc)[:, g], want_w) and torch.equal(out.view(T, G, Nq, d * H)[:, g], want_out)
        else:
            assert torch.equal(w.view(T, H, Nq, Nc), want_w) and torch.equal(out.view(T, Nq, d * H), want_out)
