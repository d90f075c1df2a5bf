"""The long per-shot key state on the MI355X: mlhot_favor_keys_long_fwd / mlhot_favor_query_long_fwd at every 32-slot
chunk edge up to 256 slots - out, w and F_k against float64, out with w bit-equal to out without, row invariance, the masked state
with poisoned rows, capacity invariance, the bit-for-bit tie to the shipped cached kernels at one chunk, every float of the state
written, the envelope.  Inputs and float64 references: tests/favor_long_cases.py.  Run with -m gpu.

The bars are the project's U.RTOL for values and Nc 2^-23 for the row sum of w (tests/attention_readout_cases.rowsum_bound: one
rounding per quotient plus the Nc - 1 of D's own sum)."""
import ctypes as C

import pytest
import torch

from tests import attention_readout_cases as AC
from tests import favor_cached_ref as R
from tests import favor_long_cases as LC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = LC.T, LC.H


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _rowsum_excess(w):
    return float((w.double().sum(dim=-1) - 1.0).abs().max())


def _setup(kind, d, m, Nc):
    from mlhot.ops import favor_keys_long
    q, k, v, proj = LC.inputs(kind, d, m, Nc)
    qd, vd, pd = _dev(q), _dev(v), proj.to(DEV)
    state = favor_keys_long(_dev(k), pd)
    assert state.route == "long" and state.lens is None and state.dims == (T, Nc, H, d, m)
    return qd, state, vd, pd


# ---- 1. values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,m,Nc", LC.cases())
def test_out_and_weights_against_float64(gpulib, kind, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup(kind, d, m, Nc)
    k = LC.inputs(kind, d, m, Nc)[1]
    w64, out64 = LC.want(kind, d, m, Nc)
    fk, M = state.features()
    fk64, M64 = R.key_features(k, pd.cpu())
    ferr = U.rel_err(fk[..., :m], fk64)
    print(f"favor_keys_long {kind} d={d} m={m} Nc={Nc}: F_k {ferr:.2e} of its scale, M {float(M):.6f} against {float(M64):.6f}")
    assert ferr <= U.RTOL and abs(float(M) - float(M64)) <= U.RTOL * max(1.0, abs(float(M64)))
    assert not bool(fk[..., m:].any())                               # features >= m are zeros
    for Nq in [n for n in LC.NQS if (d, m) != LC.DM_BIG or n <= LC.NQ_BIG]:
        rows = qd[:, :Nq].contiguous()
        out, w = favor_query(rows, state, vd, pd, weights=True)
        assert w.shape == (T, H, Nq, Nc) and w.is_contiguous() and out.shape == (T, Nq, d * H)
        assert torch.equal(out, favor_query(rows, state, vd, pd)), Nq             # out with w is out without
        eo, ew, excess = U.rel_err(out, R.merged(out64[:, :, :Nq])), U.rel_err(w, w64[:, :, :Nq]), _rowsum_excess(w)
        line = (f"favor_query long {kind} d={d} m={m} Nc={Nc} Nq={Nq}: out {eo:.2e}, w {ew:.2e} of their scales, |sum_n w - 1| {excess:.2e} "
                f"({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
        print(line)
        assert bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0, line
        assert eo <= U.RTOL and ew <= U.RTOL, line
        assert excess <= AC.rowsum_bound(Nc), line


def test_the_launches(gpulib):
    from mlhot.ops import favor_keys_long, favor_query
    q, k, v, proj = LC.inputs("live", 16, 16, 65)
    qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
    labels, state = U.launch_labels(gpulib, lambda: favor_keys_long(kd, pd))
    assert labels == ["favor.lkeys1", "favor.lkeys2"]
    assert U.launch_labels(gpulib, lambda: favor_query(qd, state, vd, pd))[0] == ["favor.lquery"]             # one launch for any Nq
    assert U.launch_labels(gpulib, lambda: favor_query(qd, state, vd, pd, weights=True))[0] == ["favor.lqueryw"]


# ---- 2. row invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", LC.NCS)
@pytest.mark.parametrize("d,m", LC.DM)
def test_rows_do_not_depend_on_the_launch(gpulib, d, m, Nc):
    from mlhot.ops import favor_query
    qd, state, vd, pd = _setup("live", d, m, Nc)
    full_out, full_w = favor_query(qd, state, vd, pd, weights=True)
    assert full_w.shape == (T, H, LC.NQ, Nc) and bool(torch.isfinite(full_w).all())

    def same(rows, sel):
        out, w = favor_query(rows.contiguous(), state, vd, pd, weights=True)
        return torch.equal(out, full_out[:, sel]) and torch.equal(w, full_w[:, :, sel])
    for n in (0, 15, 16, 39):                                          # a row alone
        assert same(qd[:, n:n + 1], slice(n, n + 1)), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17), (20, 20)):
        assert same(qd[:, start:start + L], slice(start, start + L)), (start, L)
    perm = torch.randperm(LC.NQ, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert same(qd[:, perm], perm)
    big = 3.0 * torch.randn(T, 100, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)           # other rows, another regime
    big[:, 37:37 + LC.NQ] = qd
    out, w = favor_query(big, state, vd, pd, weights=True)
    assert torch.equal(out[:, 37:37 + LC.NQ], full_out) and torch.equal(w[:, :, 37:37 + LC.NQ], full_w)


# ---- 3. the masked state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", LC.RAGGED_NCS)
@pytest.mark.parametrize("d,m", LC.DM)
def test_ragged_tasks_with_poisoned_rows(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys_long, favor_query
    for lens in LC.ragged_lens(Nc):
        q, kn, vp, proj, w64, out64, fk64, M64 = LC.ragged("live", d, m, Nc, lens)
        qd, vd, pd = _dev(q), _dev(vp), proj.to(DEV)
        state = favor_keys_long(_dev(kn), pd, lens=list(lens))
        assert state.lens == tuple(lens) and state.lens_dev.dtype == torch.int32
        fk, M = state.features()
        out, w = favor_query(qd, state, vd, pd, weights=True)
        assert torch.equal(out, favor_query(qd, state, vd, pd))
        assert bool(torch.isfinite(fk).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all())
        for t, L in enumerate(lens):
            assert not bool(fk[t, :, L:].any()) and bool((w[t, :, :, L:] == 0.0).all()), (lens, t)          # exact zeros
            assert float(w[t, :, :, :L].min()) > 0.0, (lens, t)
        ferr, eo, ew, excess = U.rel_err(fk[..., :m], fk64), U.rel_err(out, R.merged(out64)), U.rel_err(w, w64), _rowsum_excess(w)
        print(f"favor long, masked lens={lens} d={d} m={m} Nc={Nc}: F_k {ferr:.2e}, out {eo:.2e}, w {ew:.2e} of their scales, "
              f"|sum_n w - 1| {excess:.2e} ({excess / AC.rowsum_bound(Nc):.2f} of the bound)")
        assert ferr <= U.RTOL and eo <= U.RTOL and ew <= U.RTOL and excess <= AC.rowsum_bound(Nc)
        assert abs(float(M) - float(M64)) <= U.RTOL * max(1.0, abs(float(M64)))
        for t, L in enumerate(lens):                                   # ... and on the valid part of every task on its own
            assert U.rel_err(w[t, :, :, :L], w64[t, :, :, :L]) <= U.RTOL and U.rel_err(out[t], R.merged(out64)[t]) <= U.RTOL


# ---- 4. capacity invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(40, 40), (40, 7)])
@pytest.mark.parametrize("d,m", LC.DM)
def test_the_same_shots_at_another_capacity_give_the_same_bits(gpulib, d, m, lens):
    from mlhot.ops import favor_keys_long, favor_query
    q, k, v, proj = LC.inputs("live", d, m, 40)
    qd, pd = _dev(q), proj.to(DEV)
    got = {}
    for cap in (40, 64, 256):
        kc = torch.full((T, H, cap, d), float("nan"))
        vc = torch.full((T, H, cap, d), -1e30)
        for t, L in enumerate(lens):
            kc[t, :, :L], vc[t, :, :L] = k[t, :, :L], v[t, :, :L]
        state = favor_keys_long(_dev(kc), pd, lens=list(lens))
        out, w = favor_query(qd, state, _dev(vc), pd, weights=True)
        assert bool((w[..., 40:] == 0.0).all()) and bool(torch.isfinite(out).all())
        got[cap] = (out, w[..., :40].contiguous(), state.features()[0][:, :, :40].contiguous(), state.features()[1].clone())
    for cap in (64, 256):
        for a, b in zip(got[cap], got[40]):
            assert torch.equal(a, b), cap
    if lens == (40, 40):                                               # ... and full tasks need no lens at all
        state = favor_keys_long(_dev(k), pd)
        out, w = favor_query(qd, state, _dev(v), pd, weights=True)
        assert torch.equal(out, got[40][0]) and torch.equal(w, got[40][1]) and torch.equal(state.features()[0], got[40][2])


# ---- 5. the tie to the shipped kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", LC.TIE_NCS)
@pytest.mark.parametrize("d,m", LC.DM + [LC.DM_BIG])
def test_one_chunk_has_the_cached_kernels_bits(gpulib, d, m, Nc):
    from mlhot.ops import favor_keys, favor_keys_long, favor_query
    for kind in LC.KINDS:
        q, k, v, proj = LC.inputs(kind, d, m, Nc)
        qd, kd, vd, pd = _dev(q)[:, :LC.NQ_BIG].contiguous(), _dev(k), _dev(v), proj.to(DEV)
        cached, long = favor_keys(kd, pd), favor_keys_long(kd, pd)
        assert cached.route == "cached" and long.route == "long"
        for a, b in zip(long.features(), cached.features()):
            assert torch.equal(a, b), kind
        out, w = favor_query(qd, long, vd, pd, weights=True)
        want_out, want_w = favor_query(qd, cached, vd, pd, weights=True)
        assert torch.equal(out, want_out) and torch.equal(w, want_w), kind
        assert torch.equal(favor_query(qd, long, vd, pd), want_out), kind


@pytest.mark.parametrize("d,m", LC.DM)
def test_the_first_chunk_of_a_longer_state_is_the_cached_state_of_its_shots(gpulib, d, m):
    from mlhot.ops import favor_keys, favor_keys_long
    q, k, v, proj = LC.peak_first(d, m)
    kd, pd = _dev(k), proj.to(DEV)
    long, cached = favor_keys_long(kd, pd), favor_keys(kd[:, :32].contiguous(), pd)
    assert cached.route == "cached"
    assert torch.equal(long.features()[1], cached.features()[1])       # the stabiliser sits in the first 32 shots
    assert torch.equal(long.features()[0][:, :, :32], cached.features()[0])


# ---- 6. every float of the state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [None, (1, 33)])
@pytest.mark.parametrize("Nc", [33, 65])
def test_the_state_is_written_whatever_the_buffer_held(gpulib, Nc, lens):
    d, m = 64, 266
    q, k, v, proj = LC.inputs("live", d, m, Nc)
    kd, pd = _dev(k), proj.to(DEV)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    fresh = gpulib.favor_keys_long_fwd(kd, pd, ld)
    nb = gpulib.favor_keys_long_bytes(T, H, Nc, d, m)
    buf = torch.full((nb // 4,), float("nan"), device=DEV).view(torch.uint8)
    assert gpulib.favor_keys_long_fwd(kd, pd, ld, out=buf) is buf
    fk, M = gpulib.favor_state_views(buf, T, H, Nc, m)
    assert bool(torch.isfinite(fk).all()) and bool(torch.isfinite(M).all())
    want_fk, want_M = gpulib.favor_state_views(fresh, T, H, Nc, m)
    assert torch.equal(fk, want_fk) and torch.equal(M, want_M)


def test_nothing_is_written_outside_w_and_out(gpulib):
    """Nq 17: a full row tile and a tile of one row; Nc 65: three chunks, a row length that is no multiple of 4; w starts 3 floats
    into its buffer."""
    d, m, Nc, Nq, lead, guard = 64, 266, 65, 17, 3, 4096
    qd, state, vd, pd = _setup("live", d, m, Nc)
    rows = qd[:, :Nq].contiguous()
    want_out, want_w = gpulib.favor_query_long_fwd(rows, state.buf, vd, pd, weights=True)
    n, no = T * H * Nq * Nc, T * Nq * d * H
    buf = torch.full((lead + guard + n + guard,), float("nan"), device=DEV)
    obuf = torch.full((guard + no + guard,), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    w, out = buf[lead + guard:lead + guard + n], obuf[guard:guard + no]
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = gpulib.c.mlhot_favor_query_long_fwd(p(rows), p(state.buf), p(vd), p(pd), None, T, H, Nq, Nc, d, m, p(out), p(w), p(ws), 256, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(buf[:lead + guard]).all()) and bool(torch.isnan(buf[lead + guard + n:]).all())
    assert bool(torch.isnan(obuf[:guard]).all()) and bool(torch.isnan(obuf[guard + no:]).all())
    assert torch.equal(w.view(T, H, Nq, Nc), want_w) and torch.equal(out.view(T, Nq, d * H), want_out)


# ---- 7. the envelope -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,d,m", [(257, 16, 16), (40, 24, 32), (40, 16, 8), (40, 272, 32)])
def test_outside_the_envelope_nothing_is_written(gpulib, Nc, d, m):
    Nq = 5
    g = torch.Generator().manual_seed(3)
    q, k = (0.25 * torch.randn(T, n, H, d, generator=g).to(DEV) for n in (Nq, Nc))
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((1 << 16,), 7.0, device=DEV)
    out = torch.full((T, Nq, d * H), float("nan"), device=DEV)
    w = torch.full((T, H, Nq, Nc), float("nan"), device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    c = gpulib.c
    assert not gpulib.favor_long_supported(T, H, Nc, d, m) and gpulib.favor_keys_long_bytes(T, H, Nc, d, m) == 0
    assert c.mlhot_favor_keys_long_fwd(p(k), p(proj), None, T, H, Nc, d, m, p(state), state.numel() * 4, None) == 4      # MLHOT_ERR_UNSUPPORTED
    assert "favor_keys_long_fwd serves Nc <= 256" in c.mlhot_last_error().decode()
    assert c.mlhot_favor_query_long_fwd(p(q), p(state), p(k), p(proj), None, T, H, Nq, Nc, d, m, p(out), p(w), p(ws), 256, None) == 4
    assert "favor_query_long_fwd serves Nc <= 256" in c.mlhot_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(w).all()) and bool((state == 7.0).all())


def test_the_envelope_ends_at_256_slots_and_at_aligned_pointers(gpulib):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_keys_long
    assert gpulib.favor_long_supported(T, H, 256, 256, 1536) and gpulib.favor_long_supported(T, H, 1, 16, 16)
    assert not gpulib.favor_long_supported(T, H, 257, 256, 1536)
    d, m, Nc = 16, 16, 40
    k = torch.zeros(T * Nc * H * d + 1, device=DEV)[1:].view(T, Nc, H, d)          # 4 bytes off
    proj = torch.randn(m, d).to(DEV)
    state = torch.full((1 << 14,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert k.data_ptr() % 16 != 0
    assert gpulib.c.mlhot_favor_keys_long_fwd(p(k), p(proj), None, T, H, Nc, d, m, p(state), state.numel() * 4, None) == 4
    torch.cuda.synchronize()
    assert bool((state == 7.0).all())
    with pytest.raises(MlhotError, match="favor_keys_long serves Nc <= 256.*Nc=257"):
        favor_keys_long(torch.zeros(T, 257, H, d, device=DEV), proj)
    with pytest.raises(MlhotError, match=r"lens must lie in 1\.\.40"):
        favor_keys_long(torch.zeros(T, Nc, H, d, device=DEV), proj, lens=[0, 40])
