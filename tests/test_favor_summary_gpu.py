"""The fixed-size FAVOR+ summary state on the MI355X (csrc/favor_summary.h): values and state contents against
float64 over every chunking and value case of tests/favor_summary_ref.py, masking, row invariance and determinism bit for bit,
agreement with the per-shot route, the envelope.  The bar is tests/test_condition_gpu.py's for favor_query against float64:
U.RTOL of out's scale.  Run with -m gpu."""
import ctypes as C

import pytest
import torch

from tests import favor_cached_ref as R
from tests import favor_summary_ref as S
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = S.H


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _absorb(c, poison=None):
    """favor_absorb over the case's calls; lens goes out only where a call is ragged (None is the kernels' NULL path).  `poison`:
    what the invalid slots of k and v hold."""
    from mlhot.ops import favor_absorb
    state, pd = None, c["proj"].to(DEV)
    for kc, vc, lens in c["chunks"]:
        n = kc.shape[2]
        if poison is not None:
            kc, vc = kc.clone(), vc.clone()
            for t, L in enumerate(lens):
                kc[t, :, L:], vc[t, :, L:] = poison, poison
        state = favor_absorb(state, _dev(kc), _dev(vc), pd, lens=None if all(L == n for L in lens) else lens)
    return state


def _live(d, m, T, Nc, Nq, seed=5):
    g = torch.Generator().manual_seed(seed + d + m + Nc)
    q, k = 0.25 * torch.randn(T, H, Nq, d, generator=g), 0.25 * torch.randn(T, H, Nc, d, generator=g)
    return q, k, torch.randn(T, H, Nc, d, generator=g), S.proj_for(d, m)


# ---- 1. values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("chunking", list(S.CHUNKINGS))
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_query_values_against_float64(gpulib, d, m, chunking, kind):
    from mlhot.ops import favor_query
    c = S.case(kind, d, m, chunking)
    want = R.merged(S.reference(c))
    state = _absorb(c)
    assert state.route == "summary" and list(state.lens) == c["totals"]
    qd, pd = _dev(c["q"]), c["proj"].to(DEV)
    got = favor_query(qd, state, None, pd)
    err = U.rel_err(got, want)
    line = f"summary favor_query {kind} d={d} m={m} {chunking}: {err:.2e} of out's scale"
    if len(set(c["totals"])) == 1:                   # mlhot_favor_fwd has no mask: it serves the uniform totals
        plain = gpulib.favor_fwd(qd, _dev(c["k"]), _dev(c["v"]), pd)[0]
        line += f"; mlhot_favor_fwd on the kept keys {U.rel_err(plain, want):.2e}"
    print(line)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= U.RTOL, line


# ---- 2. state contents ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["live", "peak_last", "peak_first_t0"])
@pytest.mark.parametrize("chunking", list(S.CHUNKINGS))
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_state_against_float64(gpulib, d, m, chunking, kind):
    from mlhot.ops import favor_keys
    c = S.case(kind, d, m, chunking)
    T, mp = c["T"], (m + 15) // 16 * 16
    A, a, vs, cnt, M = _absorb(c).summary()
    assert A.shape == (T, H, mp, d) and a.shape == (T, H, mp) and vs.shape == (T, H, d) and cnt.shape == (T, H) and cnt.dtype == torch.int32
    assert gpulib.favor_summary_bytes(T, H, d, m) >= 4 * (A.numel() + a.numel() + vs.numel() + 1 + cnt.numel())
    want = S.streamed(c)
    eA, ea, ev = U.rel_err(A[:, :, :m], want.A), U.rel_err(a[:, :, :m], want.a), U.rel_err(vs, want.vs)
    dd_scale = torch.einsum("thnd,md->thnm", d ** -0.25 * c["k"].double(), c["proj"].double()).abs().max().item()
    eM = abs(M.item() - want.M) / max(dd_scale, 1e-30)
    print(f"summary state {kind} d={d} m={m} {chunking}: A {eA:.2e}, a {ea:.2e}, vs {ev:.2e} of their scales, M {M.item():.4f} off by {eM:.2e} of dd's scale")
    assert max(eA, ea, ev, eM) <= U.RTOL
    assert cnt.cpu().tolist() == [[n] * H for n in c["totals"]]
    assert bool((A[:, :, m:] == 0).all()) and bool((a[:, :, m:] == 0).all())            # features >= m are exactly zero
    # M is the float32 maximum favor_keys reports on the same keys: per call and task where a call holds more tasks' shots than
    # favor_keys' mask can express (a task without a shot), over <= 32 shots each
    pd, seen = c["proj"].to(DEV), []
    for kc, _, lens in c["chunks"]:
        for t, L in enumerate(lens):
            if L:
                st = favor_keys(_dev(kc[t:t + 1, :, :L]), pd)
                assert st.route == "cached"
                seen.append(st.features()[1].item())
    assert M.item() == max(seen)


def test_a_fresh_state_and_an_absorb_without_a_shot(gpulib):
    from mlhot.ops import favor_absorb
    d, m, T = 64, 266, 2
    buf = gpulib.favor_summary_init(T, H, d, m, DEV)
    A, a, vs, cnt, M = gpulib.favor_summary_views(buf, T, H, d, m)
    assert M.item() == float("-inf") and not bool(A.any()) and not bool(a.any()) and not bool(vs.any()) and not bool(cnt.any())
    c = S.case("live", d, m, "ragged")
    kc, vc, _ = c["chunks"][0]
    pd = c["proj"].to(DEV)
    none = favor_absorb(None, _dev(kc), _dev(vc), pd, lens=[0, 0])
    A, a, vs, cnt, M = none.summary()
    assert M.item() == float("-inf") and not bool(A.any()) and not bool(cnt.any()) and none.lens == (0, 0)
    one = favor_absorb(none, _dev(kc), _dev(vc), pd, lens=[5, 0])                       # the first shots: no 0 x inf, no exp(-inf - -inf)
    A, a, vs, cnt, M = one.summary()
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(M).all()) and one.lens == (5, 0)
    assert not bool(A[1].any()) and cnt.cpu().tolist() == [[5, 5], [0, 0]]
    assert none.summary()[4].item() == float("-inf")                                 # the input state stays as it was


# ---- 3. masking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_rows_behind_lens_are_never_read(gpulib, d, m):
    c = S.case("live", d, m, "ragged")
    clean = _absorb(c).summary()
    for poison in (float("nan"), float("inf")):
        for x, y in zip(_absorb(c, poison=poison).summary(), clean):
            assert torch.equal(x, y)


# ---- 4. row invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(64, 266), (256, 1419)])
def test_query_rows_do_not_depend_on_the_launch(gpulib, d, m):
    from mlhot.ops import favor_absorb, favor_query
    T = S.tasks(d, m)
    q, k, v, proj = _live(d, m, T, 40, 40)
    qd, pd = _dev(q), proj.to(DEV)
    state = favor_absorb(None, _dev(k), _dev(v), pd)                    # 40 shots in one call: two kernel calls of 32 and 8
    assert state.lens == (40,) * T
    full = favor_query(qd, state, None, pd)
    assert full.shape == (T, 40, d * H) and U.rel_err(full, R.merged(R.attention(q, k, v, proj))) <= U.RTOL

    def run(rows):
        return favor_query(rows.contiguous(), state, None, pd)
    for n in (0, 15, 16, 39):
        assert torch.equal(run(qd[:, n:n + 1]), full[:, n:n + 1]), n
    for start in (0, 3):
        for L in (15, 16, 17):
            assert torch.equal(run(qd[:, start:start + L]), full[:, start:start + L]), (start, L)
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(run(qd[:, perm]), full[:, perm])
    big = 3.0 * torch.randn(T, 100, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)           # other rows, another regime
    big[:, 37:77] = qd
    assert torch.equal(run(big)[:, 37:77], full)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(64, 266), (256, 1419)])
def test_the_same_calls_give_the_same_bits_and_in_place_equals_out_of_place(gpulib, d, m):
    from mlhot.ops import favor_query
    c = S.case("live", d, m, "7_32_31")
    qd, pd = _dev(c["q"]), c["proj"].to(DEV)
    s1, s2 = _absorb(c), _absorb(c)
    for x, y in zip(s1.summary(), s2.summary()):
        assert torch.equal(x, y)
    assert torch.equal(favor_query(qd, s1, None, pd), favor_query(qd, s2, None, pd))
    T = c["T"]
    views = lambda buf: gpulib.favor_summary_views(buf, T, H, d, m)
    apart = aliased = gpulib.favor_summary_init(T, H, d, m, DEV)
    aliased = aliased.clone()
    for kc, vc, _ in c["chunks"]:
        kd, vd = _dev(kc), _dev(vc)
        before = [x.clone() for x in views(apart)]
        nxt = gpulib.favor_summary_absorb(kd, vd, pd, apart)                       # state_in != state_out
        for x, y in zip(views(apart), before):
            assert torch.equal(x, y)                                            # the input state is left as it is
        apart = nxt
        assert gpulib.favor_summary_absorb(kd, vd, pd, aliased, out=aliased) is aliased      # state_in == state_out
        for x, y in zip(views(apart), views(aliased)):
            assert torch.equal(x, y)
    for x, y in zip(views(apart), s1.summary()):
        assert torch.equal(x, y)


# ---- 6. today's route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", [15, 32])
@pytest.mark.parametrize("d,m", S.SHAPES)
def test_summary_and_cached_routes_meet_the_same_bar(gpulib, d, m, Nc):
    from mlhot.ops import favor_absorb, favor_keys, favor_query
    T = S.tasks(d, m)
    q, k, v, proj = _live(d, m, T, Nc, 33)
    want = R.merged(R.attention(q, k, v, proj))
    qd, kd, vd, pd = _dev(q), _dev(k), _dev(v), proj.to(DEV)
    cached = favor_keys(kd, pd)
    assert cached.route == "cached"
    summary = favor_absorb(None, kd, vd, pd)
    e_c, e_s = U.rel_err(favor_query(qd, cached, vd, pd), want), U.rel_err(favor_query(qd, summary, None, pd), want)
    print(f"d={d} m={m} Nc={Nc}: cached favor_query {e_c:.2e}, summary favor_query {e_s:.2e} of out's scale")
    assert e_c <= U.RTOL and e_s <= U.RTOL
    assert summary.summary()[4].item() == cached.features()[1].item()                # one stabiliser, to the bit


# ---- 7. envelope ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(24, 32), (16, 1537)])
def test_outside_the_envelope(gpulib, d, m):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_absorb
    T, n, Nq = 2, 4, 5
    c = gpulib.c
    assert c.mlhot_favor_summary_bytes(T, H, d, m) == 0 and c.mlhot_favor_summary_ws_bytes(T, H, n, d, m) == 0
    assert c.mlhot_favor_summary_query_ws_bytes(T, H, Nq, d, m) == 0
    assert c.mlhot_favor_summary_ws_bytes(T, H, 33, 16, 16) == 0 and c.mlhot_favor_summary_ws_bytes(T, H, 32, 16, 16) > 0
    g = torch.Generator().manual_seed(3)
    q, k, v = (0.25 * torch.randn(T, r, H, d, generator=g).to(DEV) for r in (Nq, n, n))
    proj = torch.randn(m, d, generator=g).to(DEV)
    state = torch.full((1 << 16,), 7.0, device=DEV)
    out = torch.full((T, Nq, d * H), 7.0, device=DEV)
    ws = torch.full((1 << 16,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    nb = 4 * state.numel()
    assert c.mlhot_favor_summary_init(T, H, d, m, p(state), nb, None) == 4                         # MLHOT_ERR_UNSUPPORTED
    assert c.mlhot_favor_summary_absorb(p(k), p(v), p(proj), None, T, H, n, d, m, p(state), p(state), nb, p(ws), nb, None) == 4
    assert c.mlhot_favor_summary_query_fwd(p(q), p(state), p(proj), T, H, Nq, d, m, p(out), p(ws), nb, None) == 4
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((out == 7.0).all()) and bool((ws == 7.0).all())
    with pytest.raises(MlhotError, match="favor_absorb serves"):
        favor_absorb(None, k, v, proj)
