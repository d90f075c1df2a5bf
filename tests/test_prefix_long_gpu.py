"""mlhot.ops.favor_prefixes_long on the MI355X (csrc/favor_prefix_long.h): values against float64 over the shapes,
context sizes, target counts, prefix sets and value kinds of tests/prefix_long_ref.py, equivalence with today's prefix route and with
mlhot_favor_fwd on the sliced context, masking, row invariance and determinism bit for bit, the envelope.  The bar is the project's
U.RTOL of out's scale.  Every figure is printed before it is asserted.  Run with -m gpu."""
import ctypes as C

import pytest
import torch

from tests import prefix_long_ref as L
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = L.T, L.H


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _inputs(c, Nq=None):
    q = c["q"] if Nq is None else c["q"][:, :, :Nq]
    return _dev(q), _dev(c["k"]), _dev(c["v"]), c["proj"].to(DEV)


# ---- 1. values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("Nc", L.NCS)
@pytest.mark.parametrize("d,m", L.SHAPES)
def test_values_against_float64(gpulib, d, m, Nc, kind):
    """Every Nq of L.NQS x every prefix set of L.ks_sets(Nc); with it out[k] against mlhot_favor_fwd on the sliced context, both
    against float64 and against each other, at U.RTOL."""
    from mlhot.ops import favor_prefixes_long
    c = L.case(kind, d, m, Nc)
    worst, worst_plain, worst_between = 0.0, 0.0, 0.0
    for Nq in L.NQS:
        qd, kd, vd, pd = _inputs(c, Nq)
        for name, ks in L.ks_sets(Nc).items():
            got = favor_prefixes_long(qd, kd, vd, pd, ks)
            want = L.want(kind, d, m, Nc, ks, Nq)
            assert got.shape == want.shape == (len(ks), T, Nq, d * H) and bool(torch.isfinite(got).all()), (Nq, name)
            err = U.rel_err(got, want)
            worst = max(worst, err)
            assert err <= U.RTOL, f"{kind} d={d} m={m} Nc={Nc} Nq={Nq} ks={name}: {err:.2e} of out's scale"
            if name == "1_32_33_Nc":
                for i, k in enumerate(ks):
                    plain = gpulib.favor_fwd(qd, kd[:, :k].contiguous(), vd[:, :k].contiguous(), pd)[0]
                    worst_plain = max(worst_plain, U.rel_err(plain, want[i]))
                    worst_between = max(worst_between, U.rel_err(got[i], plain))
    line = (f"favor_prefixes_long {kind} d={d} m={m} Nc={Nc}: {worst:.2e} of out's scale against float64; mlhot_favor_fwd on the sliced "
            f"context {worst_plain:.2e}; one against the other {worst_between:.2e}")
    print(line)
    U.parity_log(line)
    assert worst_between <= U.RTOL, line


@pytest.mark.parametrize("kind", ["live", "big"])
@pytest.mark.parametrize("Nc", [1, 31, 32])
@pytest.mark.parametrize("d,m", L.SHAPES)
def test_up_to_32_shots_the_op_equals_todays_prefix_route(gpulib, d, m, Nc, kind):
    from mlhot.ops import favor_prefixes, favor_prefixes_long
    qd, kd, vd, pd = _inputs(L.case(kind, d, m, Nc))
    assert gpulib.favor_prefix_supported(T, H, qd.shape[1], Nc, d, m)
    old, new = favor_prefixes(qd, kd, vd, pd), favor_prefixes_long(qd, kd, vd, pd)
    err = U.rel_err(new, old)
    line = f"favor_prefixes_long against favor_prefixes {kind} d={d} m={m} Nc={Nc}: {err:.2e} of out's scale"
    print(line)
    U.parity_log(line)
    assert old.shape == new.shape and err <= U.RTOL, line


# ---- 2. masking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,lens", [(Nc, lens) for Nc, many in L.LENS.items() for lens in many])
@pytest.mark.parametrize("d,m", L.SHAPES)
def test_rows_behind_lens_are_never_read(gpulib, d, m, Nc, lens):
    from mlhot.ops import favor_prefixes_long
    c = L.case("live", d, m, Nc)
    ks = L.ks_sets(Nc)["edges"]
    want = L.merged(L.streamed(c["q"], c["k"], c["v"], c["proj"], ks, lens)[0])
    qd, kd, vd, pd = _inputs(c)
    clean = favor_prefixes_long(qd, kd, vd, pd, ks, lens=lens)
    err = U.rel_err(clean, want)
    print(f"favor_prefixes_long lens={lens} d={d} m={m} Nc={Nc}: {err:.2e} of out's scale")
    assert bool(torch.isfinite(clean).all()) and err <= U.RTOL
    for poison in (float("nan"), float("inf")):
        kp, vp = kd.clone(), vd.clone()
        for t, n in enumerate(lens):
            kp[t, n:], vp[t, n:] = poison, poison
        assert torch.equal(favor_prefixes_long(qd, kp, vp, pd, ks, lens=torch.tensor(lens)), clean)
    # a full lens is the unmasked call, bit for bit
    assert torch.equal(favor_prefixes_long(qd, kd, vd, pd, ks, lens=(Nc,) * T), favor_prefixes_long(qd, kd, vd, pd, ks))


def test_lens_are_checked_on_the_host(gpulib):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_prefixes_long
    qd, kd, vd, pd = _inputs(L.case("live", 16, 16, 33))
    for bad in ((0, 33), (1, 34), (5,), (1.0, 2.0)):
        with pytest.raises(MlhotError, match="favor_prefixes_long: lens"):
            favor_prefixes_long(qd, kd, vd, pd, [1, 33], lens=bad)


# ---- 3. row invariance and determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(64, 266), (256, 1419)])
def test_rows_and_prefixes_do_not_depend_on_the_launch(gpulib, d, m):
    from mlhot.ops import favor_prefixes_long
    Nc, Nq = 97, 40
    g = torch.Generator().manual_seed(5 + d + m)
    q, k = 0.25 * torch.randn(T, Nq, H, d, generator=g), 0.25 * torch.randn(T, Nc, H, d, generator=g)
    v, pd = torch.randn(T, Nc, H, d, generator=g).to(DEV), L.S.proj_for(d, m).to(DEV)
    qd, kd = q.to(DEV), k.to(DEV)
    ks = L.ks_sets(Nc)["edges"]
    full = favor_prefixes_long(qd, kd, v, pd, ks)

    def run(rows, sizes=ks):
        return favor_prefixes_long(rows.contiguous(), kd, v, pd, sizes)
    assert torch.equal(run(qd), full)                                            # two runs of the same input
    for n in (0, 15, 16, 39):
        assert torch.equal(run(qd[:, n:n + 1]), full[:, :, n:n + 1]), n
    for start in (0, 3):
        for n in (15, 16, 17):
            assert torch.equal(run(qd[:, start:start + n]), full[:, :, start:start + n]), (start, n)
    perm = torch.randperm(Nq, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(run(qd[:, perm]), full[:, :, perm])
    big = 3.0 * torch.randn(T, 100, H, d, generator=torch.Generator().manual_seed(9)).to(DEV)       # 100 rows, another regime around them
    big[:, 37:77] = qd
    assert torch.equal(run(big)[:, :, 37:77], full)
    # a prefix has the same bits whichever others are asked for: all 97 sizes go out as 64 + 33, the halves alone, single sizes
    every = run(qd, None)
    assert every.shape[0] == Nc and torch.equal(every[[x - 1 for x in ks]], full)
    assert torch.equal(torch.cat([run(qd, list(range(1, 51))), run(qd, list(range(51, 98)))]), every)
    for x in (1, 33, 97):
        assert torch.equal(run(qd, [x])[0], every[x - 1])


# ---- 4. envelope ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,K", [(24, 32, 2), (8, 32, 2), (272, 32, 2), (16, 15, 2), (16, 1537, 2), (16, 16, 65), (16, 16, 0)])
def test_outside_the_envelope(gpulib, d, m, K):
    from mlhot.binding import MlhotError
    from mlhot.ops import favor_prefixes_long
    Nq, Nc = 5, 70
    c = gpulib.c
    assert c.mlhot_favor_prefix_long_supported(T, H, Nq, Nc, d, m, K) == 0
    assert c.mlhot_favor_prefix_long_workspace_bytes(T, H, Nq, Nc, d, m, K) == 0
    assert c.mlhot_favor_prefix_long_supported(T, H, Nq, Nc, 16, 16, 64) == 1 and c.mlhot_favor_prefix_long_supported(T, H, Nq, Nc, 256, 1536, 1) == 1
    g = torch.Generator().manual_seed(3)
    q, k, v = (0.25 * torch.randn(T, r, H, d, generator=g).to(DEV) for r in (Nq, Nc, Nc))
    proj = torch.randn(m, d, generator=g).to(DEV)
    out = torch.full((max(K, 1), T, Nq, d * H), 7.0, device=DEV)
    ws = torch.full((1 << 20,), 7.0, device=DEV)
    ks = (C.c_int32 * max(K, 1))(*range(1, max(K, 1) + 1))
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = c.mlhot_favor_prefix_long_fwd(p(q), p(k), p(v), p(proj), ks, K, None, T, H, Nq, Nc, d, m, p(out), p(ws), 4 * ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == (4 if K > 0 else 1)                                             # MLHOT_ERR_UNSUPPORTED; K = 0 is a bad argument
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())
    if K > 0 and K <= 64:
        with pytest.raises(MlhotError, match="favor_prefixes_long serves"):
            favor_prefixes_long(q, k, v, proj, list(range(1, K + 1)))


def test_bad_ks_and_a_small_workspace_write_nothing(gpulib):
    d, m, Nq, Nc = 16, 16, 5, 40
    qd, kd, vd, pd = _inputs(L.case("live", d, m, 33), Nq)
    c = gpulib.c
    out = torch.full((2, T, Nq, d * H), 7.0, device=DEV)
    need = c.mlhot_favor_prefix_long_workspace_bytes(T, H, Nq, 33, d, m, 2)
    ws = torch.full((need // 4 + 64,), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda ks, nb: c.mlhot_favor_prefix_long_fwd(p(qd), p(kd), p(vd), p(pd), (C.c_int32 * 2)(*ks), 2, None, T, H, Nq, 33, d, m, p(out), p(ws), nb, None)
    assert need > 0 and Nc > 33
    assert call((1, 34), need) == 1 and call((0, 5), need) == 1 and call((5, 5), need) == 1              # MLHOT_ERR_ARG
    assert call((1, 33), need - 1) != 0                                                                  # MLHOT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())
    assert call((1, 33), need) == 0
