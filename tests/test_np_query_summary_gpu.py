"""The one-launch query tail on a FAVOR+ summary state on the MI355X (csrc/np_query_summary.h), operator level:
values against float64 next to the composed route's on the same state, row invariance bit for bit, the rows behind Nq, states that
came out of merge and gather, scaled keys, and the refusals.  T = 2, 8 heads.  Run with -m gpu."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import favor_summary_ref as S
from tests import np_query_summary_ref as QS
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H = QS.T, QS.HEADS
SHAPES = [(16, 16), (32, 40), (64, 266)]        # the smallest of everything; mp = 48 > m; the shipped one, a ragged last 16-feature chunk
COUNTS = [(1, 1), (33, 7), (100, 64)]           # shots per task; the last crosses absorb's 32-shot chunks and carries a rescale
NQS = (1, 15, 16, 17, 100)                      # both sides of the 16-row tile edge
NQ = 100


@functools.lru_cache(maxsize=None)
def _params(d):
    return {k: v.to(DEV) for k, v in QS.params(d).items()}


def _dims(gpulib, d, m, Nc=1):
    return gpulib.np_dims(T, Nc, 1, 3, QS.Y_DIM, d, d, QS.DIM_Z[d], [100, 100], QS.HIDDEN, "attention", QS.tanh_for(d), m)


def _absorbed(k, v, proj, lens):
    """mlhot.ops.favor_absorb's state of shots k, v [T, H, N, d] (the oracle's layout), task t's first lens[t] rows."""
    from mlhot.ops import favor_absorb
    kh, vh = (t.permute(0, 2, 1, 3).contiguous().to(DEV) for t in (k, v))
    return favor_absorb(None, kh, vh, proj.to(DEV), lens=list(lens))


class _Setup:
    """One case on the device: fused(x) is the launch, composed(x) the parent commit's operators on the same state."""

    def __init__(self, gpulib, d, m, state):
        self.lib, self.d, self.m, self.state, self.p = gpulib, d, m, state, _params(d)
        self.proj = QS.proj_matrix(d, m).to(DEV)
        self.dims = _dims(gpulib, d, m, max(state.lens))
        assert gpulib.np_query_summary_supported(self.dims) and state.route == "summary"

    def fused(self, x, out=None):
        return self.lib.np_query_summary_fwd(self.dims, self.p, x.contiguous(), self.state.buf, self.proj, out=out)

    def composed(self, x):
        from mlhot.cached import composed_tail
        x = x.contiguous()
        with torch.no_grad():
            return composed_tail(self.p, x.view(-1, self.d), T, x.shape[1], QS.tanh_for(self.d), keys=self.state, vh=None, proj=self.proj)


@functools.lru_cache(maxsize=None)
def _case(d, m, counts, key_scale=1.0):
    """(x on the device, the absorbed state, float64 mu for all NQ rows); the reference's state is built in float64 from the shots."""
    x, k, v = QS.case(d, m, max(counts), NQ, key_scale)
    proj = QS.proj_matrix(d, m)
    want = QS.tail_of_state(QS.params(d), x, QS.state_from_shots(k, v, proj, counts), proj, QS.tanh_for(d))
    return x.to(DEV), _absorbed(k, v, proj, counts), want


def _check(s, x, want, what):
    for Nq in NQS:
        fused, composed = s.fused(x[:, :Nq]), s.composed(x[:, :Nq])
        ef, ec, fc = U.rel_err(fused, want[:, :Nq]), U.rel_err(composed, want[:, :Nq]), U.rel_err(fused, composed)
        line = (f"np_query_summary {what} d={s.d} m={s.m} Nq={Nq}: fused {ef:.2e}, composed {ec:.2e} of mu's scale against float64; "
                f"fused against composed {fc:.2e}, torch.equal {torch.equal(fused, composed)}")
        print(line)
        assert fused.shape == (T, Nq, QS.Y_DIM) and bool(torch.isfinite(fused).all()), line
        assert ef <= U.RTOL and fc <= U.RTOL, line


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: f"shots{c[0]}_{c[1]}")
@pytest.mark.parametrize("d,m", SHAPES)
def test_values_against_float64_and_the_composed_route(gpulib, d, m, counts):
    x, state, want = _case(d, m, counts)
    assert state.lens == counts
    _check(_Setup(gpulib, d, m, state), x, want, f"shots {counts}")


@pytest.mark.parametrize("d,m", SHAPES)
def test_scaled_keys(gpulib, d, m):
    """Key rows scaled by 4: a wide spread of exp, most key features far below the stabiliser."""
    x, state, want = _case(d, m, (33, 7), 4.0)
    _check(_Setup(gpulib, d, m, state), x, want, "keys x 4")


# ---- 2. invariance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", SHAPES)
def test_rows_do_not_depend_on_the_launch(gpulib, d, m):
    x, state, _ = _case(d, m, (100, 64))
    s = _Setup(gpulib, d, m, state)
    full = s.fused(x)
    assert full.shape == (T, NQ, QS.Y_DIM) and bool(torch.isfinite(full).all())
    for n in (0, 15, 16, 57, 99):                                     # a row alone
        assert torch.equal(s.fused(x[:, n:n + 1]), full[:, n:n + 1]), n
    for start, L in ((0, 15), (0, 16), (0, 17), (3, 15), (3, 16), (3, 17), (31, 33)):
        assert torch.equal(s.fused(x[:, start:start + L]), full[:, start:start + L]), (start, L)
    perm = torch.randperm(NQ, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert torch.equal(s.fused(x[:, perm]), full[:, perm])
    big = 3.0 * torch.randn(T, 200, d, generator=torch.Generator().manual_seed(9)).to(DEV)              # other rows, another regime
    big[:, 37:137] = x
    assert torch.equal(s.fused(big)[:, 37:137], full)


@pytest.mark.parametrize("d,m", SHAPES)
def test_rows_behind_nq_are_never_stored(gpulib, d, m):
    x, state, _ = _case(d, m, (33, 7))
    s = _Setup(gpulib, d, m, state)
    Nq = 17                                                           # the second tile holds one row and fifteen that do not exist
    n = T * Nq * QS.Y_DIM
    buf = torch.full((n + 96,), 7.0, device=DEV)
    out = buf[32:32 + n].view(T, Nq, QS.Y_DIM)                       # 128 bytes in: aligned
    got = s.fused(x[:, :Nq], out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, s.fused(x[:, :Nq])) and not bool((out == 7.0).any())
    assert bool((buf[:32] == 7.0).all()) and bool((buf[32 + n:] == 7.0).all())


# ---- 3. states that did not come straight from absorb ------------------------------------------------------------------------------------
def _combine(states, picks):
    """The float64 state gather / merge build: task t = the sum of picks[t] = [(state, task), ..], rescaled to M' = the maximum of
    ALL the states' stabilisers."""
    d, m = states[0].vs.shape[-1], states[0].a.shape[-1]
    out = S.State(len(picks), H, d, m)
    out.M = max(st.M for st in states)
    for t, row in enumerate(picks):
        for i, u in row:
            f = math.exp(states[i].M - out.M)
            out.A[t] += f * states[i].A[u]
            out.a[t] += f * states[i].a[u]
            out.vs[t] += states[i].vs[u]
            out.cnt[t] += states[i].cnt[u]
    return out


@functools.lru_cache(maxsize=None)
def _two_states(d, m):
    """Two absorbed states with different stabilisers (the second one's keys are twice as large), on the device and in float64."""
    proj = QS.proj_matrix(d, m)
    x, ka, va = QS.case(d, m, 33, NQ)
    _, kb, vb = QS.case(d, m, 20, NQ, 2.0)
    la, lb = (33, 7), (20, 11)
    dev = (_absorbed(ka, va, proj, la), _absorbed(kb, vb, proj, lb))
    ref = (QS.state_from_shots(ka, va, proj, la), QS.state_from_shots(kb, vb, proj, lb))
    assert ref[1].M > ref[0].M + 0.5                                 # the first state's scale is below 1, M' above its tasks' own maxima
    return x.to(DEV), dev, ref


@pytest.mark.parametrize("d,m", SHAPES)
def test_a_merged_state(gpulib, d, m):
    from mlhot.ops import favor_merge
    x, dev, ref = _two_states(d, m)
    state = favor_merge(list(dev))
    assert state.lens == (53, 18)
    want = QS.tail_of_state(QS.params(d), x.cpu(), _combine(ref, [[(0, 0), (1, 0)], [(0, 1), (1, 1)]]), QS.proj_matrix(d, m), QS.tanh_for(d))
    _check(_Setup(gpulib, d, m, state), x, want, "merged")


@pytest.mark.parametrize("d,m", SHAPES)
def test_a_gathered_state(gpulib, d, m):
    from mlhot.ops import favor_gather
    x, dev, ref = _two_states(d, m)
    picks = [[(0, 1)], [(1, 0), (0, 0)]]                              # a permutation, and a two-part pick; task 0 keeps M' from state 1
    state = favor_gather(list(dev), picks)
    assert state.lens == (7, 53)
    want = QS.tail_of_state(QS.params(d), x.cpu(), _combine(ref, picks), QS.proj_matrix(d, m), QS.tanh_for(d))
    _check(_Setup(gpulib, d, m, state), x, want, "gathered")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(gpulib, dims, ps, x, Nq, state, mu_ptr):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    return gpulib.c.mlhot_np_query_summary_fwd(C.byref(dims), C.byref(ps), p(x), Nq, p(state), mu_ptr, None)


def _np_params(d, m):
    from mlhot.binding import NpParams, _set, vanilla_param_map
    ps, p = NpParams(), _params(d)
    for path, key in vanilla_param_map(2, False, True):
        if key in p:
            _set(ps, path, p[key].data_ptr())
    proj = QS.proj_matrix(d, m).to(DEV)
    ps.proj = proj.data_ptr()
    return ps, proj


def test_refusals_write_nothing(gpulib):
    from mlhot.binding import NpParams
    Nq = 5
    mu = torch.full((T * Nq * 2 + 4,), 7.0, device=DEV)
    at = C.c_void_p(mu.data_ptr())
    state = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for d, m in ((24, 32), (64, 288), (64, 8), (80, 266)):            # outside the envelope: MLHOT_ERR_UNSUPPORTED before anything is read
        dims = gpulib.np_dims(T, 40, 1, 3, 2, d, d, 12, [100, 100], 100, "attention", True, m)
        assert not gpulib.np_query_summary_supported(dims), (d, m)
        assert _raw(gpulib, dims, NpParams(), torch.randn(T, Nq, d, device=DEV), Nq, state, at) == 4, (d, m)
    assert not gpulib.np_query_summary_supported(gpulib.np_dims(T, 40, 1, 3, 2, 64, 64, 64, [100, 100], 100, "mean", True, 0))
    for dz, dh, y in ((68, 100, 2), (64, 132, 2), (64, 100, 17), (62, 100, 2), (64, 98, 2)):
        assert not gpulib.np_query_summary_supported(gpulib.np_dims(T, 40, 1, 3, y, 64, 64, dz, [100, 100], dh, "attention", True, 266)), (dz, dh, y)
    # inside it (whatever Nc says): a misaligned mu is unsupported, a NULL pointer or Nq < 1 a bad argument
    d, m = 16, 16
    x, st, _ = _case(d, m, (1, 1))
    for Nc in (0, 1, 4000):
        assert gpulib.np_query_summary_supported(_dims(gpulib, d, m, Nc))
    dims = _dims(gpulib, d, m)
    ps, proj = _np_params(d, m)
    xs = x[:, :Nq].contiguous()
    assert _raw(gpulib, dims, ps, xs, Nq, st.buf, C.c_void_p(mu.data_ptr() + 4)) == 4
    assert "16-byte aligned" in gpulib.c.mlhot_last_error().decode()
    assert _raw(gpulib, dims, ps, xs, 0, st.buf, at) == 1             # MLHOT_ERR_ARG
    assert _raw(gpulib, dims, ps, None, Nq, st.buf, at) == 1
    assert _raw(gpulib, dims, ps, xs, Nq, None, at) == 1
    assert _raw(gpulib, dims, ps, xs, Nq, st.buf, None) == 1
    assert _raw(gpulib, dims, NpParams(), xs, Nq, st.buf, at) == 1    # no parameters
    torch.cuda.synchronize()
    assert bool((mu == 7.0).all())
    assert _raw(gpulib, dims, ps, xs, Nq, st.buf, at) == 0            # and the same call with everything in place runs
    torch.cuda.synchronize()
    assert torch.equal(mu[:T * Nq * 2].view(T, Nq, 2), gpulib.np_query_summary_fwd(dims, _params(d), xs, st.buf, proj)) and bool((mu[T * Nq * 2:] == 7.0).all())
