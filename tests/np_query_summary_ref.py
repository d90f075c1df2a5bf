"""Float64 statement of the one-launch query tail on a FAVOR+ summary state (csrc/np_query_summary.h): from the
state's A, a, vs, cnt, the encoder's target rows and the query-side parameters to mu.  The attention part is
tests/favor_summary_ref.py's query, everything around it tests/np_query_ref.py's; `params` and `case` make the kernel tests'
synthetic parameters and inputs at the head widths the tests use."""
import functools

import torch

from tests import favor_cached_ref as R
from tests import favor_summary_ref as S
from tests import np_query_ref as NR

HEADS, T = NR.HEADS, NR.T
HIDDEN, Y_DIM = NR.HIDDEN, NR.Y_DIM
DIM_Z = {16: 12, 32: 20, 64: 64}        # by head width: two z widths that are no multiple of the 16-column tile, and the shipped one
EPS = S.EPS


def query_tail(p, x_qry, A, a, vs, cnt, proj, tanh):
    """x_qry [T, Nq, dim_w], the state's A [T, H, m, d], a [T, H, m], vs [T, H, d], cnt (T shot counts, all >= 1) -> mu [T, Nq, y_dim]."""
    fq = R.query_features(NR.heads(x_qry, p, "_W_q"), proj, EPS)                                   # [T, H, Nq, m]
    fs = fq.sum(dim=-1, keepdim=True)
    n = torch.as_tensor(cnt, dtype=torch.float64)[:, None, None]
    num = torch.einsum("thqm,thme->thqe", fq, A.double()) + EPS * fs * vs.double()[:, :, None, :]
    den = torch.einsum("thqm,thm->thq", fq, a.double()) + EPS * n * fs[..., 0]
    z = NR._lin(NR._lin(R.merged(num / den[..., None]), p, "_W.linear"), p, "r_to_z")
    return NR.decoder(x_qry, z, p, tanh)


def state_from_shots(k, v, proj, lens=None, chunk=32):
    """The float64 summary state of shots k, v [T, H, N, d] (task t's first lens[t] rows), absorbed `chunk` at a time."""
    Tn, H, N, d = k.shape
    lens = [N] * Tn if lens is None else list(lens)
    st = S.State(Tn, H, d, proj.shape[0])
    for s in range(0, N, chunk):
        st.absorb(k[:, :, s:s + chunk], v[:, :, s:s + chunk], proj, [min(max(n - s, 0), min(chunk, N - s)) for n in lens])
    return st


def tail_of_state(p, x_qry, st, proj, tanh):
    return query_tail(p, x_qry, st.A, st.a, st.vs, st.cnt, proj, tanh)


# ---- the kernel tests' synthetic cases ------------------------------------------------------------------------------------------------
def tanh_for(d):
    return d == 64             # the shipped width runs decoder0's tanh, the small ones the plain head


proj_matrix = NR.proj_matrix


@functools.lru_cache(maxsize=None)
def params(d):
    """Query-side parameters at head width d = dim_w = dim_r: tests/np_query_ref.py's where it has them, its recipe otherwise."""
    if d in NR.DIM_Z:
        assert NR.DIM_Z[d] == DIM_Z[d]
        return NR.params(d)
    g = torch.Generator().manual_seed(31 + d)
    dz = DIM_Z[d]
    p = {}

    def lin(name, n_out, n_in):
        p[name + ".weight"] = torch.randn(n_out, n_in, generator=g) * n_in ** -0.5
        p[name + ".bias"] = 0.1 * torch.randn(n_out, generator=g)
    for i in range(HEADS):
        lin(f"_W_q.{i}.linear", d, d)
    lin("_W.linear", d, HEADS * d)
    lin("r_to_z", dz, d)
    lin("decoder0.0", HIDDEN, d + dz)
    lin("decoder0.2", HIDDEN, HIDDEN)
    lin("decoder0.4", Y_DIM, HIDDEN)
    return p


@functools.lru_cache(maxsize=None)
def case(d, m, N, Nq, key_scale=1.0):
    """(x [T, Nq, d], k, v [T, H, N, d]) on the CPU, fp32: the encoder's target rows and the context's head projections."""
    g = torch.Generator().manual_seed(1000 * d + m + 17 * N)
    x = 0.25 * torch.randn(T, Nq, d, generator=g)
    k = key_scale * 0.25 * torch.randn(T, HEADS, N, d, generator=g)
    v = torch.randn(T, HEADS, N, d, generator=g)
    return x, k, v
