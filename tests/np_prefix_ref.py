"""Float64 restatement of the vanilla family's prefix sweep (mlhot.cached.sweep, csrc/np_prefix.h): tests/np_query_ref.py's
`condition` / `query_tail` applied to the first k context shots, for every k.  The synthetic cases are np_query_ref's kinds plus
key placements that move the batch-global stabiliser M_k (the maximum of the key logits over the first k shots) along the sweep:
    peak_first  the 50-above key at shot 0: M_k is the same for every k - one group
    peak_last   the peak at the last shot: the last prefix is alone in its group
    climb       every shot's maximum about 10 above the previous one: every prefix its own group
    equal       np_query_ref's all-equal keys."""
import functools

import torch

from tests import favor_cached_ref as R
from tests import np_query_ref as NR

T, HEADS, Y_DIM = NR.T, NR.HEADS, NR.Y_DIM
ATTENTION_KINDS = ("live", "big", "peak", "equal", "peak_first", "peak_last", "climb")
LATENT_KINDS = ("live", "big")


def _peak_key(d, m, height):
    """A key whose logit at feature m // 2 is `height` (np_query_ref's "peak" construction)."""
    pr = NR.proj_matrix(d, m)[m // 2]
    return pr * (height / (d ** -0.25 * float(pr @ pr)))


@functools.lru_cache(maxsize=None)
def case(kind, d, m, Nc, Nq):
    """(x [T, Nq, d], k [T, H, Nc, d], v [T, H, Nc, d], z [Nc, T, dim_z]) on the CPU; z[k - 1] is the latent of prefix k."""
    base = kind if kind in ("live", "big", "peak", "equal") else "live"
    x, k, v, _ = NR.case(base, d, m, Nc, Nq)
    g = torch.Generator().manual_seed(7000 + 1000 * d + m + 17 * Nc + len(kind))
    z = torch.randn(Nc, T, NR.DIM_Z[d], generator=g)
    if kind in ("peak_first", "peak_last", "climb"):
        k = 0.05 * torch.randn(T, HEADS, Nc, d, generator=g)
        if kind == "climb":
            for j in range(Nc):
                k[j % T, j % HEADS, j] = _peak_key(d, m, 10.0 * (j + 1))
        else:
            k[1, 0, 0 if kind == "peak_first" else Nc - 1] = _peak_key(d, m, 50.0)
    return x, k, v, z


def running_max(kind, d, m, Nc):
    """M_1 .. M_Nc in float64, [Nc]."""
    k = case(kind, d, m, Nc, 1)[1].double()
    dd = torch.einsum("thnd,md->thnm", d ** -0.25 * k, NR.proj_matrix(d, m).double())
    return torch.cummax(dd.amax(dim=(0, 1, 3)), dim=0).values


def group_boundary(kind, d, m, Nc):
    """The last k >= 2 at which M_k differs from M_(k-1) (a prefix that opens a group), or 1 when there is none."""
    M = running_max(kind, d, m, Nc)
    moved = [k for k in range(2, Nc + 1) if M[k - 1] != M[k - 2]]
    return moved[-1] if moved else 1


@functools.lru_cache(maxsize=None)
def want(kind, d, m, Nc, Nq, attend, tanh):
    """The float64 result for every prefix, [Nc, T, Nq, Y_DIM]."""
    x, k, v, z = case(kind, d, m, Nc, Nq)
    proj = NR.proj_matrix(d, m)
    out = []
    for kk in range(1, Nc + 1):
        if attend:
            state = {"kind": "attention", "fk": R.key_features(k[:, :, :kk], proj)[0], "vh": v[:, :, :kk].double()}
        else:
            state = {"kind": "latent", "z": z[kk - 1].double()}
        out.append(NR.query_tail(NR.params(d), x, state, tanh, proj))
    return torch.stack(out)
