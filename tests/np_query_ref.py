"""Float64 restatement of the vanilla family's cached-context path (mlhot/cached.py, csrc/np_query.h): `condition` - what the
forward computes from the context alone - and `query_tail` - everything behind the encoder that sees the targets.  The attention
part is tests/favor_cached_ref.py's split FAVOR+.  Parameters travel as a dict with the models' state_dict keys; `case` makes the
kernel tests' synthetic parameters and inputs (the cached-FAVOR tests' input kinds)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import favor_cached_ref as R
from tests import util as U

HEADS = 8


def _lin(x, p, name):
    return F.linear(x.double(), p[name + ".weight"].double(), p[name + ".bias"].double())


def heads(x, p, name):
    """[T, N, k] -> [T, H, N, d]: the eight per-head Linears."""
    return torch.stack([_lin(x, p, f"{name}.{i}.linear") for i in range(HEADS)], dim=1)


def decoder(x, z, p, tanh):
    h = torch.relu(_lin(torch.cat([x.double(), z.double()], dim=-1), p, "decoder0.0"))
    mu = _lin(torch.relu(_lin(h, p, "decoder0.2")), p, "decoder0.4")
    return torch.tanh(mu) if tanh else mu


def encoder_fc(x, p):
    names = sorted((k[:-7] for k in p if k.startswith("encoder_r.layers.") and k.endswith(".weight")), key=lambda k: int(k.split(".")[-1]))
    for name in names[:-1]:
        x = torch.relu(_lin(x, p, name))
    return _lin(x, p, names[-1])


def condition(p, x_ctx, ctx_y, agg_mode, proj=None):
    """x_ctx [T, Nc, dim_w] (the encoder's context rows), ctx_y [T, Nc, L] -> the state as a dict: kind "attention" (fk [T, H, Nc, m],
    vh [T, H, Nc, d]), "latent" (z [T, dim_z]) or "empty" (z zeros)."""
    T, Nc = x_ctx.shape[:2]
    if Nc == 0:
        return {"kind": "empty", "z": torch.zeros(T, p["r_to_z.weight"].shape[0], dtype=torch.float64)}
    rs = encoder_fc(torch.cat([x_ctx.double(), _lin(ctx_y, p, "transform_y")], dim=-1), p)
    if agg_mode == "attention":
        return {"kind": "attention", "fk": R.key_features(heads(x_ctx, p, "_W_k"), proj)[0], "vh": heads(rs, p, "_W_v")}
    if agg_mode == "mean":
        r = rs.mean(dim=1)
    elif agg_mode == "max":
        r = rs.max(dim=1).values
    else:
        assert agg_mode == "baco"
        inv = 1.0 / (1e-5 + F.softplus(_lin(rs, p, "rs_to_var")))
        r = (inv * _lin(rs, p, "rs_to_mu")).sum(dim=1) / (1.0 + inv.sum(dim=1))
    return {"kind": "latent", "z": _lin(r, p, "r_to_z")}


def query_tail(p, x_qry, state, tanh, proj=None):
    """x_qry [T, Nq, dim_w] (the encoder's target rows) and a state of `condition` -> mu [T, Nq, y_dim]; row-wise in the targets."""
    T, Nq = x_qry.shape[:2]
    if state["kind"] == "attention":
        out = R.query(heads(x_qry, p, "_W_q"), state["fk"], state["vh"], proj)
        z = _lin(_lin(R.merged(out), p, "_W.linear"), p, "r_to_z")
    else:
        z = state["z"][:, None, :].expand(T, Nq, -1)
    return decoder(x_qry, z, p, tanh)


# ---- the kernel tests' synthetic cases ----------------------------------------------------------------------------------------
T = 2
HIDDEN, Y_DIM = 100, 2
DIM_Z = {16: 12, 64: 64}        # by head width: one z width that is no multiple of the 16-column tile, and the shipped one


@functools.lru_cache(maxsize=None)
def proj_matrix(d, m):
    if (d, m) == (64, 266):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor.npz"))["d64_big/proj"])
    with torch.random.fork_rng():
        torch.manual_seed(77 + m)
        return O.gaussian_orthogonal_random_matrix(m, d).float()


@functools.lru_cache(maxsize=None)
def params(d):
    """Query-side parameters at head width d = dim_w = dim_r (AttnLinear's N(0, 1 / in) weights; the decoder alike)."""
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
def case(kind, d, m, Nc, Nq):
    """(x [T, Nq, d], k [T, H, Nc, d], v [T, H, Nc, d], z [T, dim_z]) on the CPU: x such that the query heads are in the kind's
    regime, k / v as the head projections would leave them (the oracle's layout), z for the latent mode."""
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nc + len(kind))
    x = 0.25 * torch.randn(T, Nq, d, generator=g)
    k = 0.25 * torch.randn(T, HEADS, Nc, d, generator=g)
    v = torch.randn(T, HEADS, Nc, d, generator=g)
    z = torch.randn(T, DIM_Z[d], generator=g)
    if kind == "big":                      # large norm: most features sit on the 1e-4 floor
        x, k = 4 * x, 4 * k
    elif kind == "peak":                   # one key whose dd maximum sits ~50 above the rest
        k = 0.05 * torch.randn(T, HEADS, Nc, d, generator=g)
        pr = proj_matrix(d, m)[m // 2]
        k[1, 0, Nc - 1] = pr * (50.0 / (d ** -0.25 * float(pr @ pr)))
    elif kind == "equal":                  # all keys equal
        k = k[:1, :1, :1].expand(T, HEADS, Nc, d).contiguous()
    else:
        assert kind == "live"
    return x, k, v, z


def want(kind, d, m, Nc, Nq, attend, tanh):
    """The float64 result of a synthetic case, [T, Nq, Y_DIM]."""
    x, k, v, z = case(kind, d, m, Nc, Nq)
    if attend:
        state = {"kind": "attention", "fk": R.key_features(k, proj_matrix(d, m))[0], "vh": v.double()}
    else:
        state = {"kind": "latent", "z": z.double()}
    return query_tail(params(d), x, state, tanh, proj_matrix(d, m))
