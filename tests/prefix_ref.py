"""What the prefix sweep has to compute, stated with the existing oracle (checker only).

`forward_prefixes_ref` IS the definition: oracle.ref_cpu.resnet_np_forward once per context size k on ctx[:, :k].  Beside it a
numpy (float64) statement of the two operators that see k - the shot-axis aggregators as running sums / maxima and FAVOR+ with its
batch-global key stabiliser per prefix, M_k = max over all tasks, heads, features and the FIRST k shots - which
tests/test_prefix_sweep_cpu.py checks against oracle.ref_cpu's aggregators and FAVOR+ on sliced inputs for every k."""
import numpy as np
import torch

from oracle import ref_cpu as O


def forward_prefixes_ref(p, ctx_x, ctx_y, qry_x, agg_mode, img_agg, ks=None):
    """-> mu [K, T, Nq, out]: one plain oracle forward per context size."""
    ks = range(1, ctx_x.shape[1] + 1) if ks is None else ks
    with torch.no_grad():
        return torch.stack([O.resnet_np_forward(p, ctx_x[:, :k], ctx_y[:, :k], qry_x, agg_mode, img_agg) for k in ks])


def _softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def agg_prefixes_np(mode, rs, lv=None):
    """rs [T, Nc, R] (baco: rs = mu, lv = the pre-softplus variance logits) -> [Nc, T, R]; row k-1 aggregates rs[:, :k]."""
    rs = np.asarray(rs, dtype=np.float64)
    Nc = rs.shape[1]
    if mode == "mean":
        out = np.cumsum(rs, axis=1) / np.arange(1, Nc + 1)[None, :, None]
    elif mode == "max":
        out = np.maximum.accumulate(rs, axis=1)
    elif mode == "baco":
        iv = 1.0 / (1e-5 + _softplus(np.asarray(lv, dtype=np.float64)))
        out = np.cumsum(iv * rs, axis=1) / (1.0 + np.cumsum(iv, axis=1))          # prior N(0, 1)
    else:
        raise ValueError(mode)
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def favor_stabilisers_np(k, proj):
    """M_1..M_Nc of keys k [T, H, Nc, d]: the running maximum over the shots of max(dd) over tasks, heads and features."""
    k, proj = np.asarray(k, dtype=np.float64), np.asarray(proj, dtype=np.float64)
    dd = np.einsum("thnd,md->thnm", k.shape[-1] ** -0.25 * k, proj)
    return np.maximum.accumulate(dd.max(axis=(0, 1, 3)))


def favor_prefixes_np(q, k, v, proj, eps=1e-4):
    """q [T, H, Nq, d], k / v [T, H, Nc, d], proj [m, d] -> [Nc, T, H, Nq, d]: FAVOR+ (fast_attention.py:74-99, 151-156) on the first
    kk keys / values for kk = 1..Nc.  The projections are taken once; only the key stabiliser M_kk and the sums see kk."""
    q, k, v, proj = (np.asarray(t, dtype=np.float64) for t in (q, k, v, proj))
    d, m = q.shape[-1], proj.shape[0]
    c, ratio = d ** -0.25, m ** -0.5
    ddq = np.einsum("thnd,md->thnm", c * q, proj)
    ddk = np.einsum("thnd,md->thnm", c * k, proj)
    diag_q = (q * q).sum(-1, keepdims=True) * 0.5 * c * c
    diag_k = (k * k).sum(-1, keepdims=True) * 0.5 * c * c
    qp = ratio * (np.exp(ddq - diag_q - ddq.max(-1, keepdims=True)) + eps)
    M = np.maximum.accumulate(ddk.max(axis=(0, 1, 3)))
    out = []
    for kk in range(1, k.shape[2] + 1):
        kp = ratio * (np.exp(ddk[:, :, :kk] - diag_k[:, :, :kk] - M[kk - 1]) + eps)
        S = np.einsum("thnm,thjm->thnj", qp, kp)
        out.append(np.einsum("thnj,thje->thne", S, v[:, :, :kk]) / S.sum(-1, keepdims=True))
    return np.stack(out)

