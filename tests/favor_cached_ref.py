"""Float64 restatement of FAVOR+ split at the context (csrc/favor_cached.h): the key features with the batch-global maximum, the
query features with their row maximum, S = F_q F_k^T, D = rowsum(S), out = S V / D.  Layout [T, H, N, d] like oracle.ref_cpu."""
import torch


def key_features(k, proj, eps=1e-4):
    """k [T, H, Nc, d], proj [m, d] -> (F_k [T, H, Nc, m], M): F_k = ratio (exp(dd - diag - M) + eps), M = max of dd over everything."""
    k, proj = k.double(), proj.double()
    d, m = k.shape[-1], proj.shape[0]
    c, ratio = d ** -0.25, m ** -0.5
    dd = torch.einsum("thnd,md->thnm", c * k, proj)
    diag = (k * k).sum(dim=-1, keepdim=True) * 0.5 * (c * c)
    M = dd.max()
    return ratio * (torch.exp(dd - diag - M) + eps), M


def query_features(q, proj, eps=1e-4):
    q, proj = q.double(), proj.double()
    d, m = q.shape[-1], proj.shape[0]
    c, ratio = d ** -0.25, m ** -0.5
    dd = torch.einsum("thnd,md->thnm", c * q, proj)
    diag = (q * q).sum(dim=-1, keepdim=True) * 0.5 * (c * c)
    return ratio * (torch.exp(dd - diag - dd.max(dim=-1, keepdim=True).values) + eps)


def query(q, fk, v, proj):
    """q [T, H, Nq, d], F_k from key_features, v [T, H, Nc, d] -> out [T, H, Nq, d]; row-wise in q."""
    S = torch.einsum("thnm,thcm->thnc", query_features(q, proj), fk)
    return torch.einsum("thnc,thce->thne", S, v.double()) / S.sum(dim=-1, keepdim=True)


def attention(q, k, v, proj):
    return query(q, key_features(k, proj)[0], v, proj)


def merged(out):
    """[T, H, N, d] -> the kernels' merged order [T, N, d*H]: out[t, n, e*H + h]."""
    T, H, N, d = out.shape
    return out.permute(0, 2, 3, 1).reshape(T, N, d * H)
