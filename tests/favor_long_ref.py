"""Float64 restatement of the chunked per-shot stream (csrc/favor_long.h), step for step as the kernels walk it:
the key features 32 rows at a time with one partial maximum per chunk folded into the batch-global M, S per 32-column chunk, D as the
in-order sum of the columns, S V as one chain over the slots with the accumulator carried from chunk to chunk, and the masks BY
INDEX: a row behind lens[t] of k or v is never touched, so it may hold NaN.  In exact arithmetic this is
tests/favor_cached_ref.attention / tests/attention_readout_ref.weights (tests/ragged_ref's with lens); the CPU test holds the
restatement to them.  Layout [T, H, N, d] like oracle.ref_cpu."""
import torch

from tests import favor_cached_ref as R

CHUNK = 32


def _dd_diag(rows, proj):
    d = rows.shape[-1]
    c = d ** -0.25
    return (c * rows) @ proj.T, (rows * rows).sum(dim=-1, keepdim=True) * 0.5 * (c * c)


def key_features(k, proj, lens=None, eps=1e-4):
    """k [T, H, Nc, d] (rows behind lens[t] never read), proj [m, d] -> (F_k [T, H, Nc, m] float64, M).  K1: per (task, 32-row chunk)
    the dd of the valid rows and their maximum, -inf for a chunk without a shot; K2: M = the fold of all maxima, the features of
    the valid rows, zeros elsewhere."""
    T, H, Nc, d = k.shape
    m = proj.shape[0]
    lens = (Nc,) * T if lens is None else tuple(lens)
    proj = proj.double()
    ratio = m ** -0.5
    parts, kept = [], {}
    for t in range(T):
        for r0 in range(0, Nc, CHUNK):
            n = min(lens[t] - r0, CHUNK)
            if n <= 0:
                parts.append(torch.tensor(float("-inf"), dtype=torch.float64))
                continue
            dd, diag = _dd_diag(k[t, :, r0:r0 + n].double(), proj)
            assert bool(torch.isfinite(dd).all())
            kept[t, r0] = (dd, diag)
            parts.append(dd.max())
    M = torch.stack(parts).max()
    fk = torch.zeros(T, H, Nc, m, dtype=torch.float64)
    for (t, r0), (dd, diag) in kept.items():
        fk[t, :, r0:r0 + dd.shape[1]] = ratio * (torch.exp(dd - diag - M) + eps)
    return fk, M


def stream(q, k, v, proj, lens=None):
    """q [T, H, Nq, d], k, v [T, H, Nc, d], proj [m, d], lens [T] or None -> (out [T, H, Nq, d], w [T, H, Nq, Nc]) float64.  Per task
    the query walks need = lens[t] slots in chunks of 32; the columns of w from need on are zeros written by index."""
    T, H, Nc, d = k.shape
    Nq = q.shape[2]
    lens = (Nc,) * T if lens is None else tuple(lens)
    fk, _ = key_features(k, proj, lens)
    fq = R.query_features(q, proj)
    out = torch.zeros(T, H, Nq, d, dtype=torch.float64)
    w = torch.zeros(T, H, Nq, Nc, dtype=torch.float64)
    for t in range(T):
        need = lens[t]
        S = torch.full((H, Nq, Nc), float("nan"), dtype=torch.float64)          # columns >= need stay unwritten and unread
        for c0 in range(0, need, CHUNK):
            n = min(CHUNK, need - c0)
            S[:, :, c0:c0 + n] = fq[t] @ fk[t, :, c0:c0 + n].transpose(1, 2)
        D = torch.zeros(H, Nq, dtype=torch.float64)
        for n in range(need):
            D = D + S[:, :, n]
        acc = torch.zeros(H, Nq, d, dtype=torch.float64)
        for c0 in range(0, need, CHUNK):
            n = min(CHUNK, need - c0)
            acc = acc + S[:, :, c0:c0 + n] @ v[t, :, c0:c0 + n].double()
        out[t] = acc / D[..., None]
        w[t, :, :, :need] = S[:, :, :need] / D[..., None]
    return out, w
