"""Float64 statement of the masked read-outs (csrc/favor_cached.h mlhot_favor_query_masked_fwd, csrc/favor_long.h
mlhot_favor_query_long_masked_fwd), in the notation of tests/favor_cached_ref.py: F_k with the state's batch-global
M over ALL valid shots, the masked ones included - the mask does not move the stabiliser -, S = F_q F_k^T, then per group g the kept
columns S o mask_g, D_g = rowsum(S o mask_g), w_g = (S o mask_g) / D_g, out_g = (S o mask_g) V / D_g.  A slot counts iff its mask bit
is set and it is a valid shot (n < lens[t]); a row that keeps none is zeros in w and out.  Layout [T, H, N, d] like oracle.ref_cpu;
mask bool [T, G, Nq, Nc]; w [T, G, H, Nq, Nc], out [T, G, H, Nq, d]."""
import torch

from tests import favor_cached_ref as R
from tests import ragged_ref as RR


def scores(q, k, proj, lens=None):
    """S [T, H, Nq, Nc] of q against the (ragged) key state: columns behind lens[t] are exact zeros."""
    lens = (k.shape[2],) * k.shape[0] if lens is None else lens
    return torch.einsum("thnm,thcm->thnc", R.query_features(q, proj), RR.key_features(k, proj, lens)[0])


def from_scores(S, v, mask, lens=None):
    """S [T, H, Nq, Nc] (float64), v [T, H, Nc, d], mask bool [T, G, Nq, Nc] -> (out [T, G, H, Nq, d], w [T, G, H, Nq, Nc])."""
    T, H, Nq, Nc = S.shape
    valid = RR.valid_mask((Nc,) * T if lens is None else lens, Nc)
    keep = (mask & valid[:, None, None, :])[:, :, None]                                  # [T, G, 1, Nq, Nc]
    Sm = torch.where(keep, S[:, None], torch.zeros((), dtype=torch.float64))             # selected, never subtracted
    D = Sm.sum(dim=-1, keepdim=True)
    w = torch.where(D > 0, Sm / torch.where(D > 0, D, torch.ones_like(D)), torch.zeros_like(Sm))
    vd = torch.where(valid[:, None, :, None], v.double(), torch.zeros((), dtype=torch.float64))
    return torch.einsum("tghnc,thce->tghne", w, vd), w


def masked(q, k, v, proj, mask, lens=None):
    """q [T, H, Nq, d], k, v [T, H, Nc, d], proj [m, d], mask bool [T, G, Nq, Nc], lens [T] or None -> (out, w) as from_scores."""
    return from_scores(scores(q, k, proj, lens), v, mask, lens)


def merged(out):
    """[T, G, H, N, d] -> the kernels' [T, G, N, d*H]: out[t, g, n, e*H + h]."""
    T, G, H, N, d = out.shape
    return out.permute(0, 1, 3, 4, 2).reshape(T, G, N, d * H)
