"""Float64 statement of the attention read-out (csrc/favor_cached.h, mlhot_favor_query_weights_fwd): FAVOR+'s implied
attention w[t, h, q, n] = S[q, n] / D[q], with S = F_q F_k^T and D = rowsum(S) exactly the S and D of tests/favor_cached_ref.py's
query (out = S V / D), so sum_n w = 1, w >= 0 and out = sum_n w v.  It is FAVOR+'s own weighting - the 1e-4 floors and the
batch-global key stabiliser included - not a softmax.  The masked form takes tests/ragged_ref.py's key features: a zero row of F_k is
an exactly zero column of S and of w.  Layout [T, H, N, d] like oracle.ref_cpu; w [T, H, Nq, Nc]."""
import torch

from tests import favor_cached_ref as R
from tests import ragged_ref as RR


def weights_from_features(q, fk, proj):
    """q [T, H, Nq, d], F_k [T, H, Nc, m] (float64), proj [m, d] -> w [T, H, Nq, Nc]; row-wise in q."""
    S = torch.einsum("thnm,thcm->thnc", R.query_features(q, proj), fk)
    return S / S.sum(dim=-1, keepdim=True)


def weights(q, k, proj, lens=None):
    """w of q against the keys k [T, H, Nc, d]; `lens` [T]: the masked state - slot n of task t is a context shot iff n < lens[t], the
    stabiliser is the maximum over the valid rows, what an invalid row of k holds goes nowhere and its column of w is exactly 0."""
    fk = R.key_features(k, proj)[0] if lens is None else RR.key_features(k, proj, lens)[0]
    return weights_from_features(q, fk, proj)


def apply(w, v):
    """sum_n w[t, h, q, n] v[t, h, n, e] -> [T, H, Nq, d]: what favor_cached_ref.attention returns, through w."""
    return torch.einsum("thnc,thce->thne", w.double(), v.double())
