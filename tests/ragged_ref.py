"""Float64 restatement of the masked key state (csrc/favor_cached.h, mlhot_favor_keys_ragged_fwd): row n of task t
is a context shot iff n < lens[t].  The key stabiliser is the maximum of dd over the valid rows of all tasks, valid rows get
tests/favor_cached_ref.py's features with that maximum, invalid rows are zeros - selected by index, so what an invalid row of k holds
(NaN, Inf) goes nowhere.  The reference project cannot express a ragged batch; this restatement is the oracle.  Layout [T, H, N, d]."""
import torch

from tests import favor_cached_ref as R


def valid_mask(lens, Nc):
    """[T, Nc] bool: slot n of task t holds a context shot."""
    return torch.arange(Nc)[None, :] < torch.as_tensor(list(lens))[:, None]


def key_features(k, proj, lens, eps=1e-4):
    """k [T, H, Nc, d], proj [m, d], lens [T] -> (F_k [T, H, Nc, m] with zero rows behind lens[t], M over the valid rows)."""
    T, H, Nc, d = k.shape
    m = proj.shape[0]
    valid = valid_mask(lens, Nc)
    assert bool(valid.any(dim=1).all()), "every task holds at least one context shot"
    kd = torch.where(valid[:, None, :, None], k.double(), torch.zeros((), dtype=torch.float64))       # nothing of an invalid row is read
    c, ratio = d ** -0.25, m ** -0.5
    dd = torch.einsum("thnd,md->thnm", c * kd, proj.double())
    diag = (kd * kd).sum(dim=-1, keepdim=True) * 0.5 * (c * c)
    M = dd[valid[:, None, :].expand(T, H, Nc)].max()
    fk = ratio * (torch.exp(dd - diag - M) + eps)
    return torch.where(valid[:, None, :, None], fk, torch.zeros((), dtype=torch.float64)), M


def attention(q, k, v, proj, lens):
    """FAVOR+ of q [T, H, Nq, d] against the ragged context: every task attends to its own first lens[t] shots, with the one
    stabiliser of the ragged batch (R.query on the zero rows: their column of S is 0, they add nothing to D or to out)."""
    fk, _ = key_features(k, proj, lens)
    vd = torch.where(valid_mask(lens, k.shape[2])[:, None, :, None], v.double(), torch.zeros((), dtype=torch.float64))
    return R.query(q, fk, vd, proj)


def attention_sliced(q, k, v, proj, lens):
    """The same from the sliced keys: per task R.query against F_k of its own lens[t] rows alone (no zero row anywhere), the
    stabiliser still the ragged batch's.  Equal to attention() in exact arithmetic; the tests compare the kernels against this one."""
    fk, _ = key_features(k, proj, lens)
    out = [R.query(q[t:t + 1], fk[t:t + 1, :, :L], v[t:t + 1, :, :L], proj) for t, L in enumerate(lens)]
    return torch.cat(out, dim=0)
