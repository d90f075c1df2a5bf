"""The top-k attention read-out (csrc/favor_topk.h) stated in torch: per (task, head, target row) the valid slots
ranked by a score, descending, ties to the lower slot index; entries behind the number of valid slots are idx = -1, value +0.
`topk_of` is that statement over any score tensor; `topk64` applies it to the float64 read-out tests/attention_readout_ref.weights.
The kernels rank the un-normalised S and divide k numbers; `topk_of` over w = S / D gives the same VALUES (division by the row's
D > 0 is monotone) and, where two different S round to one w, possibly other indices."""
import torch

from tests import attention_readout_ref as AR


def valid_counts(lens, T, Nc):
    return [Nc] * T if lens is None else [int(n) for n in lens]


def topk_of(score, lens, k):
    """score [T, H, Nq, Nc] (any float dtype), lens [T] or None, k -> (idx int64 [T, H, Nq, k], val [T, H, Nq, k] in score's dtype).
    A stable descending sort over the task's valid slots: equal scores keep their slot order."""
    T, H, Nq, Nc = score.shape
    idx = torch.full((T, H, Nq, k), -1, dtype=torch.int64)
    val = torch.zeros(T, H, Nq, k, dtype=score.dtype)
    for t, n in enumerate(valid_counts(lens, T, Nc)):
        order = torch.sort(score[t, :, :, :n], dim=-1, descending=True, stable=True)
        j = min(k, n)
        idx[t, :, :, :j] = order.indices[..., :j]
        val[t, :, :, :j] = order.values[..., :j]
    return idx, val


def gather_at(w, idx):
    """w [T, H, Nq, Nc], idx [T, H, Nq, k] with -1 padding -> w at idx, 0 where idx is -1"""
    got = torch.gather(w, -1, idx.long().clamp_min(0))
    return torch.where(idx >= 0, got, torch.zeros((), dtype=w.dtype))


def topk64(q, k, proj, lens, kk):
    """q [T, H, Nq, d], k [T, H, Nc, d], proj [m, d] -> (w64 [T, H, Nq, Nc], idx, val) of the float64 read-out"""
    w = AR.weights(q, k, proj, lens)
    return (w,) + topk_of(w, lens, kk)


def check_shape_rules(idx, wk, lens, Nc, k):
    """What holds for every result whatever the scores: dtypes, the padding exact, indices valid and distinct, values descending."""
    T, H, Nq, kk = idx.shape
    assert kk == k and wk.shape == idx.shape and idx.dtype == torch.int32 and wk.dtype == torch.float32
    idx, wk = idx.cpu(), wk.cpu()
    for t, n in enumerate(valid_counts(lens, T, Nc)):
        j = min(k, n)
        head, pad_i, pad_w = idx[t, :, :, :j], idx[t, :, :, j:], wk[t, :, :, j:]
        assert bool((pad_i == -1).all()) and bool((pad_w == 0.0).all()) and not bool(torch.signbit(pad_w).any()), (t, n)
        assert bool((head >= 0).all()) and bool((head < n).all()), (t, n)
        assert bool((torch.sort(head, dim=-1).values.diff(dim=-1) > 0).all()), (t, "indices repeat")
        assert bool((wk[t, :, :, :j].diff(dim=-1) <= 0).all()) and bool((wk[t, :, :, :j] > 0).all()), (t, "not descending")
