"""The inputs of the shared-target query tests (tests/test_shared_query_cpu.py, tests/test_shared_query_gpu.py), one
recipe for both: ONE set of query rows q [H, NQ, d] asked of T stored contexts k, v [T, H, Nc, d].  The shapes are the smallest at
which the kernels of csrc/favor_shared.h can go wrong: one task, two and five (a task group that is no divisor of T), query rows
either side of the 16-row tile, context slots either side of the 32-slot chunk and at the entries' limits, a task with a single shot.

The float64 reference is the per-task reference - tests/attention_readout_ref.py, tests/favor_cached_ref.py and tests/ragged_ref.py for
the "cached" form, tests/favor_long_ref.py for the "long" one - applied to the BROADCAST query: q.expand(T, ...), a view, no copy.
It is computed once per case and shared.  Layout [T, H, N, d] on the CPU, like oracle.ref_cpu."""
import functools

import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import favor_cached_ref as R
from tests import favor_long_ref as FL
from tests import ragged_ref as RR

H = AC.H
NQ = 33                          # rows generated per case: two full tiles and a tile of one row
NQS = [1, 15, 16, 17, 33]        # a smaller Nq takes the first rows
DM = [(16, 16), (64, 266)]
DM_BIG = (256, 1419)             # the shipped ResNet shape: the largest F_q tile
TASK_GROUPS = (1, 2, "T", 0)     # "T": all tasks in one group; 0: the library's choice

# (form, T, Nc, lens): lens None = every task full
SHAPES = [
    ("cached", 1, 1, None),
    ("cached", 2, 31, None),
    ("cached", 2, 32, (1, 32)),
    ("cached", 5, 32, None),
    ("cached", 5, 31, (1, 31, 16, 17, 5)),
    ("long", 1, 33, None),
    ("long", 2, 64, (1, 64)),
    ("long", 5, 65, (33, 65, 1, 32, 64)),
    ("long", 2, 256, (255, 33)),
    ("long", 5, 33, None),
]
# (form, T, Nc, d, m, lens, Nq rows the GPU test runs)
CASES = [(form, T, Nc, d, m, lens, NQ) for d, m in DM for form, T, Nc, lens in SHAPES] + [("cached", 2, 15, *DM_BIG, None, 17)]
POISON_CASES = [("cached", 5, 31, 64, 266, (1, 31, 16, 17, 5)), ("long", 5, 65, 64, 266, (33, 65, 1, 32, 64))]
POISON = {"cached": 3.0, "long": 1e30}     # finite and not 0: the cached entry multiplies it by an exactly zero column, the long one never reads it


def case_id(c):
    form, T, Nc, d, m, lens = c[:6]
    return f"{form}-T{T}-Nc{Nc}-d{d}m{m}" + ("" if lens is None else "-ragged")


@functools.lru_cache(maxsize=None)
def inputs(form, T, Nc, d, m):
    """(q [H, NQ, d] shared by the tasks, k, v [T, H, Nc, d], proj [m, d])"""
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nc + 101 * T + len(form))
    q = 0.25 * torch.randn(H, NQ, d, generator=g)
    k = 0.25 * torch.randn(T, H, Nc, d, generator=g)
    v = torch.randn(T, H, Nc, d, generator=g)
    return q, k, v, AC.proj(d, m)


def broadcast(q, T):
    """The shared rows as every task's: [T, H, Nq, d], a view of the one copy"""
    return q[None].expand(T, *q.shape)


def operands(form, T, Nc, d, m, lens, poison=None):
    """(q, k, v, proj) as the kernels get them: k NaN behind lens[t]; v behind lens[t] zeros ("cached": the entry reads them against an
    exactly zero column), NaN ("long": never read), or `poison` for either"""
    q, k, v, p = inputs(form, T, Nc, d, m)
    if lens is None:
        return q, k, v, p
    valid = RR.valid_mask(lens, Nc)[:, None, :, None]
    fill = poison if poison is not None else 0.0 if form == "cached" else float("nan")
    return q, torch.where(valid, k, torch.full((), float("nan"))), torch.where(valid, v, torch.full((), fill)), p


def reference_for(qt, k, v, p, form, lens):
    """(w64 [T, H, Nq, Nc], out64 [T, H, Nq, d]) of per-task query rows qt [T, H, Nq, d]: the per-task references, as they are"""
    if form == "long":
        out, w = FL.stream(qt, k, v, p, lens)
        return w, out
    if lens is None:
        return AR.weights(qt, k, p), R.attention(qt, k, v, p)
    return AR.weights(qt, k, p, lens), RR.attention(qt, k, v, p, lens)


@functools.lru_cache(maxsize=None)
def want(form, T, Nc, d, m, lens):
    """(w64, out64) of the case: the per-task reference on the broadcast query"""
    q, k, v, p = inputs(form, T, Nc, d, m)
    return reference_for(broadcast(q, T), k, v, p, form, lens)
