"""The case tables of the sliding-window tests, shared by the CPU and the GPU files."""
import functools

import torch

from tests import favor_summary_ref as S

H = S.H
SHAPES = S.SHAPES                                   # (d, m) = (16, 16), (64, 266), (256, 1419)

# ---- mlhot_rows_compact ------------------------------------------------------------------------------------------------------------
ROW_TS = (1, 3)
ROW_SHAPES = ((1, 4), (32, 32), (33, 512), (257, 2048), (4096, 16))          # (cap, W)
ROW_SETS = (1, 2, 4)
PLANS = ("identity", "drop_first", "drop_last", "drop_255_256", "all_zero", "out_of_range")


def row_plan(kind, T, cap):
    """[T][cap] host ints: the source slot of every destination slot."""
    if kind == "identity":
        keep = list(range(cap))
    elif kind == "drop_first":
        keep = list(range(1, cap))
    elif kind == "drop_last":
        keep = list(range(cap - 1))
    elif kind == "drop_255_256":                    # the page edge of the paged form; smaller capacities drop their middle pair
        a = 255 if cap > 256 else max(cap // 2 - 1, 0)
        keep = [s for s in range(cap) if s not in (a, a + 1)]
    elif kind == "all_zero":
        keep = []
    else:                                           # values the kernel must hold to "a row of zeros"
        keep = [cap, -2, 2 ** 31 - 1, -2 ** 31][:cap]
    rows = [keep + [-1] * (cap - len(keep)) for _ in range(T)]
    if kind == "out_of_range" and cap > 4:
        rows = [r[:4] + [0] + r[5:] for r in rows]  # and one valid entry behind them
    return rows


# ---- evicted key states ------------------------------------------------------------------------------------------------------------
EVICT_T = 3
EVICT_FORMS = (("keys", 17), ("keys", 32), ("long", 33), ("long", 256), ("paged", 257), ("paged", 513))
PEAK = (0, 1)                                       # (task, slot) of the shot that holds M, 5 above the rest; it is dropped


def evict_lens(cap):
    return [cap, max(cap // 2, 4), 3]               # one task full, ..., one that is left with a single shot


def evict_drop(cap):
    lens = evict_lens(cap)
    edge = [s for s in (255, 256) if s < lens[0]]
    return [sorted({PEAK[1], lens[0] - 1, *edge}), [0, 2], [0, 2]]


@functools.lru_cache(maxsize=None)
def evict_inputs(d, m, cap):
    """k [T, H, cap, d] fp32 whose rows behind lens hold NaN, proj, lens, drop.  The PEAK shot's dd is at least 5 above every other."""
    g = torch.Generator().manual_seed(31 + d + m + cap)
    proj = S.proj_for(d, m)
    k = 0.25 * torch.randn(EVICT_T, H, cap, d, generator=g)
    c = d ** -0.25
    top = torch.einsum("thnd,md->thnm", c * k.double(), proj.double()).max().item()
    p = proj[0].double()
    k[PEAK[0], :, PEAK[1]] = ((top + 5.0) * p / (c * (p * p).sum())).float()
    lens = evict_lens(cap)
    for t, L in enumerate(lens):
        k[t, :, L:] = float("nan")
    return k, proj, lens, evict_drop(cap)


# ---- retract -----------------------------------------------------------------------------------------------------------------------
RETRACT_T = 3
# (absorbed shots N, retracted R, which): "first" / "last" - the first / last R of every task; "ragged" - per task (R, 0, R // 2 or 1)
RETRACTS = ((8, 1, "first"), (8, 4, "last"), (40, 4, "ragged"), (40, 1, "last"), (64, 33, "first"), (64, 33, "ragged"), (64, 4, "last"))
REGIMES = ("live", "equal")
NQ = 20


@functools.lru_cache(maxsize=None)
def retract_inputs(regime, d, m, N):
    """q [T, H, NQ, d], k, v [T, H, N, d], proj - fp32 on the CPU.  "live": random keys, every feature live; "equal": one key per
    (task, head).  The live keys are 0.1 randn: dd's spread is 0.1 d^(1/4) <= 0.4, so no single shot holds most of a feature's sum
    and taking out half of the shots leaves kappa <= 4 (tests/test_context_window_cpu.py asserts it for every case)."""
    g = torch.Generator().manual_seed(97 + d + m + N)
    q = 0.25 * torch.randn(RETRACT_T, H, NQ, d, generator=g)
    k = 0.1 * torch.randn(RETRACT_T, H, N, d, generator=g)
    if regime == "equal":
        k = k[:, :, :1].expand(-1, -1, N, -1).contiguous()
    return q, k, torch.randn(RETRACT_T, H, N, d, generator=g), S.proj_for(d, m)


def retract_split(N, R, which):
    """-> (old_lens per task, old index lists per task, remaining index lists per task)."""
    lens = [R, 0, max(R // 2, 1)] if which == "ragged" else [R] * RETRACT_T
    old = [list(range(N - L, N)) if which == "last" else list(range(L)) for L in lens]
    return lens, old, [[s for s in range(N) if s not in set(o)] for o in old]


def gathered(x, idx, n):
    """x [T, H, N, d], idx per task -> [T, H, n, d]: task t's rows idx[t] in front, zeros behind."""
    out = torch.zeros(x.shape[0], x.shape[1], n, x.shape[3], dtype=x.dtype)
    for t, i in enumerate(idx):
        out[t, :, :len(i)] = x[t, :, i]
    return out
