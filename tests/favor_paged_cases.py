"""The inputs of the paged per-shot state's tests (tests/test_favor_paged_cpu.py, tests/test_favor_paged_gpu.py), one
recipe for both: tests/attention_readout_cases.py's value kinds at the slot counts either side of every 256-slot page edge (257: a
page and one slot; 288: a page and one full chunk; 511, 512, 513: the second page a slot short, full, and a third page of one slot;
600: a third page of two chunks and a partial one).  The float64 references are tests/favor_long_ref.py's stream - general in Nc -
and tests/context_mask_ref.py, computed once per case and shared."""
import functools

import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import context_mask_ref as CM
from tests import ragged_ref as RR

T, H = AC.T, AC.H
DM = [(16, 16), (64, 266)]
DM_BIG = (256, 1419)           # one case at the shipped ResNet shape
NC_BIG, NQ_BIG = 257, 17
NCS = [257, 288, 511, 512, 513, 600]
NQS = [1, 16, 17, 37]
NQ = 37                        # query rows per case: the first 37 of AC.inputs' 100
KINDS = AC.KINDS
TIE_NCS = [1, 32, 33, 255, 256]          # one page: the long entries' bits
RAGGED_NCS = [513, 600]
MASK_NCS = [300, 513]
PAGE = 256


def inputs(kind, d, m, Nc):
    """(q [T, H, NQ, d], k, v [T, H, Nc, d], proj [m, d])"""
    q, k, v, p = AC.inputs(kind, d, m, Nc)
    return q[:, :, :NQ].contiguous(), k, v, p


def cases():
    """every (kind, d, m, Nc) the GPU value test runs"""
    return [(kind, d, m, Nc) for d, m in DM for Nc in NCS for kind in KINDS] + [(kind, *DM_BIG, NC_BIG) for kind in KINDS]


@functools.lru_cache(maxsize=None)
def want(kind, d, m, Nc):
    """(w64 [T, H, NQ, Nc], out64 [T, H, NQ, d])"""
    w, out = AC.want(kind, d, m, Nc)
    return w[:, :, :NQ], out[:, :, :NQ]


def ragged_lens(Nc):
    """1, 256, 257 and full, two tasks at a time: a task of one shot beside a full one, the two sides of the first page edge"""
    return [(1, Nc), (256, 257), (Nc, 257)]


@functools.lru_cache(maxsize=None)
def ragged(kind, d, m, Nc, lens):
    """(q, k with NaN behind lens[t], v with +-1e30 there, proj, w64 [T, H, NQ, Nc], out64, F_k64 [T, H, Nc, m], M64)"""
    q, k, v, p = inputs(kind, d, m, Nc)
    valid = RR.valid_mask(lens, Nc)[:, None, :, None]
    kn = torch.where(valid, k, torch.full((), float("nan")))
    sign = torch.where(torch.arange(Nc) % 2 == 0, 1.0, -1.0)[None, None, :, None]
    vp = torch.where(valid, v, 1e30 * sign.expand_as(v))
    fk, M = RR.key_features(k, p, lens)
    return q, kn, vp, p, AR.weights(q, k, p, lens), RR.attention(q, k, v, p, lens), fk, M


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def mask_lens(Nc):
    """task 0 full, task 1 ends inside the second page"""
    return (Nc, 270)


def mask(pattern, Nc, lens, Nq=NQ):
    """bool [T, 3, Nq, Nc] (G = 3).  random: group 0 keeps slot 0 besides, the others may leave a row empty; page: group 0 drops the
    whole first page, group 1 the whole second one, group 2 keeps every second slot; tail: group 0 keeps only the slots of the task's
    LAST, partial page, group 1 only its last valid slot, group 2 only slot 255 and 256 (either side of the page edge)."""
    c = torch.arange(Nc)[None, None, :]
    L = torch.tensor(lens)[:, None, None]
    if pattern == "random":
        r = torch.rand(T, 3, Nq, Nc, generator=torch.Generator().manual_seed(5 + Nc)) < 0.5
        r[:, 0, :, 0] = True
        return r
    if pattern == "page":
        groups = [c >= PAGE, (c < PAGE) | (c >= 2 * PAGE), c % 2 == 0]
    else:
        assert pattern == "tail"
        groups = [c >= (L - 1) // PAGE * PAGE, c == L - 1, (c == PAGE - 1) | (c == PAGE)]
    return torch.stack([g.expand(T, Nq, Nc) for g in groups], dim=1).contiguous()


MASK_PATTERNS = ["random", "page", "tail"]


@functools.lru_cache(maxsize=None)
def mask_inputs(Nc, d, m):
    """(q [T, H, NQ, d], k, v [T, H, Nc, d], proj [m, d]) in the live regime"""
    g = torch.Generator().manual_seed(31 * d + m + 7 * Nc)
    return (0.25 * torch.randn(T, H, NQ, d, generator=g), 0.25 * torch.randn(T, H, Nc, d, generator=g), torch.randn(T, H, Nc, d, generator=g),
            AC.proj(d, m))


@functools.lru_cache(maxsize=None)
def mask_scores(Nc, d, m):
    q, k, _, p = mask_inputs(Nc, d, m)
    return CM.scores(q, k, p, mask_lens(Nc))


def mask_want(Nc, d, m, pattern):
    """(mask, out64 [T, 3, H, NQ, d], w64 [T, 3, H, NQ, Nc])"""
    mk = mask(pattern, Nc, mask_lens(Nc))
    return (mk, *CM.from_scores(mask_scores(Nc, d, m), mask_inputs(Nc, d, m)[2], mk, mask_lens(Nc)))


DOMINANT = dict(Nc=300, d=64, m=16, slot=270, drop=(270, 5, 299))


@functools.lru_cache(maxsize=None)
def dominant():
    """tests/context_mask_cases.dominant's recipe at 300 shots with the dominant one on the second page: the short key scaled
    towards the queries holds nearly all the weight, the other 299 are long keys in the null space of the projection whose features
    are the 1e-4 floor.  Groups: leave out the dominant slot, a slot of the first page, the last slot.
    -> (q, k, v, proj, mask [T, 3, NQ, Nc], out64, w64, w64 of the unmasked call)"""
    Nc, d, m, slot, drop = (DOMINANT[x] for x in ("Nc", "d", "m", "slot", "drop"))
    g = torch.Generator().manual_seed(99)
    p = AC.proj(d, m)
    q = 0.25 * torch.randn(T, H, NQ, d, generator=g)
    r = torch.randn(T, H, Nc, d, generator=g).double()
    pd = p.double()
    r = r - (r @ pd.T) @ torch.linalg.solve(pd @ pd.T, pd)                              # the part of r the projection does not see
    k = (r * ((2 * 20.0) ** 0.5 / (d ** -0.25 * r.norm(dim=-1, keepdim=True)))).float()
    k[:, :, slot] = 0.25 * q[:, :, 0]
    v = torch.randn(T, H, Nc, d, generator=g)
    mk = torch.stack([(torch.arange(Nc) != s)[None, None, :].expand(T, NQ, Nc) for s in drop], dim=1).contiguous()
    out, w = CM.masked(q, k, v, p, mk)
    full = CM.masked(q, k, v, p, torch.ones(T, 1, NQ, Nc, dtype=torch.bool))[1][:, 0]
    return q, k, v, p, mk, out, w, full
