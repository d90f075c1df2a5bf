"""The cases of the per-target context mask tests (tests/test_context_mask_cpu.py, tests/test_context_mask_gpu.py),
one table for both.  Shapes: the cached kernel at Nc 1, 31, 32 and the long kernel at Nc 33, 64, 65, 256 with ragged lens, d 16 / 64 /
256, m 16 / 266, T 2, H 2; NQ = 17 target rows are generated per case (a full 16-row tile and a tile of one row), a smaller Nq takes
the first rows.  Patterns: see `mask`.  Layout [T, H, N, d] on the CPU like oracle.ref_cpu; float64 references once per case."""
import functools

import torch

from tests import attention_readout_cases as AC
from tests import context_mask_ref as CM

T, H, NQ = 2, 2, 17
NQS = [1, 16, 17]
# (route, Nc, lens or None, d, m)
SHAPES = [
    ("cached", 1, None, 16, 16),
    ("cached", 31, None, 64, 266),
    ("cached", 32, None, 256, 266),
    ("cached", 32, (5, 32), 16, 16),
    ("long", 33, (33, 20), 16, 16),
    ("long", 64, (64, 33), 64, 266),
    ("long", 65, (65, 1), 256, 16),
    ("long", 256, (256, 100), 16, 266),
]
PATTERNS = ["ones", "single", "loo", "causal", "random", "bit31", "bit32", "last_valid"]


def lens_of(shape):
    return shape[2] if shape[2] is not None else (shape[1],) * T


def mask(pattern, Nc, lens, Nq=NQ):
    """bool [T, G, Nq, Nc].  ones: G 2, everything; single: G 2, group g of target n keeps the one slot (n + g) % lens[t]; loo: G Nc,
    group c drops slot c; causal: G 1, target n sees the first n % lens[t] + 1 shots; random: G 2, group 0 keeps slot 0 besides,
    group 1 may leave a row empty; bit31 / bit32: G 1, only slot 31 / 32 (the last bit of word 0, the first of word 1) - a row whose
    task has no such shot keeps nothing; last_valid: G 1, only slot lens[t] - 1."""
    n, c = torch.arange(Nq)[None, :, None], torch.arange(Nc)[None, None, :]
    L = torch.tensor(lens)[:, None, None]
    if pattern == "ones":
        return torch.ones(T, 2, Nq, Nc, dtype=torch.bool)
    if pattern == "single":
        return torch.stack([c == (n + g) % L for g in range(2)], dim=1)
    if pattern == "loo":
        return (~torch.eye(Nc, dtype=torch.bool))[None, :, None, :].expand(T, Nc, Nq, Nc).contiguous()
    if pattern == "causal":
        return (c <= n % L)[:, None]
    if pattern == "random":
        r = torch.rand(T, 2, Nq, Nc, generator=torch.Generator().manual_seed(5 + Nc)) < 0.5
        r[:, 0, :, 0] = True
        return r
    if pattern in ("bit31", "bit32"):
        return (c == int(pattern[3:])).expand(T, Nq, Nc)[:, None].contiguous()
    assert pattern == "last_valid"
    return (c == L - 1).expand(T, Nq, Nc)[:, None].contiguous()


def patterns(Nc):
    return [p for p in PATTERNS if not (p == "bit31" and Nc < 32) and not (p == "bit32" and Nc < 33)]


@functools.lru_cache(maxsize=None)
def inputs(Nc, d, m):
    """(q [T, H, NQ, d], k, v [T, H, Nc, d], proj [m, d]) in the live regime of tests/attention_readout_cases.py"""
    g = torch.Generator().manual_seed(31 * d + m + 7 * Nc)
    return (0.25 * torch.randn(T, H, NQ, d, generator=g), 0.25 * torch.randn(T, H, Nc, d, generator=g), torch.randn(T, H, Nc, d, generator=g),
            AC.proj(d, m))


@functools.lru_cache(maxsize=None)
def scores(Nc, lens, d, m):
    q, k, _, p = inputs(Nc, d, m)
    return CM.scores(q, k, p, lens)


def want(shape, pattern):
    """(mask, out64 [T, G, H, NQ, d], w64 [T, G, H, NQ, Nc]) of a shape and a pattern; S is computed once per shape."""
    _, Nc, lens, d, m = shape
    mk = mask(pattern, Nc, lens_of(shape))
    return (mk, *CM.from_scores(scores(Nc, lens, d, m), inputs(Nc, d, m)[2], mk, lens))


DOMINANT = dict(Nc=4, d=64, m=16, slot=1)


@functools.lru_cache(maxsize=None)
def dominant():
    """One shot that holds more than 0.999 of every target's weight.  FAVOR+ subtracts 0.5 c^2 |k|^2 and the batch maximum from every
    key's exponent, so a key cannot dominate by being long: a long key's features fall to the 1e-4 floor.  The dominant key is
    therefore the SHORT one, scaled towards the (short) queries, and the other three are long - |k| with 0.5 c^2 |k|^2 = 20 - and
    lie in the null space of the 16 x 64 projection, so they do not move the stabiliser: their features are the floor, 1e-4 of
    the dominant key's.  Leave-one-out over it: the group that drops the dominant shot is what "full sum minus the masked part"
    would lose to cancellation.  -> (q, k, v, proj, mask [T, Nc, NQ, Nc], out64, w64, w64 of the unmasked call)"""
    Nc, d, m, slot = (DOMINANT[x] for x in ("Nc", "d", "m", "slot"))
    g = torch.Generator().manual_seed(99)
    p = AC.proj(d, m)
    q = 0.25 * torch.randn(T, H, NQ, d, generator=g)
    r = torch.randn(T, H, Nc, d, generator=g).double()
    pd = p.double()
    r = r - (r @ pd.T) @ torch.linalg.solve(pd @ pd.T, pd)                              # the part of r the projection does not see
    k = (r * ((2 * 20.0) ** 0.5 / (d ** -0.25 * r.norm(dim=-1, keepdim=True)))).float()
    k[:, :, slot] = 0.25 * q[:, :, 0]
    v = torch.randn(T, H, Nc, d, generator=g)
    mk = mask("loo", Nc, (Nc,) * T)
    out, w = CM.masked(q, k, v, p, mk)
    full = CM.masked(q, k, v, p, torch.ones(T, 1, NQ, Nc, dtype=torch.bool))[1][:, 0]
    return q, k, v, p, mk, out, w, full
