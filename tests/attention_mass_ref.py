"""The attention mass (csrc/favor_mass.h) stated twice: from its definition in float64,
    mass[t, h, c] = sum_n tw[t, n] w[t, h, n, c],   w = tests/attention_readout_ref.weights,
and `fold32`, the kernels' documented fp32 order in numpy - per 16-row tile the rows in ascending order from +0.0, then the tiles in
ascending order from +0.0, every add one rounded float32 add and, with tw, every term one rounded float32 multiply before it (numpy
has no FMA to contract into).  `prune_by_hand` is prune's slot choice written the slow way."""
import numpy as np
import torch

from tests import attention_readout_ref as AR

TILE = 16


def mass64(q, k, proj, lens=None, tw=None):
    """q [T, H, Nq, d], k [T, H, Nc, d], proj [m, d], lens, tw [T, Nq] -> mass [T, H, Nc] in float64 from the definition"""
    w = AR.weights(q, k, proj, lens)                                        # float64 [T, H, Nq, Nc]
    if tw is not None:
        w = w * tw.double()[:, None, :, None]
    return w.sum(dim=2)


def mass64_of(w, tw=None):
    """The same from a given w [T, H, Nq, Nc] (any float dtype): the exact column sums of THESE weights, in float64."""
    w = torch.as_tensor(w).double()
    if tw is not None:
        w = w * torch.as_tensor(tw).double()[:, None, :, None]
    return w.sum(dim=2)


def tile_partials32(w, tw=None):
    """w [T, H, Nq, Nc] float32, tw [T, Nq] float32 or None -> part [T, H, ceil(Nq / 16), Nc] float32: sequential float32 adds over
    the rows of each tile, a separate float32 multiply with tw"""
    w = np.ascontiguousarray(torch.as_tensor(w).cpu().numpy(), dtype=np.float32)
    T, H, Nq, Nc = w.shape
    twn = None if tw is None else np.ascontiguousarray(torch.as_tensor(tw).cpu().numpy(), dtype=np.float32)
    ntile = (Nq + TILE - 1) // TILE
    part = np.zeros((T, H, ntile, Nc), dtype=np.float32)
    for n in range(Nq):
        term = w[:, :, n, :] if twn is None else (twn[:, None, n, None] * w[:, :, n, :]).astype(np.float32)
        part[:, :, n // TILE, :] = (part[:, :, n // TILE, :] + term).astype(np.float32)
    return part


def fold_tiles32(part):
    """part [T, H, tiles, Nc] float32 -> [T, H, Nc]: the tiles added in ascending order from +0.0"""
    part = np.asarray(part, dtype=np.float32)
    acc = np.zeros(part.shape[:2] + part.shape[3:], dtype=np.float32)
    for i in range(part.shape[2]):
        acc = (acc + part[:, :, i, :]).astype(np.float32)
    return acc


def fold32(w, tw=None):
    """The documented order -> mass [T, H, Nc] as a float32 torch tensor"""
    return torch.from_numpy(fold_tiles32(tile_partials32(w, tw)))


def prune_by_hand(score, lens, keep):
    """drop lists: per task, repeatedly take away the valid slot with the smallest score - of equal scores the HIGHEST index, so ties
    keep the lower one - until keep[t] are left"""
    drop = []
    for t, n in enumerate(lens):
        alive = list(range(n))
        gone = []
        while len(alive) > keep[t]:
            worst = min(alive, key=lambda c: (float(score[t][c]), -c))
            alive.remove(worst)
            gone.append(worst)
        drop.append(sorted(gone))
    return drop
