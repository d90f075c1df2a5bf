"""Shared by tests/test_mt_stream_cpu.py and tests/test_mt_stream_gpu.py: the case table that walks the branches of the device
continuation of torch's CPU normal_() stream (csrc/mt_normal.h: mt_fill_kernel, mt_window / mt_jump / mt_chunk_kernel,
mt_box_muller_kernel; mlhot/rng.py) and the reference every case is judged by - torch's own CPU generator on the same state.

A case = an engine position + a list of segment sizes (one normal_() call each).  The position is reached explicitly: a generator is
seeded, its state unpacked (mlhot.rng._unpack), advanced by `skip` outputs with mlhot_mt19937_advance and packed back; `left` and `next`
are asserted, not assumed.  With r = left - 1 usable words in the current block, the draw lengths sit around r, r + 624 j (a draw that
ends exactly on a block boundary must leave left = 1, next = 624) and n_sub * S * 624 from left = 1 (every sub-stream busy to its last
word); the sizes {16, 17, 31, 32, 33, 47, 48, 100} meet the Box-Muller tail rule (a size that is no multiple of 16 takes 16 more
outputs for its last 16 elements, which overlap the last body group) in several orders.

A total of t outputs is reachable as one segment of t elements (t % 16 == 0) or of t - 16 elements (t % 16 != 0, t >= 33): totals of
17 .. 31 do not exist, so `total == r + 1` is met where r + 1 is reachable."""
import functools
import types

import numpy as np
import torch

N = 624
ULP_BOUND = 6                                  # normals against torch's (Sleef inside ATen): the project's figure
TAIL_SIZES = (16, 17, 31, 32, 33, 47, 48, 100)
JUMP_CONFIGS = [(n_sub, S) for S in (1, 2) for n_sub in (2, 3, 8)]          # (sub-streams, blocks per sub-stream)
PAD = 64                                        # NaN floats behind the uniforms and behind the last segment

# name -> (outputs skipped after seeding, left, next); next of a freshly seeded engine is whatever torch sets (asserted as found: 0)
POSITIONS = {"seeded": (0, 1, None), "left624": (1, 624, 1), "left623": (2, 623, 2), "left17": (608, 17, 608), "left2": (623, 2, 623),
             "mid": (300, 325, 300), "block_end": (624, 1, 624)}


def outputs_of(sizes):
    return sum(n + (16 if n % 16 else 0) for n in sizes)


def _fill(sizes, total):
    """sizes + one more segment so that the draw takes exactly `total` outputs."""
    rest = total - outputs_of(sizes)
    n = rest if rest % 16 == 0 else rest - 16
    assert n >= 16 and outputs_of(list(sizes) + [n]) == total, (sizes, total)
    return list(sizes) + [n]


def _case(name, pos, sizes, seed=7, note=""):
    return types.SimpleNamespace(name=name, pos=pos, sizes=list(sizes), seed=seed, total=outputs_of(sizes), note=note)


def _table():
    T = TAIL_SIZES
    c = []
    # ---- mid-block, r = 324 ----
    c.append(_case("mid_below_r", "mid", [100], note="nb == 0"))
    c.append(_case("mid_equals_r", "mid", [308], note="nb == 0, the block used up: left = 1, next = 624"))
    c.append(_case("mid_r_plus_1", "mid", [309], note="one word of a new block"))
    c.append(_case("mid_block_end_1", "mid", _fill(T, 324 + 624), note="ends on a block boundary"))
    c.append(_case("mid_block_end_2", "mid", _fill(T[::-1], 324 + 2 * 624)))
    c.append(_case("mid_tails_interleaved", "mid", [33, 16, 100, 17, 48, 31, 32, 47, 17, 17, 16, 16, 33]))
    # ---- left = 624 / 623 / 17 / 2 ----
    c.append(_case("left624_below_r", "left624", [16]))
    c.append(_case("left624_equals_r", "left624", [607]))
    c.append(_case("left624_r_plus_1", "left624", [624]))
    c.append(_case("left624_block_end_2", "left624", _fill([47, 100, 17], 623 + 2 * 624)))
    c.append(_case("left623_equals_r", "left623", [606]))
    c.append(_case("left623_r_plus_1", "left623", [607]))
    c.append(_case("left17_equals_r", "left17", [16]))
    c.append(_case("left17_tail_in_new_block", "left17", [17], note="16 body uniforms from the old block, the tail's 16 and 1 more from the new"))
    c.append(_case("left17_block_end_1", "left17", _fill([31, 33], 16 + 624)))
    c.append(_case("left17_sixty_segments", "left17", [T[i % 8] for i in range(60)], note="the linear segment search"))
    c.append(_case("left2_one_group", "left2", [16]))
    c.append(_case("left2_block_end_1", "left2", [609]))
    # ---- left = 1: freshly seeded, and at the end of a block ----
    c.append(_case("seeded_one_group", "seeded", [16]))
    c.append(_case("seeded_one_word_into_block_2", "seeded", [609], note="total = 625"))
    c.append(_case("block_end_block_end_1", "block_end", [624]))
    c.append(_case("block_end_tails", "block_end", list(T[3:]) + list(T[:3])))
    for n_sub, S in JUMP_CONFIGS:                   # nb == n_sub * S exactly: 1248, 1872, 4992, 2496, 3744, 9984 outputs
        total = n_sub * S * N
        sizes = _fill(T if S == 1 else T[::-1], total) if n_sub != 3 else [total]
        c.append(_case(f"seeded_full_{n_sub}x{S}", "seeded", sizes, note="every sub-stream busy to its last word"))
    c.append(_case("seeded_blocks_5_and_a_bit", "seeded", _fill([100, 17], 5 * N + 40), note="the last block in a middle sub-stream of 8 x 1, the last of 3 x 2"))
    # ---- the one large case: one-workgroup route and DeviceNormal only (64 blocks: no jump table of stride 1 or 2 covers it) ----
    c.append(_case("mid_40k", "mid", [40001, 17, 48], note="40129 outputs"))
    return c


CASES = _table()
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def configs_for(c):
    """The jump configurations whose sub-streams cover the case (the entry refuses the others)."""
    return [(n_sub, S) for n_sub, S in JUMP_CONFIGS if n_sub * S * N >= c.total]


def segments(sizes):
    """(dst, size, src, first_group) per segment as mlhot.rng.DeviceNormal builds them -> (segs, out floats, outputs, groups)."""
    segs, dst, src, groups = [], 0, 0, 0
    for n in sizes:
        segs.append((dst, n, src, groups))
        dst += (n + 3) // 4 * 4
        src += n + (16 if n % 16 else 0)
        groups += n // 16 + (1 if n % 16 else 0)
    return segs, dst, src, groups


def chunk_plan(left0, total, n_sub, S):
    """mt_chunk_kernel's arithmetic restated: (new blocks, the sub-stream that makes the last one or None, left and next afterwards)."""
    r = left0 - 1 if left0 > 1 else 0
    fresh = total - r
    nb = (fresh + N - 1) // N if fresh > 0 else 0
    if nb == 0:
        return 0, None, left0 - total, None
    assert nb <= n_sub * S
    take = total - r - (nb - 1) * N
    return nb, (nb - 1) // S, N + 1 - take, take


# ---- the engine position -------------------------------------------------------------------------------------------------------
def positioned_state(lib, c):
    """The state tensor of a torch CPU generator seeded with c.seed and advanced to c.pos by mlhot_mt19937_advance; left and next
    asserted.  lib: any build of the library (the entry is host code)."""
    from mlhot.rng import _pack, _unpack
    skip, left, nxt = POSITIONS[c.pos]
    g = torch.Generator().manual_seed(c.seed)
    s0 = g.get_state()
    engine = _unpack(s0)
    assert int(engine[N]) == 1, "a freshly seeded engine has left == 1"
    if skip:
        lib.mt19937_advance(engine, skip)
    assert int(engine[N]) == left and (nxt is None or int(engine[N + 1]) == nxt), (c.pos, int(engine[N]), int(engine[N + 1]))
    state = _pack(s0, engine)
    # the position is torch's own after the same number of outputs
    if skip:
        torch.empty(skip).uniform_(generator=g)
        assert torch.equal(g.get_state(), state), c.pos
    back = _unpack(state)
    assert np.array_equal(back, engine)
    return state


def reference(state, sizes, draws=2):
    """torch's CPU generator from `state`: per draw the uniforms behind it (bits), the normals per segment and the engine afterwards;
    and 7 uniforms the generator gives after the last draw."""
    from mlhot.rng import _unpack
    total = outputs_of(sizes)
    out = []
    g = torch.Generator()
    g.set_state(state)
    for _ in range(draws):
        before = g.get_state()
        uniforms = torch.empty(total).uniform_(generator=g)
        g.set_state(before)
        normals = [torch.empty(n).normal_(generator=g) for n in sizes]
        out.append(types.SimpleNamespace(uniforms=uniforms, normals=normals, engine=_unpack(g.get_state()), state=g.get_state()))
    return out, torch.rand(7, generator=g)


def ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai, bi = np.where(ai < 0, -(ai & 0x7fffffff), ai), np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


@functools.lru_cache(maxsize=None)
def polys(S, n_sub):
    """int32 [n_sub - 1, 624] jump polynomials of stride S (mlhot.mt_jump: host seconds once per stride and process)."""
    from mlhot import mt_jump
    return torch.from_numpy(mt_jump.jump_polys(S, n_sub - 1).view(np.int32).copy())
