"""No GPU: the case table of tests/mt_stream_cases.py proven against torch here.  Every engine position is reached and asserted; on
every case the restatement of torch's stream (oracle/mt_normal.py) gives torch's uniforms bit for bit, torch's normals within 6 ulp and
torch's engine after one draw and after two; the table is shown to hold every branch of mt_fill_kernel / mt_chunk_kernel it is meant
to walk (by the restatement of the kernel's own arithmetic, chunk_plan, held against torch's left / next).  The GPU run of the table is
tests/test_mt_stream_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import mt_normal as MT
from tests import mt_stream_cases as MC

N = MC.N


@pytest.fixture(scope="module")
def states(hostsim):
    return {c.name: MC.positioned_state(hostsim, c) for c in MC.CASES}


def test_every_position_is_reached_and_asserted(hostsim, states):
    from mlhot.rng import _unpack
    seen = set()
    for c in MC.CASES:
        e = _unpack(states[c.name])
        seen.add(int(e[N]))
        if c.pos == "seeded":
            assert int(e[N]) == 1 and int(e[N + 1]) == 0
        if c.pos == "block_end":
            assert int(e[N]) == 1 and int(e[N + 1]) == 624
    assert seen == {1, 2, 17, 325, 623, 624}


@pytest.mark.parametrize("case", MC.CASES, ids=MC.CASE_IDS)
def test_the_restatement_gives_torchs_stream_on_every_case(states, case):
    state = states[case.name]
    ref, _ = MC.reference(state, case.sizes)
    st, left, nxt = MT.unpack_state(state)
    for draw in ref:
        raw, _, _, _ = MT.raw_outputs(st, left, nxt, case.total)
        assert np.array_equal(MT.uniforms(raw).view(np.int32), draw.uniforms.numpy().view(np.int32)), "uniforms differ from torch's"
        for n, want in zip(case.sizes, draw.normals):
            x, st, left, nxt = MT.normal_(n, st, left, nxt)
            assert MC.ulps(x, want.numpy()).max() <= MC.ULP_BOUND, (case.name, n)
        assert np.array_equal(st, draw.engine[:N]) and (left, nxt) == (int(draw.engine[N]), int(draw.engine[N + 1])), case.name


def test_the_kernels_hand_over_arithmetic_gives_torchs_left_and_next(states):
    """chunk_plan (mt_chunk_kernel's r, nb, take, left = N + 1 - take, next = take, restated) against torch's engine after the draw, on
    every case and jump configuration; a draw that ends on a block boundary leaves left = 1, next = 624."""
    from mlhot.rng import _unpack
    for c in MC.CASES:
        left0 = int(_unpack(states[c.name])[N])
        ref, _ = MC.reference(states[c.name], c.sizes, draws=1)
        left1, next1 = int(ref[0].engine[N]), int(ref[0].engine[N + 1])
        for n_sub, S in MC.configs_for(c):
            nb, k, left, nxt = MC.chunk_plan(left0, c.total, n_sub, S)
            assert left == left1 and (nxt is None or nxt == next1), (c.name, n_sub, S)
        r = left0 - 1
        if c.total >= r and (c.total - r) % N == 0:
            assert (left1, next1) == (1, 624), c.name


def test_the_table_walks_every_branch(states):
    from mlhot.rng import _unpack
    hit = set()
    for c in MC.CASES:
        left0 = int(_unpack(states[c.name])[N])
        r = left0 - 1
        hit.add("total<r" if c.total < r else "total==r" if c.total == r else "total==r+1" if c.total == r + 1 else "")
        for j in (1, 2):
            if c.total == r + N * j:
                hit.add(f"block_end_{j}")
        for n_sub, S in MC.configs_for(c):
            nb, k, _, _ = MC.chunk_plan(left0, c.total, n_sub, S)
            if nb == 0:
                hit.add("nb==0")
                continue
            if left0 <= 1:
                hit.add("left0<=1")
            hit.add("last_in_0" if k == 0 else "last_in_last" if k == n_sub - 1 else "last_in_middle")
            if n_sub >= 3 and 0 < k < n_sub - 1:
                hit.add("later_sub_streams_idle")
            if nb == n_sub * S and left0 == 1 and c.total == n_sub * S * N:
                hit.add(f"full_{n_sub}x{S}")
    want = {"total<r", "total==r", "total==r+1", "block_end_1", "block_end_2", "nb==0", "left0<=1", "last_in_0", "last_in_middle", "last_in_last",
            "later_sub_streams_idle"} | {f"full_{n}x{S}" for n, S in MC.JUMP_CONFIGS}
    assert want <= hit, want - hit
    sizes = {n for c in MC.CASES for n in c.sizes}
    assert set(MC.TAIL_SIZES) <= sizes and max(len(c.sizes) for c in MC.CASES) == 60 and any(len(c.sizes) == 1 for c in MC.CASES)
    totals = sorted(c.total for c in MC.CASES)
    assert totals[-1] > 40000 and totals[-2] < 10000
    orders = {tuple(n for n in c.sizes if n in MC.TAIL_SIZES)[:8] for c in MC.CASES if set(MC.TAIL_SIZES) <= set(c.sizes)}
    assert len(orders) >= 3


def test_segments_are_device_normals():
    """segments() is the layout mlhot.rng.DeviceNormal builds (its constructor needs no GPU up to the first device allocation: the
    sizes are checked first); dst rounds up to 4 floats, a size that is no multiple of 16 takes 16 more outputs and one more group."""
    segs, dst, src, groups = MC.segments([17, 16, 33])
    assert segs == [(0, 17, 0, 0), (20, 16, 33, 2), (36, 33, 49, 3)] and (dst, src, groups) == (72, 98, 6)


@pytest.mark.parametrize("sizes", [[15], [16, 8, 32], []])
def test_device_normal_refuses_small_draws_before_it_touches_the_generator(sizes):
    from mlhot.rng import DeviceNormal
    before = torch.get_rng_state()
    with pytest.raises(ValueError):
        DeviceNormal("cuda:0", sizes, sub_streams=1)
    assert torch.equal(torch.get_rng_state(), before)
