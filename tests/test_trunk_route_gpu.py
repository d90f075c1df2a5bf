"""The ResNet trunk's route on the MI355X (csrc/resnet_trunk.h trunk_route / trunk_plan): which launches one mlhot_trunk_fwd and one
mlhot_trunk_bwd send, in which order, and the scratch / activation sizes the library reports, for the smallest calls that reach
every decision of the route (the table of CASES).  The expected launch lists and sizes were recorded with these test bodies on the
commit BEFORE trunk_route() existed (options read where they were needed, the slab rows planned once for the size and once more for
the launches): they pin that the straight-line functions launch, and the one plan reserves, what the two copies did.  The same cases
run against torch in tests/test_gpu_parity.py::test_resnet_trunk_fwd_bwd_vs_torch.  Run with -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DEFAULTS = {"trunk_dual_dgrad": 1, "trunk_wg_rows": 128, "trunk_fuse34": 1}

# id -> (C, H, skip kernel per weight set, images per pass, one shared weight set?, options)
C5 = (3, 64, (3, 3, 1), (5, 2, 3), False)
CASES = {
    "c5_like": C5 + ({},),                                          # mixed skip kinds: two stage-A launches at block 1, wgrad34 holds (16 jobs)
    "no_fuse34": C5 + ({"trunk_fuse34": 0},),                       # per-block launches for blocks 3 and 4
    "no_dual": C5 + ({"trunk_dual_dgrad": 0},),                     # the two-launch 3x3-skip data gradient
    "rows16": C5 + ({"trunk_wg_rows": 16},),                        # another plan, other sizes
    "four_skip3": (3, 64, (3, 3, 3, 3), (2, 1, 3, 2), False, {}),   # both MAX_JOBS flushes; wgrad34 off (24 jobs > 16) under fuse34
    "six_shared": (3, 64, (1,), (1, 2, 1, 3, 1, 2), True, {}),      # MLHOT_TRUNK_MAX_PASS passes into adjacent row ranges of one set
    "distractor": (1, 128, (1, 3), (3, 2), False, {}),              # the other stem; fuse34 off by geometry; dual_dgrad at a 32 x 32 map
}


def _with_options(gpulib, opts, fn):
    try:
        for k, v in opts.items():
            gpulib.set_option(k, v)
        return fn()
    finally:
        for k, v in DEFAULTS.items():
            gpulib.set_option(k, v)


def _labels(gpulib, fn):
    gpulib.prof_begin(256)
    try:
        out = fn()
    finally:
        labels = [label for label, _ in gpulib.prof_end()]
    return labels, out


def _call(case):
    """(images per pass, weight set index per pass, [(26 tensors, skip_k)] per weight set) of a case, on the device."""
    C, H, skips, ns, share, _ = CASES[case]
    g = torch.Generator().manual_seed(sum(ns))
    imgs = [torch.rand(n, C, H, H, generator=g).to(DEV) for n in ns]
    wsets = []
    for k in skips:
        shapes = [(64, C, 5, 5)] + [s for _ in range(4) for s in ((64, 64, 3, 3), (64, 64, 3, 3), (64, 64, k, k))]
        ts = []
        for sh in shapes:
            ts += [(torch.randn(*sh, generator=g) * (1.5 / (sh[1] * sh[2] * sh[3])) ** 0.5).to(DEV), (torch.randn(64, generator=g) * 0.1).to(DEV)]
        wsets.append((ts, k))
    return imgs, [0 if share else i for i in range(len(ns))], wsets


def trunk_labels(gpulib, case):
    """(forward labels, backward labels) of one trunk_fwd + one trunk_bwd of a case."""
    imgs, wi, wsets = _call(case)
    H = CASES[case][1]
    dfeats = [torch.randn(im.shape[0], 64, H // 32, H // 32, generator=torch.Generator().manual_seed(1)).to(DEV) for im in imgs]

    def run():
        fwd, acts = _labels(gpulib, lambda: gpulib.trunk_fwd(list(zip(imgs, wi)), wsets))
        bwd, _ = _labels(gpulib, lambda: gpulib.trunk_bwd([(im, w, a) for im, w, a in zip(imgs, wi, acts)], wsets, dfeats))
        torch.cuda.synchronize()
        return fwd, bwd
    return _with_options(gpulib, CASES[case][5], run)


def trunk_scratch_bytes(gpulib, case):
    """[mlhot_trunk_scratch_bytes(backward = 0), (backward = 1)] of a case."""
    imgs, wi, wsets = _call(case)
    C, H = CASES[case][:2]
    pa, wa = gpulib._trunk_structs([(im, w, gpulib.trunk_acts(im)) for im, w in zip(imgs, wi)], wsets)
    return _with_options(gpulib, CASES[case][5],
                         lambda: [gpulib.c.mlhot_trunk_scratch_bytes(pa, len(imgs), wa, len(wsets), C, H, b) for b in (0, 1)])


# Recorded on the parent commit by trunk_labels / trunk_scratch_bytes above (see the module's docstring).
def _bwd_block(b, dgrads=("dgrad", "dgrad2"), conv1_wgrads=1):
    """Backward labels of an unfused block b: conv2's data and weight gradient, the stride-2 data gradient launches, conv1's weight gradient."""
    return ([f"trunk.bwd.conv2.dgrad.b{b}", f"trunk.bwd.conv2.wgrad.b{b}"] + [f"trunk.bwd.conv1.{d}.b{b}" for d in dgrads] +
            [f"trunk.bwd.conv1.wgrad.b{b}"] * conv1_wgrads)


BWD_END = ["trunk.bwd.skip1.wgrad", "trunk.bwd.stem.wgrad", "trunk.bwd.wsum"]
# c5's shape: block 1's stage A goes out per skip kind; ("dgrad", "dgrad2") = the 1x1-skip passes' launch, then the 3x3-skip passes' -
# the dual kernel and the second of the two-launch form carry the same label, so no_dual reads the same
C5_FWD = ["trunk.prep", "trunk.stem", "trunk.conv1.b1", "trunk.conv1.b1", "trunk.conv2.b1", "trunk.conv1.b2", "trunk.conv2.b2", "trunk.fwd.b34"]
C5_BWD = ["trunk.prep", "trunk.bwd.mask", "trunk.bwd.b34.dgrad", "trunk.bwd.b34.wgrad"] + _bwd_block(2) + _bwd_block(1) + BWD_END
EXPECTED = {
    "c5_like": (C5_FWD, C5_BWD),
    "no_fuse34": (C5_FWD[:-1] + ["trunk.conv1.b3", "trunk.conv2.b3", "trunk.conv1.b4", "trunk.conv2.b4"],
                  ["trunk.prep", "trunk.bwd.mask"] + _bwd_block(4) + _bwd_block(3) + _bwd_block(2) + _bwd_block(1) + BWD_END),
    "no_dual": (C5_FWD, C5_BWD),
    "rows16": (C5_FWD, C5_BWD),
    # eight stage-A jobs and eight conv1 + 3x3-skip weight-gradient jobs: two launches each, at every unfused block
    "four_skip3": (["trunk.prep", "trunk.stem", "trunk.conv1.b1", "trunk.conv1.b1", "trunk.conv2.b1", "trunk.conv1.b2", "trunk.conv1.b2", "trunk.conv2.b2",
                    "trunk.fwd.b34"],
                   ["trunk.prep", "trunk.bwd.mask", "trunk.bwd.b34.dgrad", "trunk.bwd.conv2.wgrad.b4", "trunk.bwd.conv1.wgrad.b4", "trunk.bwd.conv1.wgrad.b4",
                    "trunk.bwd.conv2.wgrad.b3", "trunk.bwd.conv1.wgrad.b3", "trunk.bwd.conv1.wgrad.b3"] + _bwd_block(2, ("dgrad2",), 2) +
                   _bwd_block(1, ("dgrad2",), 2) + ["trunk.bwd.stem.wgrad", "trunk.bwd.wsum"]),
    "six_shared": (["trunk.prep", "trunk.stem", "trunk.conv1.b1", "trunk.conv2.b1", "trunk.conv1.b2", "trunk.conv2.b2", "trunk.fwd.b34"],
                   ["trunk.prep", "trunk.bwd.mask", "trunk.bwd.b34.dgrad", "trunk.bwd.conv2.wgrad.b4", "trunk.bwd.conv1.wgrad.b4", "trunk.bwd.conv2.wgrad.b3",
                    "trunk.bwd.conv1.wgrad.b3"] + _bwd_block(2, ("dgrad",)) + _bwd_block(1, ("dgrad",)) + BWD_END),
    # 128 x 128: the 64 x 64 and the 32 x 32 inputs (blocks 1 and 2) split stage A by skip kind
    "distractor": (["trunk.prep", "trunk.stem", "trunk.conv1.b1", "trunk.conv1.b1", "trunk.conv2.b1", "trunk.conv1.b2", "trunk.conv1.b2", "trunk.conv2.b2",
                    "trunk.conv1.b3", "trunk.conv2.b3", "trunk.conv1.b4", "trunk.conv2.b4"],
                   ["trunk.prep", "trunk.bwd.mask"] + _bwd_block(4) + _bwd_block(3) + _bwd_block(2) + _bwd_block(1) + BWD_END),
}
# [forward, backward] bytes; the options that change no size (no_fuse34, no_dual) included
SCRATCH = {"c5_like": [5508352, 22740224], "no_fuse34": [5508352, 22740224], "no_dual": [5508352, 22740224], "rows16": [5508352, 18752000],
           "four_skip3": [7688448, 24029184], "six_shared": [1930496, 18463232], "distractor": [4360448, 32148992]}
# (C, H, n) -> floats of activation k = 0..8
ACT_FLOATS = {(3, 64, 5): [327680, 81920, 81920, 20480, 20480, 5120, 5120, 1280, 1280],
              (1, 128, 3): [786432, 196608, 196608, 49152, 49152, 12288, 12288, 3072, 3072]}


@pytest.mark.parametrize("case", list(CASES))
def test_trunk_launch_sequence(gpulib, case):
    fwd, bwd = trunk_labels(gpulib, case)
    print(f"[trunk route {case}] forward {fwd}\n[trunk route {case}] backward {bwd}")
    assert (fwd, bwd) == EXPECTED[case]


@pytest.mark.parametrize("case", list(CASES))
def test_trunk_scratch_bytes_are_what_they_were(gpulib, case):
    got = trunk_scratch_bytes(gpulib, case)
    print(f"[trunk route {case}] scratch bytes forward / backward {got}")
    assert got == SCRATCH[case]


def test_trunk_act_floats_are_what_they_were(gpulib):
    """mlhot_trunk_act_floats for k = 0..8 (a0, then (mid_i, y_i) of the four blocks) at one n per geometry."""
    got = {key: [gpulib.c.mlhot_trunk_act_floats(*key, k) for k in range(9)] for key in ACT_FLOATS}
    assert got == ACT_FLOATS
