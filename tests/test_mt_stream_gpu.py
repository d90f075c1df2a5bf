"""torch's CPU normal_() stream continued on the device (mlhot_mt19937_normal, mlhot_mt19937_normal_par; csrc/mt_normal.h) against
torch's own CPU generator over the case table of tests/mt_stream_cases.py: the uniforms bit for bit, the engine (624 words, left, next)
after one draw and after a second, every normal within 6 ulp, the one-workgroup route and every jump configuration with the same bits,
the padding of `out` and the floats behind the uniforms untouched, and the CPU generator continuing exactly after hand_back().
The entries are called through lib() with segments built the way DeviceNormal builds them, so that draws of a few hundred outputs take
the jump route too.  Run on the MI355X box:  pytest tests -m gpu.  Figures on record: profiles/INDEX_b1_envelope.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mt_stream_cases as MC
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1                   # csrc/common.h MLHOT_ERR_ARG
N = MC.N


def _engine_tensor(state):
    from mlhot.rng import _unpack
    return torch.from_numpy(_unpack(state).view(np.int32).copy()).to(DEV)


def _draws(gpulib, case, state, config, draws=2):
    """`draws` consecutive draws on one engine through the one-workgroup entry (config None) or the jump entry (config (n_sub, S)) ->
    per draw (uniform bits, out, engine) on the CPU; the workspaces are NaN beforehand and PAD floats longer than the entry needs."""
    segs, n_out, total, groups = MC.segments(case.sizes)
    assert total == case.total
    segs_d = torch.tensor(segs, dtype=torch.int64).to(DEV)
    engine = _engine_tensor(state)
    if config is not None:
        n_sub, S = config
        polys = MC.polys(S, n_sub).to(DEV)
        ws = torch.zeros(gpulib.mt19937_jump_ws_words(n_sub), dtype=torch.int32, device=DEV)
    res = []
    for _ in range(draws):
        u = torch.full((total + MC.PAD,), float("nan"), device=DEV)
        out = torch.full((n_out + MC.PAD,), float("nan"), device=DEV)
        if config is None:
            gpulib.mt19937_normal(engine, u, out, segs_d, len(segs), total, groups)
        else:
            gpulib.mt19937_normal_par(engine, u, out, segs_d, len(segs), total, groups, polys, n_sub, S, ws)
        torch.cuda.synchronize()
        res.append((u.cpu(), out.cpu(), engine.cpu().numpy().view(np.uint32).copy()))
    return res


def _check(case, res, ref, what):
    """One route's draws against torch's -> worst ulp."""
    segs, n_out, total, _ = MC.segments(case.sizes)
    worst = 0
    for d, ((u, out, engine), want) in enumerate(zip(res, ref)):
        assert torch.equal(u[:total].view(torch.int32), want.uniforms.view(torch.int32)), f"{case.name} {what} draw {d}: uniforms differ from torch's"
        assert bool(torch.isnan(u[total:]).all()), f"{case.name} {what}: written behind the uniforms"
        assert np.array_equal(engine[:N], want.engine[:N]), f"{case.name} {what} draw {d}: engine words"
        assert (int(engine[N]), int(engine[N + 1])) == (int(want.engine[N]), int(want.engine[N + 1])), \
            f"{case.name} {what} draw {d}: left, next = {int(engine[N])}, {int(engine[N + 1])}, torch's {int(want.engine[N])}, {int(want.engine[N + 1])}"
        written = torch.zeros(n_out + MC.PAD, dtype=torch.bool)
        for (dst, n, _, _), normals in zip(segs, want.normals):
            written[dst:dst + n] = True
            ulp = int(MC.ulps(out[dst:dst + n].numpy(), normals.numpy()).max())
            worst = max(worst, ulp)
            assert ulp <= MC.ULP_BOUND, f"{case.name} {what} draw {d}, segment of {n} at {dst}: {ulp} ulp"
        assert bool(torch.isnan(out[~written]).all()), f"{case.name} {what} draw {d}: padding between or behind the segments written"
    return worst


@pytest.mark.parametrize("case", MC.CASES, ids=MC.CASE_IDS)
def test_mt_stream_over_the_table(gpulib, case):
    state = MC.positioned_state(gpulib, case)
    ref, after = MC.reference(state, case.sizes)
    one = _draws(gpulib, case, state, None)
    worst = _check(case, one, ref, "one workgroup")
    for config in MC.configs_for(case):
        par = _draws(gpulib, case, state, config)
        worst = max(worst, _check(case, par, ref, f"jump {config[0]} x {config[1]}"))
        for (u0, o0, e0), (u1, o1, e1) in zip(one, par):
            assert torch.equal(u0.view(torch.int32), u1.view(torch.int32)) and torch.equal(o0.view(torch.int32), o1.view(torch.int32)) \
                and np.array_equal(e0, e1), f"{case.name}: jump {config} and the one-workgroup route differ in bits"
    print(f"mt_stream {case.name}: {len(MC.configs_for(case))} jump configurations, worst {worst} ulp")
    U.parity_log(f"mt_stream {case.name} worst_ulp {worst}")
    # through DeviceNormal (one workgroup: its own jump route starts at n_sub * 2496 outputs with strides of its own)
    from mlhot.rng import DeviceNormal
    g = torch.Generator()
    g.set_state(state)
    dn = DeviceNormal(DEV, case.sizes, sub_streams=1)
    assert (dn.total, dn.total_outputs, dn.total_groups) == MC.segments(case.sizes)[1:]
    dn.take_over(g)
    for d in range(2):
        flat = dn.draw().cpu()
        assert all(torch.equal(flat[o:o + n].view(torch.int32), one[d][1][o:o + n].view(torch.int32)) for o, n in zip(dn.offsets, case.sizes))
    dn.hand_back()
    assert torch.equal(torch.rand(7, generator=g), after), f"{case.name}: the CPU generator does not continue where torch's would"


@pytest.mark.parametrize("n_sub,S", MC.JUMP_CONFIGS, ids=[f"{n}x{S}" for n, S in MC.JUMP_CONFIGS])
def test_mt_one_output_too_many_is_refused(gpulib, n_sub, S):
    """total_outputs = n_sub * S * 624 + 1: MLHOT_ERR_ARG, and the engine, the uniforms and `out` are as they were."""
    case = MC.BY_NAME["seeded_one_group"]
    state = MC.positioned_state(gpulib, case)
    segs, n_out, _, groups = MC.segments(case.sizes)
    segs_d = torch.tensor(segs, dtype=torch.int64).to(DEV)
    engine = _engine_tensor(state)
    keep = engine.clone()
    polys = MC.polys(S, n_sub).to(DEV)
    ws = torch.zeros(gpulib.mt19937_jump_ws_words(n_sub), dtype=torch.int32, device=DEV)
    u, out = torch.full((256,), float("nan"), device=DEV), torch.full((256,), float("nan"), device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    rc = gpulib.c.mlhot_mt19937_normal_par(P(engine), P(u), P(out), P(segs_d), len(segs), n_sub * S * N + 1, groups, P(polys), n_sub, S, P(ws), s)
    assert rc == ERR_ARG and b"do not cover" in gpulib.c.mlhot_last_error()
    torch.cuda.synchronize()
    assert torch.equal(engine, keep) and bool(torch.isnan(u).all()) and bool(torch.isnan(out).all()) and not ws.any()


@pytest.mark.parametrize("sizes", [[15], [16, 8, 32]])
def test_device_normal_refuses_small_draws_before_take_over(gpulib, sizes):
    from mlhot.rng import DeviceNormal
    before = torch.get_rng_state()
    with pytest.raises(ValueError):
        DeviceNormal(DEV, sizes)
    assert torch.equal(torch.get_rng_state(), before)
