"""tests/favor_linear_cases.py and tests/favor_linear_ref.py are fit to judge the linear-form FAVOR+ route (csrc/favor_linear.h): the
hand-derived formulas agree with the autograd reference in float64, the query / key gradients are live where the table says so, and
every case sits above the 32-shot cap and inside the envelope that favor_linear.h's own constants state."""
import os
import re

import pytest
import torch

from tests import favor_linear_cases as LC
from tests import favor_linear_ref as LR

FAVOR_LINEAR_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "what-matters-for-meta-learning_amd", "csrc",
                              "favor_linear.h")


@pytest.mark.parametrize("name", LC.CASE_IDS)
def test_formulas_agree_with_the_autograd_reference(name):
    """out, dq, dk, dv of the restated formulas against O.favor_attention + backward, both float64: 1e-10 of each tensor's scale (dead
    tensors at dv's scale)."""
    c = LC.BY_NAME[name]
    ref = LC.reference(c, torch.float64)
    got = LR.run(LC.inputs(name))
    floor = LC.floors(c, ref)
    for n in LC.NAMES:
        scale = max(ref[n].abs().max().item(), floor[n], 1e-300)
        err = (got[n] - ref[n]).abs().max().item() / scale
        print(f"favor_linear_ref {name} {n}: {err:.2e}")
        assert err <= 1e-10, (name, n, err)


@pytest.mark.parametrize("name", LC.CASE_IDS)
def test_gradients_are_live_or_exactly_zero(name):
    """dq and dk reach at least 1e-3 of dv's scale in every case not marked dead; with one key they are exactly zero."""
    c = LC.BY_NAME[name]
    r = LC.reference(c, torch.float64)
    assert all(bool(torch.isfinite(t).all()) for t in r.values())
    dv = r["dv"].abs().max().item()
    ratio = {n: r[n].abs().max().item() / dv for n in ("dq", "dk")}
    print(f"favor_linear_cases {name} live: max|dq| / max|dv| = {ratio['dq']:.3g}, max|dk| / max|dv| = {ratio['dk']:.3g}")
    for n in ("dq", "dk"):
        if n in c.exact_zero:
            assert ratio[n] < 1e-6, (name, n, ratio[n])
        elif n not in c.dead:
            assert ratio[n] >= 1e-3, (name, n, ratio[n])
    if c.Nc == 1:      # with the centre Ctx is exactly 0: the restated formulas give exact zeros, not residue
        got = LR.run(LC.inputs(name))
        assert not got["dq"].any() and not got["dk"].any()


def test_reference_float32_error_keeps_the_bound_tight():
    """e32 <= RTOL on every case, as tests/test_favor_cases_cpu.py asks of its table: the bound RTOL + 2 e32 never exceeds 3e-4."""
    for c in LC.CASES:
        e = LC.e32(c)
        print(f"favor_linear_cases {c.name} e32: " + " ".join(f"{n}={e[n]:.2e}" for n in LC.NAMES))
        for n in LC.NAMES:
            assert LC.bounds(c)[n] <= 3e-4, (c.name, n, e[n])


def test_variants_are_what_the_table_says():
    for c in LC.CASES:
        x = LC.inputs(c.name)
        if c.variant == "dup":
            assert bool((x.k == x.k[0, 0, 0]).all()) and torch.equal(x.q[:, :, 0], x.q[:, :, 1]) and not torch.equal(x.q[:, :, 0], x.q[:, :, 2])
        if c.variant == "peak_last":
            dd = torch.einsum("thnd,md->thnm", x.k.double() * c.d ** -0.25, x.proj.double())
            t, h, n, _ = (int(i) for i in torch.unravel_index(dd.argmax(), dd.shape))
            assert (t, n) == (c.T - 1, c.Nc - 1) and n // 16 == (c.Nc - 1) // 16, (t, h, n)


def _constants():
    src = open(FAVOR_LINEAR_H).read()
    env = {}
    for name in ("MINN", "MIND", "MAXD", "MINM", "MAXM"):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, src)
        assert m, name
        env[name] = int(eval(m.group(1), {}, dict(env)))
    return src, env


def test_cases_sit_above_the_cap_and_inside_the_envelope():
    """fl::applies() restated from favor_linear.h's own constants; the table's envelope is literals, so a change of a constant or of
    the guard makes this test speak up."""
    src, k = _constants()
    guard = re.search(r"inline bool applies\(const FavorDims& f\) \{ return ([^;]+); \}", src)
    assert guard and guard.group(1) == ("(f.Nq > MINN || f.Nc > MINN) && f.Nq >= 1 && f.Nc >= 1 && f.d % 16 == 0 && f.d >= MIND && f.d <= MAXD && "
                                        "f.m >= MINM && f.m <= MAXM && grid_ok(f)")
    assert (k["MINN"], k["MIND"], k["MAXD"], k["MINM"], k["MAXM"]) == (32, 16, 256, 16, 1536)
    for c in LC.CASES:
        applies = (max(c.Nq, c.Nc) > k["MINN"] and c.d % 16 == 0 and k["MIND"] <= c.d <= k["MAXD"] and k["MINM"] <= c.m <= k["MAXM"])
        assert applies and LC.in_envelope(*c.shape), c.name
    # the table reaches the envelope's edges
    assert {c.d for c in LC.CASES} >= {16, 256} and {c.m for c in LC.CASES} >= {16, 17, 1536}
    assert any(c.Nq <= 32 < c.Nc for c in LC.CASES) and any(c.Nc <= 32 < c.Nq for c in LC.CASES) and any(c.Nc == 33 for c in LC.CASES)
    for shape in ((2, 2, 16, 16, 64, 266), (1, 2, 6, 40, 40, 147), (1, 1, 5, 40, 64, 1537), (1, 2, 5, 40, 64, 15), (1, 1, 40, 40, 272, 266)):
        assert not LC.in_envelope(*shape), shape
