"""tests/favor_cases.py is fit to judge a kernel: the float64 reference's own float32 error stays under the project's tolerance on
every case, the query / key gradients are live where the table says so (and exactly zero where it says that), and every case sits on
the route - two-launch kernels or operator chain, <2> or <4> row tiles, number of feature chunks - that the table names."""
import math
import os
import re

import pytest
import torch

from tests import favor_cases as FC
from tests import util as U

FAVOR2_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "what-matters-for-meta-learning_amd", "csrc", "favor2.h")


@pytest.mark.parametrize("name", FC.CASE_IDS)
def test_reference_float32_error_is_under_the_tolerance(name):
    """e32 = rel_err(reference in float32, reference in float64) <= RTOL for out, dq, dk, dv: the bound RTOL + 2 e32 of the GPU test
    then never exceeds 3e-4.  (Dead tensors are measured at dv's scale.)"""
    c = FC.BY_NAME[name]
    e = FC.e32(c)
    print(f"favor_cases {name} e32: " + " ".join(f"{n}={e[n]:.2e}" for n in FC.NAMES))
    for n in FC.NAMES:
        assert e[n] <= U.RTOL, (name, n, e[n])
        assert FC.bounds(c)[n] <= 3e-4


@pytest.mark.parametrize("name", FC.CASE_IDS)
def test_gradients_are_live_or_exactly_zero(name):
    c = FC.BY_NAME[name]
    r = FC.reference(c, torch.float64)
    assert all(bool(torch.isfinite(t).all()) for t in r.values())
    dv = r["dv"].abs().max().item()
    ratio = {n: r[n].abs().max().item() / dv for n in ("dq", "dk")}
    print(f"favor_cases {name} live: max|dq| / max|dv| = {ratio['dq']:.3g}, max|dk| / max|dv| = {ratio['dk']:.3g}")
    for n in ("dq", "dk"):
        if n in c.exact_zero:
            assert ratio[n] < 1e-6, (name, n, ratio[n])
        elif n not in c.dead:
            assert ratio[n] >= 0.2, (name, n, ratio[n])


def test_dup_and_outlier_inputs_are_what_the_table_says():
    for c in FC.CASES:
        x = FC.inputs(c.name)
        if c.variant == "dup":
            assert bool((x.k == x.k[0, 0, 0]).all()) and torch.equal(x.q[:, :, 0], x.q[:, :, 1]) and not torch.equal(x.q[:, :, 0], x.q[:, :, 2])
            r = FC.reference(c, torch.float64)
            assert torch.equal(r["out"][:, :, 0], r["out"][:, :, 1])
        if c.variant == "outlier":
            # every key feature but the outlier row's sits under the +1e-4 floor: exp(dd - diag - max) < 1e-4
            dd = torch.einsum("thnd,md->thnm", x.k.double() * c.d ** -0.25, x.proj.double())
            arg = dd - (x.k.double() ** 2).sum(-1, keepdim=True) * 0.5 * c.d ** -0.5 - dd.max()
            arg[0, 0, 0] = -1e9
            assert arg.max().item() < math.log(1e-4)


def _constants():
    src = open(FAVOR2_H).read()
    env = {}
    for name in ("F1_TPW", "FCH", "MAXN", "NPMAX"):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, src)
        assert m, name
        env[name] = int(eval(m.group(1), {}, dict(env)))
    return src, env


def test_cases_sit_on_the_route_the_table_names():
    """fv::applies() and the <2> / <4> dispatch restated from favor2.h's own constants; the table's route, rt and chunks are literals,
    so a change of MAXN, FCH or NPMAX (or of the guard) makes this test speak up."""
    src, k = _constants()
    guard = re.search(r"inline bool applies\(const FavorDims& f\) \{ return ([^;]+); \}", src)
    assert guard and guard.group(1) == ("f.Nq <= MAXN && f.Nc <= MAXN && f.d % 16 == 0 && f.d <= 256 && f.m >= 16 && f.m <= FCH * NPMAX / 4")
    assert src.count("if (R <= 32) hipLaunchKernelGGL((f1_kernel<2>)") == 1 and src.count("if (R <= 32) hipLaunchKernelGGL((b2_kernel<2>)") == 1
    assert src.count("else hipLaunchKernelGGL((f1_kernel<4>)") == 1 and src.count("else hipLaunchKernelGGL((b2_kernel<4>)") == 1
    assert (k["MAXN"], k["FCH"], k["NPMAX"]) == (32, 192, 32)
    seen = set()
    for c in FC.CASES:
        applies = c.Nq <= k["MAXN"] and c.Nc <= k["MAXN"] and c.d % 16 == 0 and c.d <= 256 and c.m >= 16 and c.m <= k["FCH"] * k["NPMAX"] // 4
        stated = c.Nq <= 32 and c.Nc <= 32 and c.d % 16 == 0 and c.d <= 256 and 16 <= c.m <= 1536
        assert applies == stated == (c.route == "two_launch"), c.name
        if c.route == "two_launch":
            assert c.rt == (2 if c.Nq + c.Nc <= 32 else 4), c.name
            assert c.chunks == -(-c.m // k["FCH"]) == -(-c.m // 192) and 4 * c.chunks <= k["NPMAX"], c.name
            seen.add((c.rt, c.chunks))
        else:
            assert c.rt is None and c.chunks is None
    assert {(2, 1), (2, 2), (2, 8), (4, 1), (4, 2), (4, 4), (4, 8)} <= seen
    assert all(c.route == "two_launch" for c in FC.STAGED[:2]) and FC.STAGED[2].route == "chain"
