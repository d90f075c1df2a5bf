"""Shared by tests/test_glue_ops_cpu.py (host flavour of the library) and tests/test_glue_ops_gpu.py (MI355X): the element-wise and
per-segment glue kernels called directly through the binding, each against torch on the CPU - bitwise where the operation is a single
rounding (add_relu, axpy, pool2 and their backwards), at util.RTOL against float64 where it sums (spatial_mean, bn_relu, Adam).

Sizes: run_foreach (csrc/foreach.h) clamps its grid at 4096 workgroups of 256 threads and strides beyond, so 4096 * 256 - 1, + 0, + 1
straddle the clamp; 255 / 256 / 257 straddle one workgroup; run_reduce_seg folds N * HW items per channel through a 256-thread tree."""
import pytest
import torch
import torch.nn.functional as F

from tests import util as U

CLAMP = 4096 * 256
FOREACH_N = [1, 255, 256, 257, CLAMP - 1, CLAMP, CLAMP + 1]
MEAN_SHAPES = [(planes, hw) for hw in (1, 4, 49) for planes in (1, 257)]
POOL_SHAPES = [(1, 2, 2), (3, 2, 6), (3, 6, 2), (5, 10, 14), (257, 16, 16)]
# count = N * HW: 2 (twice), 255 at C = 3, just under / at / over the 256-thread tree at C = 64, 240 spread over 15 shots, and 5100 >> 256 at C = 7
BN_SHAPES = [(1, 1, 2), (2, 3, 1), (5, 3, 51), (1, 64, 255), (1, 64, 256), (1, 64, 257), (15, 64, 16), (3, 7, 1700)]
BN_MOMENTA = [0.1, 0.3]


def need(lib, symbol):
    """The CPU twin runs wherever the host flavour exports the entry."""
    if not hasattr(lib.c, symbol):
        pytest.skip(f"hostsim lacks {symbol}")


def bits_equal(a, b):
    """Same fp32 bit patterns (torch.equal would take -0.0 for 0.0)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- add_relu ---------------------------------------------------------------------------------------------------------------
def add_relu_inputs(n):
    """N(0, 1) pairs with, strided through them (and all of them among the first elements, so that n = 1 .. 257 see them too): exact
    a + b == 0 of both orders, every pairing of -0.0 and 0.0, -0.0 beside an ordinary value, and sums that land in the fp32 subnormals
    (a flush-to-zero adder rounds those to zero) of either sign."""
    g = _gen(11 + n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    special = [(None, "neg"), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 0.0), (-0.0, 1.25), (-0.0, -1.25), (1.5e-38, -1.4e-38),
               (-1.5e-38, 1.4e-38), (2.5, -2.5)]
    for k, (va, vb) in enumerate(special):
        for start, step in ((k, 64), (3 * k + 1, 997)):
            if va is None:
                b[start::step] = -a[start::step]
            else:
                a[start::step], b[start::step] = va, vb
    return a, b


def check_add_relu(lib, n, dev):
    a, b = add_relu_inputs(n)
    dy = torch.randn(n, generator=_gen(n))
    a_ref = a.clone().requires_grad_(True)
    y_ref = torch.relu(a_ref + b)
    y_ref.backward(dy)
    y = lib.add_relu_fwd(a.to(dev), b.to(dev))
    assert bits_equal(y, y_ref), f"add_relu_fwd n={n}: {int((y.cpu().view(torch.int32) != y_ref.detach().view(torch.int32)).sum())} elements differ"
    g = lib.add_relu_bwd(y, dy.to(dev))
    assert bits_equal(g, a_ref.grad), f"add_relu_bwd n={n}"


# ---- axpy -------------------------------------------------------------------------------------------------------------------
def check_axpy(lib, n, dev, with_a):
    """y = a + alpha * x with the product and the sum rounded separately: the bits of the two fp32 torch operators."""
    g = _gen(23 + n)
    x, a = torch.randn(n, generator=g), torch.randn(n, generator=g)
    alpha = torch.tensor(0.37, dtype=torch.float32)            # the fp32 value the C ABI receives
    prod = x * alpha
    want = a + prod if with_a else prod
    got = lib.axpy(a.to(dev) if with_a else None, x.to(dev), float(alpha))
    assert bits_equal(got, want), f"axpy n={n} with_a={with_a}"


# ---- spatial mean -----------------------------------------------------------------------------------------------------------
def check_spatial_mean(lib, planes, hw, dev):
    """Worst error of (forward, backward) against float64; x = 3 + N(0, 1) keeps the mean away from cancellation."""
    g = _gen(31 + planes + 1000 * hw)
    n, c = (planes, 1) if planes % 257 else (planes // 257, 257)
    x = 3.0 + torch.randn(n, c, hw, generator=g)
    dy = torch.randn(n, c, generator=g)
    x64 = x.double().requires_grad_(True)
    y64 = x64.mean(dim=2)
    y64.backward(dy.double())
    y = lib.spatial_mean_fwd(x.to(dev))
    dx = lib.spatial_mean_bwd(dy.to(dev), (n, c, hw))
    assert y.shape == (n, c) and dx.shape == (n, c, hw)
    errs = (U.rel_err(y, y64), U.rel_err(dx, x64.grad))
    print(f"glue spatial_mean planes={planes} HW={hw}: fwd {errs[0]:.2e} bwd {errs[1]:.2e}")
    assert max(errs) <= U.RTOL, errs
    return errs


# ---- pool2 ------------------------------------------------------------------------------------------------------------------
POOL_VALUES = torch.tensor([-1.5, -0.0, 0.0, 0.75, 0.75])  # four values (the largest twice as likely): ~ 64 % of the 2 x 2 windows tie; -0.0 against 0.0; both signs


def check_pool2(lib, shape, dev):
    planes, H, W = shape
    g = _gen(41 + planes + 10 * H + 100 * W)
    x = POOL_VALUES[torch.randint(0, 5, (1, planes, H, W), generator=g)]
    dy = torch.randn(1, planes, H // 2, W // 2, generator=g)
    x_ref = x.clone().requires_grad_(True)
    y_ref, idx = F.max_pool2d(x_ref, 2, return_indices=True)
    y_ref.backward(dy)
    code = (((idx // W) & 1) << 1) | ((idx % W) & 1)          # torch's flat index in the plane -> the window code the kernel stores
    y, amax = lib.pool2_fwd(x.to(dev))
    assert amax.dtype == torch.uint8 and bits_equal(y, y_ref), f"pool2_fwd {shape}: values"
    assert torch.equal(amax.cpu().long(), code), f"pool2_fwd {shape}: arg-max (ATen's first maximum in scan order)"
    dx = lib.pool2_bwd(dy.to(dev), amax, H, W)
    assert bits_equal(dx, x_ref.grad), f"pool2_bwd {shape}"
    ties = float((x.reshape(planes, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(-1, 4) == y_ref.detach().reshape(-1, 1)).sum(1).gt(1).float().mean())
    assert planes * H * W < 400 or ties > 0.5, "the inputs are meant to tie in most windows"


def check_pool2_refusals(lib, dev):
    from mlhot.binding import MlhotError
    for shape in ((1, 1, 3, 2), (1, 1, 2, 3), (1, 1, 0, 2), (1, 1, 2, 0), (0, 1, 2, 2), (1, 0, 2, 2)):
        x = torch.zeros(shape, device=dev)
        with pytest.raises(MlhotError):
            lib.pool2_fwd(x)
        n, c, H, W = shape
        with pytest.raises(MlhotError):
            lib.pool2_bwd(torch.zeros(n, c, H // 2, W // 2, device=dev), torch.zeros(n, c, H // 2, W // 2, dtype=torch.uint8, device=dev), H, W)


# ---- bn_relu ----------------------------------------------------------------------------------------------------------------
def bn_inputs(shape):
    """x = 3 + N(0, 1), gamma in [0.5, 1.5], beta in [-0.5, 0.5]: |mean| ~ 3, variance ~ 1 >> eps."""
    N, C_, HW = shape
    g = _gen(53 + N + 10 * C_ + 1000 * HW)
    return (3.0 + torch.randn(N, C_, HW, generator=g), 0.5 + torch.rand(C_, generator=g), torch.rand(C_, generator=g) - 0.5,
            torch.randn(C_, generator=g), 0.5 + torch.rand(C_, generator=g), torch.randn(N, C_, HW, generator=g))


def bn_reference(x, gamma, beta, rm, rv, dy, momentum, eps, y_kernel, dtype=torch.float64):
    """F.batch_norm(training=True) + ReLU and its autograd in `dtype`; the ReLU mask of the backward is the kernel's y > 0."""
    x_, g_, b_ = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    rm_, rv_ = (None, None) if rm is None else (rm.to(dtype).clone(), rv.to(dtype).clone())
    pre = F.batch_norm(x_, rm_, rv_, g_, b_, training=True, momentum=momentum, eps=eps)
    (pre * (y_kernel.cpu() > 0).to(dtype)).backward(dy.to(dtype))
    xd = x.to(dtype)
    return dict(y=torch.relu(pre).detach(), mean=xd.mean(dim=(0, 2)), var=xd.var(dim=(0, 2), unbiased=False), run_mean=rm_, run_var=rv_,
                dx=x_.grad, dgamma=g_.grad, dbeta=b_.grad)


def bn_kernel(lib, x, gamma, beta, rm, rv, dy, momentum, eps, dev):
    rm_d, rv_d = (None, None) if rm is None else (rm.clone().to(dev), rv.clone().to(dev))
    xd, gd = x.to(dev), gamma.to(dev)
    y, mean, var = lib.bn_relu_fwd(xd, gd, beta.to(dev), rm_d, rv_d, momentum, eps)
    dx, dgamma, dbeta = lib.bn_relu_bwd(xd, y, dy.to(dev), gd, mean, var, eps)
    return dict(y=y, mean=mean, var=var, run_mean=rm_d, run_var=rv_d, dx=dx, dgamma=dgamma, dbeta=dbeta)


def bn_errors(got, ref):
    return {k: U.rel_err(got[k], ref[k]) for k in ref if ref[k] is not None}


def check_bn(lib, shape, momentum, dev, running=True, eps=1e-5):
    """y, batch mean, biased variance, the in-place running-statistics update (unbiased variance), dx, dgamma, dbeta against float64 at
    util.RTOL; the inputs keep |mean| ~ 3, the variance ~ 1 >> eps and the largest dx away from cancellation.

    One output cannot meet RTOL in fp32 whatever the kernel does: dx at count == 2, the shapes (1, 1, 2) and (2, 3, 1).  With two
    samples xhat = +-s, s^2 = var / (var + eps), and dx = gamma / sqrt(var + eps) * (g0 - g1) / 2 * (1 - s^2): the three terms of
    the formula are O(1) and cancel to eps / (var + eps) ~ 1e-5 of themselves, so one ulp in the mean or the variance is ~ 1e-2 of dx.
    For dx of those two shapes the bound is therefore 4 x the error of torch's own fp32 CPU F.batch_norm + autograd against the same
    float64 reference on the same inputs (computed here, never from the kernel's output).  Measured on the build host: (1, 1, 2): torch
    fp32 1.3e-2 -> bound 5.2e-2, host flavour of the kernel 2.8e-2; (2, 3, 1): torch fp32 1.1e-3 -> bound 4.4e-3, host flavour 1.2e-3."""
    N, _, HW = shape
    x, gamma, beta, rm, rv, dy = bn_inputs(shape)
    if not running:
        rm = rv = None
    got = bn_kernel(lib, x, gamma, beta, rm, rv, dy, momentum, eps, dev)
    ref = bn_reference(x, gamma, beta, rm, rv, dy, momentum, eps, got["y"])
    bounds = {k: U.RTOL for k in ref}
    if N * HW == 2:
        t32 = bn_reference(x, gamma, beta, rm, rv, dy, momentum, eps, got["y"], dtype=torch.float32)
        bounds["dx"] = max(U.RTOL, 4.0 * U.rel_err(t32["dx"], ref["dx"]))
    errs = bn_errors(got, ref)
    assert running == ("run_mean" in errs)
    print(f"glue bn_relu {shape} momentum={momentum} running={running}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f" (dx bound {bounds['dx']:.2e})")
    for k, e in errs.items():
        assert e <= bounds[k], f"bn_relu {shape}: {k} rel err {e:.2e} > {bounds[k]:.2e}"
    return errs


def check_bn_count1(lib, C_, momentum, dev, eps=1e-5):
    """count == 1, shape (1, C, 1): torch refuses it.  The formulas of csrc/ops_direct.h written out: mean = x, var = 0, so
    y = relu(gamma * 0 / sqrt(eps) + beta) = relu(beta); run_mean <- (1 - m) run_mean + m x; the running variance takes the biased
    variance (0) where the unbiased one does not exist: run_var <- (1 - m) run_var.  Backward with g = dy * (y > 0): xhat = 0, so
    dbeta = g, dgamma = g * xhat = 0, dx = gamma / sqrt(eps) * (g - g / 1 - 0 * dgamma / 1) = 0."""
    x, gamma, beta, rm, rv, dy = bn_inputs((1, C_, 1))
    got = bn_kernel(lib, x, gamma, beta, rm, rv, dy, momentum, eps, dev)
    g = dy.double().reshape(-1) * (beta.double() > 0)
    want = dict(y=torch.relu(beta.double()).reshape(1, C_, 1), mean=x.double().reshape(-1), var=torch.zeros(C_, dtype=torch.float64),
                run_mean=(1 - momentum) * rm.double() + momentum * x.double().reshape(-1), run_var=(1 - momentum) * rv.double(),
                dbeta=g)
    for k, w in want.items():
        assert U.rel_err(got[k], w) <= U.RTOL, (k, got[k], w)
    assert int(torch.count_nonzero(got["var"])) == 0 and int(torch.count_nonzero(got["dgamma"])) == 0 and int(torch.count_nonzero(got["dx"])) == 0


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def check_adam(lib, dev, n=CLAMP + 1, steps=3):
    """Three steps past the grid clamp with weight decay and a gradient scale: the device-counter variant equals the host-step one
    bitwise after each step and its counter reads 1, 2, 3; both follow the float64 formula of csrc/ops_direct.h in p, m and v.  The
    hyper-parameters of the formula are the fp32 values the C ABI receives (1 - fp32(0.999) is 1.3e-5 off 1 - 0.999).  lr = 0.05 makes
    the parameter check a check of the step: RTOL of max |p| ~ 5 is 1 % of an update.  (The update on its own is not compared: where
    |g| ~ eps, m / (sqrt(v) + eps) amplifies the fp32 rounding of g = scale * grad + wd * p - among 2^20 elements a few always are.)"""
    lr, b1, b2, eps, wd, scale = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.05, 0.9, 0.999, 1e-8, 0.01, 0.5))
    g = _gen(67)
    p0 = torch.randn(n, generator=g)
    pa, ma, va = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb, mb, vb = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    worst = 0.0
    for t in range(1, steps + 1):
        grad = torch.randn(n, generator=g)
        lib.adam_step(pa, grad.to(dev), ma, va, lr, b1, b2, eps, wd, scale, t)
        lib.adam_step_counter(pb, grad.to(dev), mb, vb, lr, b1, b2, eps, wd, scale, counter)
        assert int(counter.item()) == t
        assert bits_equal(pa, pb) and bits_equal(ma, mb) and bits_equal(va, vb), f"step {t}: counter variant differs from the host-step one"
        gi = scale * grad.double() + wd * p64
        m64 = b1 * m64 + (1 - b1) * gi
        v64 = b2 * v64 + (1 - b2) * gi * gi
        p64 = p64 - (lr / (1 - b1 ** t)) * m64 / (v64.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        errs = (U.rel_err(pa, p64), U.rel_err(ma, m64), U.rel_err(va, v64))
        print(f"glue adam step {t}: p {errs[0]:.2e} m {errs[1]:.2e} v {errs[2]:.2e}")
        assert max(errs) <= U.RTOL, (t, errs)
        worst = max(worst, *errs)
    return worst
