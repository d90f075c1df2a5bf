"""The glue kernels on the MI355X, called directly (tests/glue_ops.py has the cases, the inputs and the references): add_relu, axpy,
spatial_mean, pool2, bn_relu forward + backward, and the two Adam steps past run_foreach's grid clamp.  Run with -m gpu.  Worst errors
on record: profiles/INDEX_linear_abi.md."""
import pytest

from tests import glue_ops as G
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n", G.FOREACH_N)
def test_add_relu_bitwise(gpulib, n):
    """relu(a + b) and dy * (y > 0) have torch's fp32 bits, signed zeros and subnormal sums included."""
    G.check_add_relu(gpulib, n, DEV)


@pytest.mark.parametrize("with_a", [True, False], ids=["a", "no_a"])
@pytest.mark.parametrize("n", G.FOREACH_N)
def test_axpy_bitwise(gpulib, n, with_a):
    G.check_axpy(gpulib, n, DEV, with_a)


@pytest.mark.parametrize("n", G.FOREACH_N)
def test_spatial_mean_foreach_sizes(gpulib, n):
    G.check_spatial_mean(gpulib, n, 1, DEV)


@pytest.mark.parametrize("planes,hw", G.MEAN_SHAPES)
def test_spatial_mean_shapes(gpulib, planes, hw):
    G.check_spatial_mean(gpulib, planes, hw, DEV)


@pytest.mark.parametrize("shape", G.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool2_ties_bitwise(gpulib, shape):
    """Values, ATen's first-maximum arg-max and the routed gradient on inputs that tie in most windows."""
    G.check_pool2(gpulib, shape, DEV)


def test_pool2_refusals(gpulib):
    G.check_pool2_refusals(gpulib, DEV)


@pytest.mark.parametrize("momentum", G.BN_MOMENTA)
@pytest.mark.parametrize("shape", G.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_vs_float64(gpulib, shape, momentum):
    G.check_bn(gpulib, shape, momentum, DEV)


@pytest.mark.parametrize("shape", [(2, 3, 1), (5, 3, 51)], ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_without_running_stats(gpulib, shape):
    G.check_bn(gpulib, shape, 0.1, DEV, running=False)


@pytest.mark.parametrize("momentum", G.BN_MOMENTA)
def test_bn_relu_count_one(gpulib, momentum):
    G.check_bn_count1(gpulib, 5, momentum, DEV)


def test_adam_variants_past_the_grid_clamp(gpulib):
    assert G.check_adam(gpulib, DEV) <= U.RTOL
