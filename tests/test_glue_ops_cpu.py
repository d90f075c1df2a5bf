"""The glue kernels' functors in the host flavour of the library, called directly (tests/glue_ops.py has the cases, the inputs and
the references): the twin of tests/test_glue_ops_gpu.py - the same cases and assertions wherever the host flavour exports the entry.
It proves the functors' arithmetic and the references before the device run; the launch geometry is the device twin's."""
import pytest

from tests import glue_ops as G
from tests import util as U

DEV = "cpu"


@pytest.mark.parametrize("n", G.FOREACH_N)
def test_add_relu_bitwise(hostsim, n):
    """relu(a + b) and dy * (y > 0) have torch's fp32 bits, signed zeros and subnormal sums included."""
    G.need(hostsim, "mlhot_add_relu_fwd")
    G.check_add_relu(hostsim, n, DEV)


@pytest.mark.parametrize("with_a", [True, False], ids=["a", "no_a"])
@pytest.mark.parametrize("n", G.FOREACH_N)
def test_axpy_bitwise(hostsim, n, with_a):
    G.need(hostsim, "mlhot_axpy")
    G.check_axpy(hostsim, n, DEV, with_a)


@pytest.mark.parametrize("n", G.FOREACH_N)
def test_spatial_mean_foreach_sizes(hostsim, n):
    G.need(hostsim, "mlhot_spatial_mean_fwd")
    G.check_spatial_mean(hostsim, n, 1, DEV)


@pytest.mark.parametrize("planes,hw", G.MEAN_SHAPES)
def test_spatial_mean_shapes(hostsim, planes, hw):
    G.need(hostsim, "mlhot_spatial_mean_fwd")
    G.check_spatial_mean(hostsim, planes, hw, DEV)


@pytest.mark.parametrize("shape", G.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool2_ties_bitwise(hostsim, shape):
    """Values, ATen's first-maximum arg-max and the routed gradient on inputs that tie in most windows."""
    G.need(hostsim, "mlhot_pool2_fwd")
    G.check_pool2(hostsim, shape, DEV)


def test_pool2_refusals(hostsim):
    G.need(hostsim, "mlhot_pool2_fwd")
    G.check_pool2_refusals(hostsim, DEV)


@pytest.mark.parametrize("momentum", G.BN_MOMENTA)
@pytest.mark.parametrize("shape", G.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_vs_float64(hostsim, shape, momentum):
    G.need(hostsim, "mlhot_bn_relu_fwd")
    G.check_bn(hostsim, shape, momentum, DEV)


@pytest.mark.parametrize("shape", [(2, 3, 1), (5, 3, 51)], ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_without_running_stats(hostsim, shape):
    G.need(hostsim, "mlhot_bn_relu_fwd")
    G.check_bn(hostsim, shape, 0.1, DEV, running=False)


@pytest.mark.parametrize("momentum", G.BN_MOMENTA)
def test_bn_relu_count_one(hostsim, momentum):
    G.need(hostsim, "mlhot_bn_relu_fwd")
    G.check_bn_count1(hostsim, 5, momentum, DEV)


def test_adam_variants_past_the_grid_clamp(hostsim):
    G.need(hostsim, "mlhot_adam_step_counter")
    assert G.check_adam(hostsim, DEV) <= U.RTOL
