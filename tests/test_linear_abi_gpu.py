"""mlhot_linear_fwd / mlhot_linear_bwd through their C ABI on the MI355X: every route of the dispatch (tests/linear_abi.py names them
per case), every stride, element offset, accumulate, null pointer and M == 0, against the float64 reference, with the sentinel check
around every window and the backward's launch labels (one `linear_bwd` = the combined launch, `linear_bwd.w` / `linear_bwd.x` = the
separate ones).  Run with -m gpu.  Worst errors on record: profiles/INDEX_linear_abi.md."""
import pytest

from tests import linear_abi as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("act", L.ACTS)
@pytest.mark.parametrize("c", L.CASES, ids=L.CASE_IDS)
def test_linear_abi_case(gpulib, c, act):
    L.check_case(gpulib, c, act, DEV, profile=True)


@pytest.mark.parametrize("act", L.ACTS)
@pytest.mark.parametrize("shape", L.PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_abi_aligned_vs_offset(gpulib, shape, act):
    """Skinny forward + combined backward against the generic kernels on the same data."""
    L.check_pair(gpulib, shape, act, DEV)
