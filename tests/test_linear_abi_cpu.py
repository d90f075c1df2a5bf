"""mlhot_linear_fwd / mlhot_linear_bwd through their C ABI on the host flavour of the library: the whole case table of
tests/linear_abi.py (strides, element offsets, accumulate, null pointers, M == 0) against the float64 reference, with the sentinel
check around every window.  The host flavour takes the generic chain on every leg; what this file proves is the generic functors'
index arithmetic and - before the device run - the caller, the sentinel check and the reference themselves."""
import pytest

from tests import linear_abi as L


@pytest.mark.parametrize("act", L.ACTS)
@pytest.mark.parametrize("c", L.CASES, ids=L.CASE_IDS)
def test_linear_abi_case(hostsim, c, act):
    L.check_case(hostsim, c, act, "cpu")


@pytest.mark.parametrize("act", L.ACTS)
@pytest.mark.parametrize("shape", L.PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_abi_aligned_vs_offset(hostsim, shape, act):
    L.check_pair(hostsim, shape, act, "cpu")


def test_sentinel_check_sees_a_stray_write(hostsim):
    """The helper's own check: one element changed behind the window's last column, in the spare rows, or in front of the offset
    turns `outside_unchanged` false; a write inside the window does not."""
    for where in ("pad", "row", "front"):
        op = L._Operand(5, 6, 8, 1, 7, "cpu")
        assert op.outside_unchanged()
        op.buf[op.off + 2 * op.ld + 3] = 1.0                     # inside the window
        assert op.outside_unchanged()
        op.buf[{"pad": op.off + 2 * op.ld + 6, "row": op.off + 5 * op.ld, "front": 0}[where]] = 1.0
        assert not op.outside_unchanged(), where
