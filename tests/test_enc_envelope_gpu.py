"""The vanilla image encoder on the MI355X at every image count where one of its kernels changes what it does (tests/enc_cases.py has
the cases, the inputs and the float64 reference): features, saved p2 / a3, pool arg-max and all eight gradients, and for the cases that
name one the backward's launch sequence.  Run with -m gpu.  Worst errors on record: profiles/INDEX_enc_envelope.md."""
import pytest

from tests import enc_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", [c.name for c in EC.CASES])
def test_encoder_vs_float64(gpulib, name):
    EC.check_encoder(gpulib, EC.BY_NAME[name], DEV)
