"""tests/enc_cases.py on the host flavour of the library: the generic chain (all that flavour has; it ignores the options) at every
case of <= 65 images and one of 241, held to the float64 reference at the device's tolerances.  It proves without a GPU that the case
table, the input generator and the float64 reference agree with an independent fp32 implementation, and that the INPUTS meet the flip
condition (at most max(1, FLIP_RATE x decisions) routing decisions on a tie fall the other way, each proven a util.TIE tie).  The
kernels' own edges (el::RCH, the 16-row tiles, conv12_grid, C2_GRID, conv3_nw) are the device twin's: tests/test_enc_envelope_gpu.py."""
import pytest

from tests import enc_cases as EC

DEV = "cpu"


def test_table_holds_every_edge():
    """Asserted over the table, so that a later edit cannot silently drop an edge."""
    one = {c.n0 for c in EC.CASES if c.name.startswith("default") and c.n1 == 0}
    assert one == {15, 16, 17, 31, 32, 33, 127, 128, 129, 239, 240, 241, 255, 256, 257, 479, 481}
    two = {(c.n0, c.n1) for c in EC.CASES if c.name.startswith("default") and c.n1}
    assert two == {(15, 1), (16, 16), (17, 15), (239, 2), (240, 1), (1, 240), (200, 57), (256, 1)}
    merged = {(c.n0, c.opts["conv3_bwd_merged"]) for c in EC.CASES if c.name.startswith("merged")}
    assert merged == {(n, m) for n in (256, 257) for m in (0, 1, 64, 2, 255)}
    assert all(c.bwd_labels is not None for c in EC.CASES if c.name.startswith(("merged", "default")))
    assert {c.n0 for c in EC.CASES if c.opts == {"conv2_split": 7}} == {33, 241}
    assert {c.n0 for c in EC.CASES if c.opts == {"conv2_tc": 0}} == {3, 4, 63, 64, 65, 513}
    assert {(c.n0, c.dim_w) for c in EC.CASES if c.dim_w != 64} == {(65, 32), (17, 128)}
    assert all(c.n0 + c.n1 <= 65 or c.name == "default-n241" for c in (EC.BY_NAME[k] for k in EC.CPU_CASES))


@pytest.mark.parametrize("name", EC.CPU_CASES)
def test_inputs(name):
    """Image 0 is all zero, image 1 all one, the last one random; dfeat has a row per image."""
    case = EC.BY_NAME[name]
    p, x, df = EC.inputs(case)
    n = case.n0 + case.n1
    assert x.shape == (n, 1, 128, 128) and df.shape == (n, case.dim_w) and p["encoder_w0.8.weight"].shape == (case.dim_w, 4096)
    assert float(x[0].abs().max()) == 0.0 and float((x[1] - 1).abs().max()) == 0.0
    assert float(x[n - 1].std()) > 0.25 and float(df[n - 1].abs().max()) > 0.5


@pytest.mark.parametrize("name", EC.CPU_CASES)
def test_encoder_vs_float64(hostsim, name):
    EC.check_encoder(hostsim, EC.BY_NAME[name], DEV)
