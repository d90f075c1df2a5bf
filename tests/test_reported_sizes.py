"""The workspace sizes the library reports are part of its contract with every caller that allocates once and replays (the
trainer's captured graphs, the evaluator's buffers): literals recorded from the commit before the encoder's backward slabs got
one description (csrc/encoder.h enc_bwd_slabs), through the host build - the size arithmetic is host code, the same in both builds
(except mlhot_conv12_scratch_bytes: that block is GPU build only, the host build has always reported the 256-byte floor)."""
import ctypes as C

import pytest

NS = (1, 32, 33, 255, 256, 480)
# n -> (mlhot_enc_vanilla_scratch_bytes(n, 32), (n, 64), mlhot_enc_vanilla_saved_bytes(n), mlhot_conv12_scratch_bytes(n))
ENC = {
    1: (71811328, 71811328, 618816, 256),
    32: (90095872, 90095872, 19792192, 256),
    33: (90685696, 90685696, 20410688, 256),
    255: (221626624, 221626624, 157716800, 256),
    256: (222216448, 222216448, 158335296, 256),
    480: (354337024, 354337024, 296878400, 256),
}
# mlhot_np_dims (T, Nc, Nq, label_dim, y_dim, dim_w, dim_r, dim_z, hidden, dec_hidden, agg_mode, out_tanh, m_feat) -> mlhot_np_scratch_bytes
NP = {
    "cnp": ((16, 15, 15, 3, 2, 64, 128, 64, [100, 100], 100, "max", True, 0), 355058176),
    "anp": ((16, 15, 15, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 256), 357011968),
}


def reported(lib, n):
    c = lib.c
    return (c.mlhot_enc_vanilla_scratch_bytes(n, 32), c.mlhot_enc_vanilla_scratch_bytes(n, 64), c.mlhot_enc_vanilla_saved_bytes(n),
            c.mlhot_conv12_scratch_bytes(n))


def np_reported(lib, dims):
    return lib.c.mlhot_np_scratch_bytes(C.byref(lib.np_dims(*dims)))


@pytest.mark.parametrize("n", NS)
def test_encoder_sizes_are_what_they_were(hostsim, n):
    assert reported(hostsim, n) == ENC[n]


@pytest.mark.parametrize("kind", list(NP))
def test_whole_model_scratch_is_what_it_was(hostsim, kind):
    dims, want = NP[kind]
    assert np_reported(hostsim, dims) == want
