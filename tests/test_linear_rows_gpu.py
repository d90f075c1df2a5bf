"""mlhot_linear_rows_fwd and mlhot_loss_prefix_fwd on the MI355X: the row-invariance guarantee (the bits of an output row do not
depend on the row count, on the row's place in the launch or on its neighbours), tile edges, row maps, values, refusals; the
all-prefix loss against LossFunction per slice.  Run with -m gpu."""
import numpy as np
import pytest
import torch

from tests import linear_rows_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(4, 0, 2), (20, 0, 4), (16, 12, 17), (256, 0, 256), (2048, 0, 256), (256, 256, 65)]
ACTS = ["none", "relu", "tanh"]
M0 = 300
_cache = {}


def _layer(shape, rows=M0, seed=0):
    """(x0 [rows, K0], x1 [rows, K1] or None, w, b) on the device: x ~ N(0, 1), w ~ N(0, 1) / sqrt(K); built once per shape."""
    key = (shape, rows, seed)
    if key not in _cache:
        K0, K1, N = shape
        g = torch.Generator().manual_seed(1000 * seed + K0 + 7 * K1 + 13 * N)
        x0 = torch.randn(rows, K0, generator=g)
        x1 = torch.randn(rows, K1, generator=g) if K1 else None
        w = torch.randn(N, K0 + K1, generator=g) / (K0 + K1) ** 0.5
        b = torch.randn(N, generator=g)
        _cache[key] = tuple(t.to(DEV) if t is not None else None for t in (x0, x1, w, b))
    return _cache[key]


def _run(lib, x0, x1, w, b, act, **kw):
    srcs = [(x0, 1, 0)] + ([(x1, 1, 0)] if x1 is not None else [])
    return lib.linear_rows_fwd(srcs, w, b, act, **kw)


def _full(lib, shape, act):
    key = ("y", shape, act)
    if key not in _cache:
        _cache[key] = _run(lib, *_layer(shape), act)
    return _cache[key]


def _rows(t, sel):
    return None if t is None else t[sel].contiguous()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_invariance(gpulib, shape, act):
    """The same input row gives the same bits in a 300-row call, in 1-, 65- and 64-row calls, at another index (permutation) and
    among other rows (offset 37 of 1000 rows).  The permutation is also the measurement of the kernel's one assumption: an fp32 MFMA
    computes an output element the same way at every position of its tile."""
    x0, x1, w, b = _layer(shape)
    y = _full(gpulib, shape, act)
    assert y.shape == (M0, shape[2]) and bool(torch.isfinite(y).all())
    for lo, hi in ((0, 1), (299, 300), (17, 82), (64, 128)):
        part = _run(gpulib, _rows(x0, slice(lo, hi)), _rows(x1, slice(lo, hi)), w, b, act)
        assert torch.equal(part, y[lo:hi]), (lo, hi)
    perm = torch.randperm(M0, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(_run(gpulib, _rows(x0, perm), _rows(x1, perm), w, b, act), y[perm])
    g = torch.Generator().manual_seed(6)
    big0 = torch.randn(1000, shape[0], generator=g).to(DEV)
    big1 = torch.randn(1000, shape[1], generator=g).to(DEV) if shape[1] else None
    big0[37:37 + M0] = x0
    if big1 is not None:
        big1[37:37 + M0] = x1
    assert torch.equal(_run(gpulib, big0, big1, w, b, act)[37:37 + M0], y)


@pytest.mark.parametrize("shape", [(16, 12, 17), (256, 256, 65)], ids=lambda s: "x".join(map(str, s)))
def test_tile_edges_rows_and_columns(gpulib, shape):
    """M around the 16-row MFMA tiles and the 64-row workgroup tile: the first M rows of the 300-row result, and nothing written
    behind row M or behind column N of a wider output buffer."""
    x0, x1, w, b = _layer(shape)
    y = _full(gpulib, shape, "relu")
    N, pad, sentinel = shape[2], 7, -777.0
    for M in (1, 15, 17, 31, 33, 63, 65, 127, 129):
        out = torch.full((M + 64, N + pad), sentinel, device=DEV)
        got = _run(gpulib, _rows(x0, slice(0, M)), _rows(x1, slice(0, M)), w, b, "relu", out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out[:M, :N], y[:M]), M
        assert bool((out[M:] == sentinel).all()) and bool((out[:, N:] == sentinel).all()), M


@pytest.mark.parametrize("maps", [((1, 30), (5, 0)), ((1, 30), (1, 0)), ((5, 0), (1, 0))])
def test_row_maps_equal_the_materialised_rows(gpulib, maps):
    """Output row i reads source row (i // rep) % period: equal, bit for bit, to the call on the gathered rows."""
    K0, K1, N = 16, 12, 17
    _, _, w, b = _layer((K0, K1, N))
    g = torch.Generator().manual_seed(8)
    srcs = []
    for (rep, period), k in zip(maps, (K0, K1)):
        n = int(R.source_rows(M0, rep, period).max()) + 1
        assert n == (period if period else M0 // rep)
        srcs.append((torch.randn(n, k, generator=g).to(DEV), rep, period))
    got = gpulib.linear_rows_fwd(srcs, w, b, "tanh", rows=M0)
    flat = [(R.gather(x, M0, rep, period).contiguous(), 1, 0) for x, rep, period in srcs]
    assert flat[0][0].shape == (M0, K0) and flat[1][0].shape == (M0, K1)
    assert torch.equal(got, gpulib.linear_rows_fwd(flat, w, b, "tanh"))
    want = R.linear_rows_np([(x.cpu().numpy(), rep, period) for x, rep, period in srcs], w.cpu().numpy(), b.cpu().numpy(), "tanh", M0)
    assert U.rel_err(got, want) <= U.RTOL


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_against_float64(gpulib, shape):
    """Worst error against a float64 matmul of the same inputs, in units of the output's scale: the bar of every Linear parity test
    here; mlhot_linear_fwd's figure on the same inputs is printed next to it."""
    x0, x1, w, b = _layer(shape)
    y = _full(gpulib, shape, "none")
    srcs = [(x0.cpu().numpy(), 1, 0)] + ([(x1.cpu().numpy(), 1, 0)] if x1 is not None else [])
    want = R.linear_rows_np(srcs, w.cpu().numpy(), b.cpu().numpy(), "none", M0)
    x = torch.cat([x0, x1], dim=1) if x1 is not None else x0
    plain = gpulib.linear_fwd(x.contiguous(), w, b, "none")
    err, err_plain = U.rel_err(y, want), U.rel_err(plain, want)
    print(f"linear_rows {shape}: worst error {err:.2e} of the output's scale (mlhot_linear_fwd on the same inputs: {err_plain:.2e})")
    assert err <= U.RTOL


def test_unsupported_shapes_are_refused_and_write_nothing(gpulib):
    from mlhot.binding import MlhotError
    assert gpulib.linear_rows_supported(256, 256, 2) and gpulib.linear_rows_supported(4, 0, 1)
    assert not gpulib.linear_rows_supported(6, 0, 4) and not gpulib.linear_rows_supported(8, 6, 4) and not gpulib.linear_rows_supported(0, 8, 4)
    out = torch.full((40, 8), -777.0, device=DEV)
    with pytest.raises(MlhotError, match=r"code 4"):                      # MLHOT_ERR_UNSUPPORTED: K0 = 6
        gpulib.linear_rows_fwd([(torch.randn(40, 6, device=DEV), 1, 0)], torch.randn(8, 6, device=DEV), None, "none", out=out)
    flat = torch.randn(40 * 8 + 4, device=DEV)
    shifted = flat[1:1 + 40 * 8].view(40, 8)                              # rows start 4 bytes off a 16-byte boundary
    assert shifted.data_ptr() % 16 == 4
    with pytest.raises(MlhotError, match=r"code 4"):
        gpulib.linear_rows_fwd([(shifted, 1, 0)], torch.randn(8, 8, device=DEV), None, "none", out=out)
    torch.cuda.synchronize()
    assert bool((out == -777.0).all())
    with pytest.raises(MlhotError, match="source rows"):                  # the binding never lets a row map run past its source
        gpulib.linear_rows_fwd([(torch.randn(10, 8, device=DEV), 1, 0)], torch.randn(8, 8, device=DEV), None, "none", rows=11)


def _loss_inputs(kind, P, rows, seed):
    g = torch.Generator().manual_seed(seed)
    y_dim, gt_dim = {"azimuth": (2, 3), "degree": (2, 3), "mse": (2, 2), "quaternion": (4, 4), "distractor": (2, 2)}[kind]
    mu = torch.randn(P, rows, y_dim, generator=g)
    if kind == "degree":                                                  # (cos, sin) of an angle: acos needs |mu0| <= 1
        ang = torch.rand(P, rows, generator=g) * 6.28
        mu = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1) * 0.999
    gt = torch.randn(rows, gt_dim, generator=g)
    return mu.to(DEV), gt.to(DEV)


@pytest.mark.parametrize("rows", [1, 7, 600])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("kind", ["azimuth", "mse", "quaternion", "degree", "distractor"])
def test_loss_prefixes_equal_the_loss_per_slice(gpulib, kind, P, rows):
    from mlhot.ops import LossFunction, loss_prefixes
    mu, gt = _loss_inputs(kind, P, rows, seed=rows + P)
    got = loss_prefixes(kind, mu, gt)
    want = torch.stack([LossFunction.apply(kind, mu[p], gt).view(()) for p in range(P)])
    assert got.shape == (P,) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want), (got, want)


def test_loss_prefixes_reduce_like_the_loss_over_several_passes_of_the_block(gpulib):
    """5000 rows: more than the 4096 a workgroup takes per trip, so both of the reduction's loops run."""
    from mlhot.ops import LossFunction, loss_prefixes
    mu, gt = _loss_inputs("quaternion", 2, 5000, seed=3)
    assert torch.equal(loss_prefixes("quaternion", mu, gt), torch.stack([LossFunction.apply("quaternion", mu[p], gt).view(()) for p in range(2)]))
