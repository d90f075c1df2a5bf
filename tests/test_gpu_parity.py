"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle and the golden
vectors of the reference.  Run on the MI355X box:  pytest tests -m gpu"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import split_cases as SC
from tests.autograd_cases import _bbb_ref, _chain_reference, _trunk_weights
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


# ---- igemm engine on plain GEMM shapes (MFMA lane maps, LDS images, split-K slab) --------------
@pytest.mark.parametrize("M,K,N", [(1, 3, 16), (37, 80, 100), (240, 100, 64), (480, 512, 64), (65, 17, 130), (16, 4096, 64),
                                   (4100, 96, 250)])     # the last one: >= 128 64-row tiles, the 64 x 64 x 32 tile variant
@pytest.mark.parametrize("act", ["none", "relu", "tanh"])
def test_linear_fwd_bwd(gpulib, M, K, N, act):
    g = torch.Generator().manual_seed(M * 1000 + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = {"none": lambda t: t, "relu": torch.relu, "tanh": torch.tanh}[act](F.linear(xr, wr, br))
    yr.backward(dy)
    xd, wd, bd, dyd = dev(x, w, b, dy)
    y = gpulib.linear_fwd(xd, wd, bd, act)
    dx, dw, db = gpulib.linear_bwd(xd, wd, y, dyd, act)
    assert U.rel_err(y, yr) <= U.RTOL
    assert U.rel_err(dx, xr.grad) <= U.RTOL
    assert U.rel_err(dw, wr.grad) <= U.RTOL
    assert U.rel_err(db, br.grad) <= U.RTOL


def test_linear_asymmetric_identity(gpulib):
    """A = I with an asymmetric B catches a transposed C/D lane map (cdna guide §3)."""
    n = 48
    x = torch.eye(n)
    w = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 97) / 7.0
    y = gpulib.linear_fwd(x.to(DEV), w.to(DEV), None, "none")
    assert torch.equal(y.cpu(), w.t())


@pytest.mark.parametrize("M,Ka,Kb,N,act", [(120, 256, 4, 256, "relu"), (120, 256, 256, 256, "relu"), (7, 256, 16, 256, "none"), (240, 64, 16, 100, "tanh")])
@pytest.mark.parametrize("grads", [(True, False), (True, True), (False, True)], ids=["dxa", "dxa_dxb", "dxb"])
def test_two_source_linear_vs_autograd(gpulib, M, Ka, Kb, N, act, grads):
    """Linear2Function: act(cat([xa, xb], -1) W^T + b) with the concatenation folded into the few-row Linear kernels (the reference's
    torch.cat([x_ctx, labels]) -> task_encoder[0], ANP.py:113; torch.cat([x, sample_features]) -> fc_mu[0], models.py:182): output,
    both input gradients (each optional), dW and db against torch autograd of the concatenated form."""
    from mlhot.ops import Linear2Function, linear2_ok
    g = torch.Generator().manual_seed(M + Ka + Kb)
    xa, xb = torch.randn(2, M // 2 if M % 2 == 0 else M, Ka, generator=g)[:1 if M % 2 else 2], None
    xa = torch.randn(M, Ka, generator=g)
    xb = torch.randn(M, Kb, generator=g)
    w, b = torch.randn(N, Ka + Kb, generator=g) * (Ka + Kb) ** -0.5, torch.randn(N, generator=g) * 0.1
    dy = torch.randn(M, N, generator=g)
    ar, br, wr, bbr = xa.clone().requires_grad_(grads[0]), xb.clone().requires_grad_(grads[1]), w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = F.linear(torch.cat([ar, br], -1), wr, bbr)
    yr = torch.relu(yr) if act == "relu" else torch.tanh(yr) if act == "tanh" else yr
    yr.backward(dy)
    ad, bd = xa.clone().to(DEV).requires_grad_(grads[0]), xb.clone().to(DEV).requires_grad_(grads[1])
    wd, bbd = w.clone().to(DEV).requires_grad_(), b.clone().to(DEV).requires_grad_()
    assert linear2_ok(ad, bd, wd)
    y = Linear2Function.apply(ad, bd, wd, bbd, act)
    y.backward(dy.to(DEV))
    assert U.rel_err(y, yr) <= U.RTOL
    assert U.rel_err(wd.grad, wr.grad) <= U.RTOL and U.rel_err(bbd.grad, bbr.grad) <= U.RTOL
    if grads[0]:
        assert U.rel_err(ad.grad, ar.grad) <= U.RTOL
    else:
        assert ad.grad is None
    if grads[1]:
        assert U.rel_err(bd.grad, br.grad) <= U.RTOL
    else:
        assert bd.grad is None


@pytest.mark.parametrize("M", [120, 7, 240, 16])
@pytest.mark.parametrize("case", ["task_encoder", "decoder_head", "one_layer", "tanh_no_bias"])
def test_mlp_chain_fwd_bwd_vs_autograd(gpulib, M, case):
    """csrc/mlp_chain.h: chains of few-row Linear layers in one launch (two for the backward) against torch autograd of the same
    layers with the reference's torch.cat in front (ANP.py:113 cat([x_ctx, labels]) -> task_encoder; ANP.py:128 mu, models.py:182-184
    cat([x, sample_features]) -> fc_mu): outputs, the input's, the sides' and every weight / bias gradient at 1e-4."""
    from mlhot.ops import mlp_chain
    g = torch.Generator().manual_seed(M + len(case))

    def lin(n, k, bias=True):
        return torch.randn(n, k, generator=g) * k ** -0.5, (torch.randn(n, generator=g) * 0.1 if bias else None)
    if case == "task_encoder":
        x0, side = torch.randn(M, 256, generator=g), torch.randn(M, 4, generator=g)
        spec = [(*lin(256, 260), "relu", side, False), (*lin(256, 256), "relu", None, False), (*lin(256, 256), "relu", None, False)]
    elif case == "decoder_head":
        x0, side = torch.randn(M, 256, generator=g), torch.randn(M, 256, generator=g)
        spec = [(*lin(256, 256), "none", None, False), (*lin(256, 512), "relu", side, True), (*lin(256, 256), "relu", None, False),
                (*lin(4, 256), "none", None, False)]
    elif case == "one_layer":
        x0, side = torch.randn(M, 272, generator=g), None
        spec = [(*lin(100, 272), "relu", None, False)]
    else:
        x0, side = torch.randn(M, 64, generator=g), torch.randn(M, 16, generator=g)
        spec = [(*lin(128, 80, bias=False), "tanh", side, True), (*lin(2, 128), "tanh", None, False)]
    leaves = []

    def leaf(t, dev):
        if t is None:
            return None
        t = t.clone().to(dev).requires_grad_()
        leaves.append(t)
        return t
    res = {}
    for dev in ("cpu", DEV):
        del leaves[:]
        x = leaf(x0, dev)
        sd = leaf(side, dev)
        layers = [(leaf(w, dev), leaf(b, dev), act, sd if sdx is not None else None, sf) for w, b, act, sdx, sf in spec]
        y = _chain_reference(x, layers) if dev == "cpu" else mlp_chain(x, layers)
        assert y is not None
        wout = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(dev)
        (y * wout).sum().backward()
        res[dev] = (y.detach().cpu(), [t.grad.detach().cpu() for t in leaves])
    assert U.rel_err(res[DEV][0], res["cpu"][0]) <= U.RTOL
    for i, (a, b) in enumerate(zip(res[DEV][1], res["cpu"][1])):
        assert a.shape == b.shape and U.rel_err(a, b) <= U.RTOL, (case, M, i)


def test_mlp_chain_refuses_shapes_outside_its_limits(gpulib):
    from mlhot.ops import mlp_chain
    x = torch.randn(600, 256, device=DEV)
    w, b = torch.randn(256, 256, device=DEV), torch.randn(256, device=DEV)
    assert mlp_chain(x, [(w, b, "relu", None, False)]) is None                      # > 512 rows: the caller runs the layers one by one
    assert mlp_chain(x[:8], [(torch.randn(300, 256, device=DEV), None, "relu", None, False)]) is None    # > 256 outputs
    assert mlp_chain(x[:8], [(w, b, "relu", None, False)] * 5) is None              # > 4 layers


@pytest.mark.parametrize("rows", [(120, 120, 120), (56, 184, 56), (1, 30, 1)])
def test_head_stacks_in_one_launch_vs_autograd(gpulib, rows):
    """mlhot_linear_multi_fwd / _bwd: the query / key / value head stacks (8 x Linear(256, 256) each, ANP.py:80-93) as three
    Linear(256 -> 2048) jobs of ONE launch per direction, against torch autograd of the 24 separate layers."""
    from mlhot.ops import HeadStacksFunction
    g = torch.Generator().manual_seed(sum(rows))
    H, h = 8, 256
    xs = [torch.randn(1, m, h, generator=g) for m in rows]
    ws = [torch.randn(H * h, h, generator=g) * h ** -0.5 for _ in rows]
    bs = [torch.randn(H * h, generator=g) * 0.1 for _ in rows]
    douts = [torch.randn(1, m, H, h, generator=g) for m in rows]
    # reference: per-head layers, stacked on a head axis
    xr, wr, br = [[t.clone().requires_grad_() for t in ts] for ts in (xs, ws, bs)]
    for x, w, b, do in zip(xr, wr, br, douts):
        (F.linear(x, w, b).view(1, -1, H, h) * do).sum().backward()
    xd = [t.clone().to(DEV).requires_grad_() for t in xs]
    wd, bd = [t.to(DEV) for t in ws], [t.to(DEV) for t in bs]
    heads = [[wd[i].view(H, h, h)[k].clone().requires_grad_() for k in range(H)] + [bd[i].view(H, h)[k].clone().requires_grad_() for k in range(H)]
             for i in range(3)]
    args = [t for i in range(3) for t in (xd[i], wd[i], bd[i])]
    outs = HeadStacksFunction.apply(H, 3, *args, *[p for hp in heads for p in hp])
    sum((o * do.to(DEV)).sum() for o, do in zip(outs, douts)).backward()
    for i in range(3):
        assert U.rel_err(outs[i], F.linear(xs[i], ws[i], bs[i]).view(1, -1, H, h)) <= U.RTOL
        assert U.rel_err(xd[i].grad, xr[i].grad) <= U.RTOL
        assert U.rel_err(torch.cat([p.grad for p in heads[i][:H]]), wr[i].grad) <= U.RTOL
        assert U.rel_err(torch.cat([p.grad for p in heads[i][H:]]), br[i].grad) <= U.RTOL


@pytest.mark.parametrize("mode", ["mean", "max", "baco"])
@pytest.mark.parametrize("T,Nc,R", [(3, 7, 100), (16, 15, 64), (1, 1, 256), (2, 25, 100)])
def test_agg_fwd_bwd(gpulib, mode, T, Nc, R):
    g = torch.Generator().manual_seed(T + Nc + R)
    rs, lv, dr = torch.randn(T, Nc, R, generator=g), torch.randn(T, Nc, R, generator=g) * 2, torch.randn(T, R, generator=g)
    rr, ll = rs.clone().requires_grad_(), lv.clone().requires_grad_()
    ro = O.agg_mean(rr) if mode == "mean" else O.agg_max(rr) if mode == "max" else O.agg_baco(rr, 1e-5 + F.softplus(ll))[0]
    ro.backward(dr)
    rsd, lvd, drd = dev(rs, lv if mode == "baco" else None, dr)
    r, sigma, amax = gpulib.agg_fwd(mode, rsd, lvd)
    drs, dlv = gpulib.agg_bwd(mode, rsd, lvd, r, sigma, amax, drd)
    assert U.rel_err(r, ro) <= U.RTOL
    assert U.rel_err(drs, rr.grad) <= U.RTOL
    if mode == "baco":
        assert U.rel_err(dlv, ll.grad) <= U.RTOL


@pytest.fixture(params=[1, 0], ids=["favor_two_launch", "favor_chain"])
def favor_impl(gpulib, request):
    """FAVOR+ as two launches per direction (csrc/favor2.h, up to 32 + 32 shots) and as favor.h's operator chain."""
    gpulib.set_option("favor2", request.param)
    yield request.param
    gpulib.set_option("favor2", 1)


def test_favor_against_reference_vectors(gpulib, favor_impl):
    fx = np.load(os.path.join(U.GOLDEN, "favor.npz"))
    meta = json.loads(str(fx["meta"]))
    for tag, mt in meta.items():
        proj = torch.from_numpy(fx[f"{tag}/proj"])
        q, k, v, wout = (torch.from_numpy(fx[f"{tag}/{n}"]) for n in ("q", "k", "v", "wout"))
        T, H, Nq, d = q.shape
        qn, kn, vn = (t.permute(0, 2, 1, 3).contiguous().to(DEV) for t in (q, k, v))
        out, ws = gpulib.favor_fwd(qn, kn, vn, proj.to(DEV))
        assert U.rel_err(out.view(T, Nq, d, H).permute(0, 3, 1, 2), fx[f"{tag}/out"]) <= U.RTOL, tag
        dout = wout.permute(0, 2, 3, 1).reshape(T, Nq, d * H).contiguous().to(DEV)
        dq, dk, dv = gpulib.favor_bwd(qn, kn, vn, proj.to(DEV), out, dout, ws)
        for n, gt in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert U.rel_err(gt.permute(0, 2, 1, 3), fx[f"{tag}/{n}"], floor=1e-12) <= U.RTOL, (tag, n)


@pytest.mark.parametrize("staged", [False, True], ids=["plain", "staged_world1"])
def test_favor_at_the_shipped_c5_shape_with_live_gradients(gpulib, favor_impl, staged):
    """FAVOR+ at ANPMRShapeNet3D's own shape (T = 2, 8 heads, d = 256, m = 1419; 15 + 15 and the ragged 7 + 23)
    against vectors the reference generated (tests/golden/make_fixtures.py::run_favor_c5_cases), with inputs whose features sit
    ~50x above the +1e-4 floor so that dq / dk are 0.4-0.6 of dv's scale: out / dq / dk / dv each at 1e-4 of ITS OWN scale, no
    floor, for favor2.h, favor.h's chain and - world of one - both through the staged entry points."""
    from mlhot.dist import StabiliserExchange
    fx = np.load(os.path.join(U.GOLDEN, "favor_c5.npz"))
    meta = json.loads(str(fx["meta"]))
    proj = torch.from_numpy(fx["proj"]).to(DEV)
    for tag, mt in meta.items():
        q, k, v, wout = (torch.from_numpy(fx[f"{tag}/{n}"]) for n in ("q", "k", "v", "wout"))
        T, H, Nq, d = q.shape
        assert (H, d, proj.shape[0]) == (8, 256, 1419)
        qn, kn, vn = (t.permute(0, 2, 1, 3).contiguous().to(DEV) for t in (q, k, v))
        ex = (StabiliserExchange(), torch.zeros(4, device=DEV)) if staged else None
        out, ws = gpulib.favor_fwd(qn, kn, vn, proj, exchange=ex)
        e = {"out": U.rel_err(out.view(T, Nq, d, H).permute(0, 3, 1, 2), fx[f"{tag}/out"])}
        dout = wout.permute(0, 2, 3, 1).reshape(T, Nq, d * H).contiguous().to(DEV)
        dq, dk, dv = gpulib.favor_bwd(qn, kn, vn, proj, out, dout, ws, exchange=ex)
        for n, gt in (("dq", dq), ("dk", dk), ("dv", dv)):
            e[n] = U.rel_err(gt.permute(0, 2, 1, 3), fx[f"{tag}/{n}"])
        print(f"favor_c5 {tag} impl={favor_impl} staged={staged}: " + " ".join(f"{n}={x:.2e}" for n, x in e.items()))
        assert max(e.values()) <= U.RTOL, (tag, e)
        if staged:
            assert list(ex[0].calls) == ["fwd", "bwd"]


def test_losses_against_reference_vectors(gpulib):
    fx = np.load(os.path.join(U.GOLDEN, "losses.npz"))
    for kind, tag, key, task in (("azimuth", "az", "train", "shapenet_1d"), ("degree", "az", "test", "shapenet_1d"),
                                 ("mse", "pas", "train", "pascal_1d"), ("quaternion", "quat", "train", "shapenet_3d"),
                                 ("distractor", "dis", "train", "distractor")):
        pr, gt = torch.from_numpy(fx[f"{tag}/pr"]), torch.from_numpy(fx[f"{tag}/gt"])
        loss = gpulib.loss_fwd(kind, pr.to(DEV), gt.to(DEV)).item()
        want = float(fx[f"{tag}/{key}"])
        assert abs(loss - want) <= 1e-5 * max(1.0, abs(want)), kind
        if kind != "degree":
            pro = pr.clone().requires_grad_()
            O.calc_loss(task, pro, gt).backward()
            dmu = gpulib.loss_bwd(kind, pr.to(DEV), gt.to(DEV), torch.tensor(1.0, device=DEV))
            assert U.rel_err(dmu, pro.grad) <= U.RTOL, kind


def test_objective_inside_the_loss_launches_has_the_bits_of_loss_plus_kl_beta(gpulib):
    """mlhot_loss_plus_fwd / _bwd (ABI 7): the trainer's `losses = loss + kl * beta` (trainer/model_trainer.py:77-78) inside the loss's own
    launches.  For every training loss kind on the reference's vectors: the total, d mu and d kl have the BITS of mlhot_loss_fwd +
    mlhot_axpy (and so of the reference's two torch operators: product and sum rounded separately), for several (kl, beta, upstream)
    triples; through autograd (LossFunc.calc_objective) the gradients equal those of `add_scaled(calc_loss(...), kl, beta)`."""
    from mlhot.ops import add_scaled
    from trainer.losses import LossFunc
    fx = np.load(os.path.join(U.GOLDEN, "losses.npz"))
    rs = np.random.RandomState(3)
    for kind, tag, task in (("azimuth", "az", "shapenet_1d"), ("mse", "pas", "pascal_1d"), ("quaternion", "quat", "shapenet_3d"),
                            ("distractor", "dis", "distractor")):
        pr, gt = torch.from_numpy(fx[f"{tag}/pr"]).to(DEV), torch.from_numpy(fx[f"{tag}/gt"]).to(DEV)
        for kl_v, beta, up_v in ((1383162.5, 1e-7, 1.0), (float(rs.rand() * 1e4), float(rs.rand()), float(rs.randn())), (3.0, 0.5, -2.25)):
            kl, up = torch.tensor(kl_v, device=DEV), torch.tensor(up_v, device=DEV)
            total = gpulib.loss_plus_fwd(kind, pr, gt, kl, beta)
            want = gpulib.axpy(gpulib.loss_fwd(kind, pr, gt), kl, beta)
            assert torch.equal(total, want), (kind, kl_v, beta)
            assert total.item() == np.float32(np.float32(gpulib.loss_fwd(kind, pr, gt).item()) + np.float32(np.float32(beta) * np.float32(kl_v)))
            dmu, dkl = gpulib.loss_plus_bwd(kind, pr, gt, up, beta)
            assert torch.equal(dmu, gpulib.loss_bwd(kind, pr, gt, up)) and torch.equal(dkl, gpulib.axpy(None, up, beta)), (kind, kl_v, beta)
            assert gpulib.loss_plus_bwd(kind, pr, gt, up, beta, need_dx=False)[1] is None
        # through autograd, as trainer.ModelTrainer._objective calls it
        lf = LossFunc("mse", task)
        grads = []
        for fused in (True, False):
            mu, kl = pr.clone().requires_grad_(), torch.tensor(12.5, device=DEV, requires_grad=True)
            obj = lf.calc_objective(mu, None, gt, kl * 1.0, 0.25) if fused else add_scaled(lf.calc_loss(mu, None, gt), kl * 1.0, 0.25)
            assert (type(obj.grad_fn).__name__ == "LossPlusFunctionBackward") == fused
            obj.backward()
            grads.append((obj.detach().clone(), mu.grad.clone(), kl.grad.clone()))
        for a, b in zip(*grads):
            assert torch.equal(a, b), kind
        assert lf.calc_objective(pr, None, gt, 0, 0.25).grad_fn is None and torch.equal(lf.calc_objective(pr, None, gt, 0, 0.25), lf.calc_loss(pr, None, gt))


# ---- E1 encoder vs oracle -----------------------------------------------------------------------
def _enc_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [("0.weight", (32, 1, 3, 3), 0.3), ("0.bias", (32,), 0.1), ("2.weight", (48, 32, 3, 3), 0.06), ("2.bias", (48,), 0.1),
              ("5.weight", (64, 48, 3, 3), 0.05), ("5.bias", (64,), 0.1), ("8.weight", (64, 4096), 0.02), ("8.bias", (64,), 0.1)]
    return {"encoder_w0." + k: torch.randn(*s, generator=g) * a for k, s, a in shapes}


@pytest.fixture(params=[(1, 0), (0, 0), (1, 1), (1, 7)], ids=["conv2_tc", "conv2_igemm", "conv2_split", "conv2_split_all"])
def conv2_impl(gpulib, request):
    """The implementations of the conv2 rows: the weight-stationary fp32 kernels (csrc/conv_tc.h), the generic implicit-GEMM
    problems, and the opt-in kernels with conv2 on the bf16 pipe over hi / mid / lo split operands (csrc/conv_split.h: held to
    the SAME tolerances as the fp32 kernels - the split is exact, the six kept piece products are as exact as an fp32 MFMA):
    the forward alone, or the forward and both gradients (option bits 1 | 2 | 4)."""
    gpulib.set_option("conv2_tc", request.param[0])
    gpulib.set_option("conv2_split", request.param[1])
    yield request.param
    gpulib.set_option("conv2_tc", 1)
    gpulib.set_option("conv2_split", 0)


@pytest.mark.parametrize("n0,n1", [(1, 0), (3, 2), (8, 9), (40, 0)])
def test_encoder_fwd_bwd_vs_oracle(gpulib, conv2_impl, n0, n1):
    p = _enc_params()
    g = torch.Generator().manual_seed(n0 * 10 + n1)
    x0, x1 = torch.rand(n0, 1, 128, 128, generator=g), torch.rand(n1, 1, 128, 128, generator=g)
    df = torch.randn(n0 + n1, 64, generator=g)
    pr = {k: v.clone().requires_grad_() for k, v in p.items()}
    taps = {}
    fr = O.vanilla_encoder(torch.cat([x0, x1]), pr, taps=taps)
    fr.backward(df)
    plist = [t.to(DEV) for t in p.values()]
    f0, f1, saved = gpulib.enc_vanilla_fwd(x0.to(DEV), x1.to(DEV) if n1 else None, plist, 64)
    assert U.rel_err(torch.cat([f0, f1]), fr) <= U.RTOL
    grads = gpulib.enc_vanilla_bwd(x0.to(DEV), x1.to(DEV) if n1 else None, plist, 64, df[:n0].contiguous().to(DEV),
                                   df[n0:].contiguous().to(DEV), saved)
    for (k, ref), got in zip(pr.items(), grads):
        assert U.rel_err(got, ref.grad) <= U.RTOL, k


@pytest.mark.parametrize("split", [0, 1, 7], ids=["fp32", "split", "split_all"])
def test_encoder_full_size_gradients_with_pinned_routing(gpulib, split):
    """480 images (the c2/c3 batch).  ReLU / max-pool routing is discontinuous, so gradients are
    compared with the oracle evaluated under the KERNEL's routing decisions (see
    oracle.ref_cpu.vanilla_encoder_routed); the decisions themselves must match the oracle's except
    where the oracle's own pre-activation is a rounding-level tie."""
    n = 480
    p = _enc_params(3)
    g = torch.Generator().manual_seed(480)
    x = torch.rand(n, 1, 128, 128, generator=g)
    df = torch.randn(n, 64, generator=g)
    plist = [t.to(DEV) for t in p.values()]
    xd = x.to(DEV)
    gpulib.set_option("materialize_a1", 1)      # the fused conv1+conv2 kernels never store a1; keep it for this check
    gpulib.set_option("conv2_split", split)     # bits: 1 forward, 2 data gradient, 4 weight gradient on the bf16 pipe (csrc/conv_split.h)
    try:
        f0, _, saved = gpulib.enc_vanilla_fwd(xd, None, plist, 64)
        gpulib.set_option("materialize_a1", 0)
        grads = gpulib.enc_vanilla_bwd(xd, None, plist, 64, df.to(DEV), torch.empty(0, 64, device=DEV), saved)
    finally:
        gpulib.set_option("materialize_a1", 0)
        gpulib.set_option("conv2_split", 0)
    a1, p2, am2, a3 = (t.cpu() for t in gpulib.enc_saved_views(saved, n))
    pr = {k: v.clone().requires_grad_() for k, v in p.items()}
    fr, pre = O.vanilla_encoder_routed(x, pr, (a1 > 0).float(), am2, (p2 > 0).float(), (a3 > 0).float())
    assert U.rel_err(f0, fr) <= 1e-5
    # routing decisions: any disagreement must sit on a rounding-level tie of the oracle's values
    tie = 1e-5
    bad1 = ((a1 > 0) != (pre["y1"] > 0)) & (pre["y1"].abs() > tie * pre["y1"].abs().max())
    bad3 = ((a3 > 0) != (pre["y3"] > 0)) & (pre["y3"].abs() > tie * pre["y3"].abs().max())
    win = torch.relu(pre["y2win"].detach())     # the pool runs on the post-ReLU map
    chosen = torch.gather(win, 4, am2.long().unsqueeze(-1)).squeeze(-1)
    bad2 = (win.max(dim=4).values - chosen) > tie * win.abs().max()
    assert int(bad1.sum()) == 0 and int(bad2.sum()) == 0 and int(bad3.sum()) == 0
    fr.backward(df)
    for (k, ref), got in zip(pr.items(), grads):
        assert U.rel_err(got, ref.grad) <= 2e-5, k


# ---- whole model through the plugin boundary vs the reference's golden vectors -------------------
# Outputs and loss are held to 1e-4 against the reference's vectors.  Gradients: ReLU / max-pool routing is discontinuous, and
# at the full c2 / c3 size (16 tasks x 30 images = 63 M routing decisions) a handful of rounding-level ties route differently
# in ANY two fp32 evaluation orders, each moving a conv gradient by ~1e-4 of its scale.  So every gradient is compared at 1e-4
# with the oracle evaluated under the KERNELS' OWN routing decisions (conv1 sign bits, pool arg-max, ReLU masks of every layer,
# arg-max of the max aggregator - read back from the forward's saved buffers), every decision that differs from the oracle's own
# is proven to sit on a <= 1e-5 tie of the oracle's pre-activations, and when no decision differs the reference's own gradients
# (the fixture) are compared at 1e-4 as well.
def _vanilla_routes(gpulib, taps, T, Nc, Nq, agg):
    kind, dims, saved = taps[-1]
    assert kind == "np"
    v = gpulib.np_saved_views(saved, dims)
    Rc = T * Nc
    enc = gpulib.enc_routes(saved, v["n"])
    routes = {"enc_qry": tuple(t[Rc:] for t in enc), "d": [(v["d1"] > 0).float().cpu().view(T, Nq, -1), (v["d2"] > 0).float().cpu().view(T, Nq, -1)]}
    if Nc:
        routes["enc_ctx"] = tuple(t[:Rc] for t in enc)
        routes["h"] = [(h > 0).float().cpu().view(T, Nc, -1) for h in v["h"]]
        if agg == "max":
            routes["amax"] = v["amax"].cpu()
    return routes


def _vanilla_flips(routes, pres, tie=None):
    flips = U.encoder_flips(routes["enc_qry"], pres["enc_qry"], "target images", tie)
    if "enc_ctx" in routes:
        flips += U.encoder_flips(routes["enc_ctx"], pres["enc_ctx"], "context images", tie)
        flips += sum(U.relu_flips(m, v, "encoder_r", tie) for m, v in zip(routes["h"], pres["h"]))
    flips += sum(U.relu_flips(m, v, "decoder0", tie) for m, v in zip(routes["d"], pres["d"]))
    if "amax" in routes:
        rs = pres["rs"]
        gap = rs.max(dim=1).values - torch.gather(rs, 1, routes["amax"].long().unsqueeze(1)).squeeze(1)
        assert not bool((gap > (U.TIE if tie is None else tie) * rs.abs().max()).any()), "max aggregator: arg-max differs away from a tie"
        flips += int((gap > 0).sum())
    return flips


FLIP_RATE = U.FLIP_RATE


def _count_decisions(obj):
    if torch.is_tensor(obj):
        return obj.numel()
    if isinstance(obj, dict):
        return sum(_count_decisions(v) for v in obj.values())
    return sum(_count_decisions(v) for v in obj)


def _run_case(gpulib, name):
    from mlhot import ops
    from trainer.losses import LossFunc
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = U.case_inputs(meta)
    task, agg = meta["cfg"]["task"], meta["cfg"]["agg_mode"]
    model.train()
    ops.saved_taps = []
    try:
        mu, var, kl = model(cx.to(DEV), cy.to(DEV), qx.to(DEV))
    finally:
        taps, ops.saved_taps = ops.saved_taps, None
    assert var is None and kl == 0
    loss = LossFunc("mse", task).calc_loss(mu, var, qy.to(DEV))
    loss.backward()
    assert U.rel_err(mu, fx["mu"]) <= U.RTOL
    assert abs(loss.item() - float(fx["loss"])) <= U.RTOL * max(1.0, abs(float(fx["loss"])))
    grads = {k: p.grad for k, p in model.named_parameters()}
    # the oracle under the kernels' routing
    T, Nc, Nq = cx.shape[0], cx.shape[1], qx.shape[1]
    routes = _vanilla_routes(gpulib, taps, T, Nc, Nq, agg)
    p = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
    pres = {}
    mu_r = O.vanilla_np_forward(p, cx, cy, qx, agg, tanh=model.OUT_TANH, routes=routes, pres=pres)
    O.calc_loss(task, mu_r, qy).backward()
    assert U.rel_err(mu, mu_r) <= U.RTOL
    flips = _vanilla_flips(routes, pres)
    decisions = _count_decisions(routes)
    assert flips <= max(1, FLIP_RATE * decisions), f"{name}: {flips} flips in {decisions} decisions"
    gmax = max(p[k].grad.abs().max().item() for k, _ in model.named_parameters() if p[k].grad is not None)
    worst_routed = (0.0, None)
    for k, _ in model.named_parameters():
        if p[k].grad is None:
            assert grads[k] is None, k           # an empty context leaves the latent path without gradients
            continue
        e = U.rel_err(grads[k], p[k].grad, floor=U.GRAD_FLOOR * gmax)
        if e >= worst_routed[0]:
            worst_routed = (e, k)
        assert e <= U.RTOL, k
    # the REFERENCE's own gradients (the fixture), always: at 1e-4 when every routing decision equals the oracle's, otherwise at
    # 1e-4 + (flips + 1) x U.FLIP_SHARE / n_images (tests/util.py; every differing decision was proven a <= 1e-5 tie above; their
    # exact effect, measured in the oracle, is logged) - never skipped
    def effect():          # the differing decisions' exact effect, measured in the oracle: its gradients under its OWN routing vs under the kernels'
        p2 = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
        O.calc_loss(task, O.vanilla_np_forward(p2, cx, cy, qx, agg, tanh=model.OUT_TANH), qy).backward()
        return U.flip_effect({k: p[k].grad for k, _ in model.named_parameters()}, {k: p2[k].grad for k, _ in model.named_parameters()}, U.GRAD_FLOOR * gmax)
    w_fix, k_fix, bound = U.check_grads_against_fixture_flipped(grads, fx, meta, flips, name, effect=effect)
    line = (f"{name} [{os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].split(' ')[0]}]: {flips} of {decisions} routing decisions differ from the "
            f"oracle's own (each proven a <= {U.TIE:g} tie); gradients vs the oracle under the kernels' routing: worst {worst_routed[0]:.2e} "
            f"({worst_routed[1]}) <= {U.RTOL:g}; vs the REFERENCE's own gradients (fixture): worst {w_fix:.2e} ({k_fix}) <= {bound:.2e}")
    print(line)
    U.parity_log(line)
    with torch.no_grad():
        model.eval()
        mu_t, _, _ = model(cx.to(DEV), cy.to(DEV), qx.to(DEV), test=True)
        lt = LossFunc("mse", task).calc_loss(mu_t, None, qy.to(DEV), test=True)
    # derived from the 1e-4 bar on mu (tests/util.py::test_loss_allowance: the degree loss's acos is the one amplifying step), not a flat 1e-3
    allow = U.test_loss_allowance(task, mu_t, qy) + 1e-5 * max(1.0, abs(float(fx["loss_test"])))
    err_t = abs(lt.item() - float(fx["loss_test"]))
    U.parity_log(f"{name}: test-mode loss {lt.item():.6f} vs the reference's {float(fx['loss_test']):.6f}: off by {err_t:.2e}, allowed {allow:.2e}")
    assert err_t <= allow, (name, err_t, allow)
    return flips


@pytest.fixture(params=[(1, 7935), (1, 63), (1, 0), (0, 0)], ids=["tail_spec", "tail_spec_round4_form", "tail_fused", "tail_generic"])
def tail_impl(gpulib, request):
    """The three flavours of everything between the encoder and the loss: the fused per-task / per-head tail kernels specialised
    for the shipped dimensions (csrc/tail_spec.h: dim_w = dim_z = 64, hidden 100; the default where it applies), the same
    phases with run-time shapes (csrc/tail_fused.h; ANP with <= 16 shots) and the generic operator chain.  `round4_form`: the six
    specialised kernels without round 5's additions (bits 64 .. 4096 of the option: the encoder Linear's fold inside phase A,
    the loss's gradient inside phase C', phases B' / C' / A' as two / four / four workgroups per (task, head) / task)."""
    gpulib.set_option("tail_fused", request.param[0])
    gpulib.set_option("tail_spec", request.param[1])
    yield request.param
    gpulib.set_option("tail_fused", 1)
    gpulib.set_option("tail_spec", 7935)


@pytest.mark.parametrize("name", U.model_case_names("s_"))
def test_model_edge_cases_vs_reference(gpulib, tail_impl, name):
    _run_case(gpulib, name)


TAIL_SPEC_BITS = (1, 2, 4, 8, 16, 32, 64, 128, 512, 1024, 2048, 4096)       # csrc/options.h enum TailSpec (256 is unassigned)


@pytest.mark.parametrize("bit", TAIL_SPEC_BITS)
@pytest.mark.parametrize("name", ["s_anp_shapenet1d_ragged", "s_cnp_shapenet1d_max"])
def test_model_with_one_tail_spec_bit_cleared(gpulib, name, bit):
    """`tail_impl` visits 4 states of the route table (csrc/np_vanilla.h np_route); here every assigned bit of option tail_spec is
    cleared on its own, on one whole-model case per fused family whose dims the specialised kernels accept, at the case's usual
    tolerances (_run_case)."""
    assert sum(TAIL_SPEC_BITS) == 7935
    gpulib.set_option("tail_spec", 7935 & ~bit)
    try:
        _run_case(gpulib, name)
    finally:
        gpulib.set_option("tail_spec", 7935)


def test_mid_size_case_takes_the_reference_gradient_branch(gpulib):
    """T = 2, 15 + 15 shots (60 images, 9.6 M routing decisions): no decision differs from the oracle's, so _run_case compares
    every gradient with the REFERENCE's own (the fixture) and not only with the routed oracle."""
    assert _run_case(gpulib, "s_anp_shapenet1d_t2_full") == 0


@pytest.mark.parametrize("T,Nc,Nq", [(3, 7, 9), (2, 15, 15), (1, 16, 16)])
def test_tail_with_sharp_attention_vs_oracle(gpulib, tail_impl, T, Nc, Nq):
    """At the seeded initial weights the encoder features of all images are almost identical (spread 0.008 around a common
    mean), FAVOR+'s attention is uniform and the query / key gradients are rounding residue (1e-8 of the model's largest
    gradient): the fixtures cannot see an error in the dq / dk path of the tail kernels.  Here the encoder's last layer is
    re-centred and scaled (features = 0.5 / spread * (features - mean)) so that the attention weights differ from key to key
    and those gradients are first-class (>= 1e-5 of the largest): mu, loss and every gradient at 1e-4 against the fp64 oracle
    under the kernels' routing, the W_q / W_k ones at 2e-4 of their OWN scale, no floor.  (Found by the trajectory test: a
    wrong per-row normaliser in the specialised backward, invisible at 1e-4 with the usual floor.)"""
    import types
    from mlhot import ops
    from mlhot.synth import get_batch
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=T, input_dim=3,
                                output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                dim_z=64, task="shapenet_1d")
    model = ANPShapeNet1D(cfg).to(DEV)
    cx, qx, cy, qy = get_batch("shapenet_1d", T, Nc, Nq, seed=77)
    with torch.no_grad():
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        f = O.vanilla_encoder(torch.cat([cx.reshape(-1, 1, 128, 128), qx.reshape(-1, 1, 128, 128)]), sd)
        scale = 0.5 / f.std(dim=0).mean().item()
        model.encoder_w0[8].weight.mul_(scale)
        model.encoder_w0[8].bias.copy_(((sd["encoder_w0.8.bias"] - f.mean(dim=0)) * scale).to(DEV))
    ops.saved_taps = []
    try:
        mu = model(cx.to(DEV), cy.to(DEV), qx.to(DEV))[0]
    finally:
        taps, ops.saved_taps = ops.saved_taps, None
    LossFunc("mse", "shapenet_1d").calc_loss(mu, None, qy.to(DEV)).backward()
    routes = _vanilla_routes(gpulib, taps, T, Nc, Nq, "attention")
    r64 = {k: (tuple(t.double() if t.is_floating_point() else t for t in v) if isinstance(v, tuple) else [t.double() for t in v])
           for k, v in routes.items()}
    p = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
    mu_o = O.vanilla_np_forward(p, cx.double(), cy.double(), qx.double(), "attention", tanh=True, routes=r64)
    O.calc_loss("shapenet_1d", mu_o, qy.double()).backward()
    assert U.rel_err(mu, mu_o) <= U.RTOL
    gmax = max(p[k].grad.abs().max().item() for k, _ in model.named_parameters())
    qk = [p[k].grad.abs().max().item() / gmax for k, _ in model.named_parameters() if k.startswith("_W_q") or k.startswith("_W_k")]
    assert min(qk) > 1e-6, f"attention not sharp enough for this test: query / key gradients at {min(qk):.1e} of the largest"
    worst, worst_qk = (0.0, None), (0.0, None)
    for k, prm in model.named_parameters():
        if k.startswith("_W_q") or k.startswith("_W_k"):
            e = U.rel_err(prm.grad, p[k].grad)
            worst_qk = max(worst_qk, (e, k))
            assert e <= 2e-4, f"{k}: {e:.2e} of its own scale"
        else:
            e = U.rel_err(prm.grad, p[k].grad, floor=U.GRAD_FLOOR * gmax)
            worst = max(worst, (e, k))
            assert e <= U.RTOL, f"{k}: {e:.2e}"
    print(f"sharp attention T={T} {Nc}+{Nq}: query / key gradients at {min(qk):.1e} .. {max(qk):.1e} of the largest, worst error "
          f"{worst_qk[0]:.2e} of their own scale ({worst_qk[1]}); others {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("method,agg,task,shape", [("ANPShapeNet1D", "attention", "shapenet_1d", (3, 7, 9)), ("ANPShapeNet1D", "attention", "shapenet_1d", (2, 15, 15)),
                                                   ("ANPShapeNet1D", "attention", "shapenet_1d", (2, 17, 20)), ("CNPShapeNet1D", "mean", "shapenet_1d", (3, 7, 9)),
                                                   ("ANPVanillaPascal1D", "attention", "pascal_1d", (2, 5, 5))])
def test_loss_gradient_taken_inside_the_models_backward(gpulib, method, agg, task, shape):
    """mlhot_np_vanilla_bwd_loss (mlhot.ops.defer_loss_grad): calc_loss(mu, ., y).backward() with the loss's gradient derived by the
    model's first backward kernel (phase C' of the specialised attention tail; materialised inside the C call for every other
    configuration: CNP, > 16 shots) gives BIT-IDENTICAL parameter gradients to the two-node form - also when mu has a second
    consumer (autograd adds its gradient to the zero placeholder, the kernel adds the loss's on top), and with the loss VALUE left to
    the same kernel (loss_value_aside: one extra workgroup of phase C' / the CNP tail's backward; a launch inside the C call for the
    other configurations) - the same bits as mlhot_loss_fwd's."""
    import importlib
    import types
    from mlhot import ops
    from trainer.losses import LossFunc
    T, Nc, Nq = shape
    pascal = task == "pascal_1d"
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=T, input_dim=1 if pascal else 3,
                                output_dim=1 if pascal else 2, agg_mode=agg, img_agg="", dim_w=64, n_hidden_units_r=[100, 100],
                                dim_r=64 if agg == "attention" else 100, dim_z=64, task=task)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
    g = torch.Generator().manual_seed(5)
    L = cfg.input_dim
    cx, qx = torch.rand(T, Nc, 1, 128, 128, generator=g).to(DEV), torch.rand(T, Nq, 1, 128, 128, generator=g).to(DEV)
    cy, qy = torch.rand(T, Nc, L, generator=g).to(DEV), torch.rand(T, Nq, L, generator=g).to(DEV)
    loss_fn = LossFunc("mse", task)
    seed = torch.full((), 0.75, device=DEV)

    def run(defer, second_consumer, aside):
        model.zero_grad(set_to_none=True)
        mu = model(cx, cy, qx)[0]
        with (ops.loss_value_aside(enabled=True) if aside else ops.loss_grad_in_backward(enabled=defer)):
            loss = loss_fn.calc_loss(mu, None, qy)
            total = loss + 0.3 * (mu * mu).sum() if second_consumer else loss
            total.backward(gradient=seed)
        torch.cuda.synchronize()
        return loss.item(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    assert ops.defer_loss_grad is False          # opt-in: outside a scope the two-node form runs
    for second in (False, True):
        ref_loss, ref = run(False, second, False)
        for aside in ((False, True) if not second else (False,)):      # with a second consumer the sum reads the loss inside the block: no lane
            got_loss, got = run(True, second, aside)
            assert got_loss == ref_loss and got.keys() == ref.keys()
            for k in ref:
                assert torch.equal(got[k], ref[k]), (k, second, aside)
    # the placeholder autograd carried is still all zeros (nothing accumulated into it in place)
    assert all(float(z.abs().max()) == 0.0 for z in ops._zero_grads.values())
    # asking for d loss / d mu itself (retain_grad) keeps the two-node form: the real gradient reaches mu.grad
    with ops.loss_grad_in_backward():
        mu = model(cx, cy, qx)[0]
        mu.retain_grad()
        loss_fn.calc_loss(mu, None, qy).backward()
        assert float(mu.grad.abs().max()) > 0
    # outside a scope a pass that stops at mu gets the real gradient ...
    mu = model(cx, cy, qx)[0]
    loss = loss_fn.calc_loss(mu, None, qy)
    real = torch.autograd.grad(loss, mu, retain_graph=True)[0]
    assert float(real.abs().max()) > 0
    # ... and inside one it is an ERROR, not a placeholder of zeros; the parked descriptor is gone afterwards, so a later full
    # backward of the same graph is the plain two-node one
    mu = model(cx, cy, qx)[0]
    with ops.loss_grad_in_backward():
        loss = loss_fn.calc_loss(mu, None, qy)
        with pytest.raises(RuntimeError, match="placeholder"):
            torch.autograd.grad(loss, mu, retain_graph=True)
    assert mu.grad_fn.loss is None
    model.zero_grad(set_to_none=True)
    with ops.loss_grad_in_backward():
        loss.backward(gradient=seed)
    torch.cuda.synchronize()
    ref_loss, ref = run(False, False, False)
    for k in ref:
        assert torch.equal(model.get_parameter(k).grad, ref[k]), k


@pytest.mark.parametrize("name", U.model_case_names("c"))
def test_model_baseline_configs_vs_reference(gpulib, tail_impl, name):
    """BASELINE.json configs[0..2] at their full sizes (T=4 5+5; T=16 15+15 CNP / ANP): every gradient at 1e-4."""
    _run_case(gpulib, name)


@pytest.mark.parametrize("name", U.model_case_names("c"))
@pytest.mark.parametrize("bits", [1, 7], ids=["forward", "forward_and_gradients"])
def test_model_baseline_configs_with_split_precision_conv2(gpulib, name, bits):
    """The same cases, same tolerances, with the opt-in split-precision conv2 kernels (csrc/conv_split.h) in the path: the forward
    alone, and the forward with both gradients."""
    gpulib.set_option("conv2_split", bits)
    try:
        _run_case(gpulib, name)
    finally:
        gpulib.set_option("conv2_split", 0)


@pytest.mark.parametrize("case", SC.CASES)
def test_split_precision_error_vs_fp32_mfma(gpulib, case):
    """per-element error against float64 of the split-bf16 conv12 kernels and of the exact-fp32 MFMA kernels on
    adversarial operands (tests/split_cases.py: 2^+-40 dynamic range inside one K reduction, trained-scale weights, sign-cancelling and
    same-sign sums, conv1 exact by construction so that only conv2's three reductions differ).  Measured on MI355X
    (gpurun_out/split_error_<case>.txt has the table of the run; DESIGN.md section 4 the round's):
      forward (p2): the split kernel's error is 0.2 - 0.8 x the fp32 kernel's in every case, max and rms -> asserted <= 1.0 x;
      gradients: 0.2 - 2.5 x at this size (rms: dW2 0.9 - 1.1, dW1 / db1 0.8 - 2.1); at the shipped 480 images 0.3 - 1.5 x with
      one outlier at 4.5 x (db1 of the range case; profiles/r04_final_split_error_vs_float64_480.txt).  v_mfma_f32_16x16x32_bf16 FLOORS its addends - the
      accumulator included - to 25 bits below the largest product of each 8-term step (scripts/micro/mfma_bf16_accum.hip), where an
      fp32 chain rounds to nearest; the gradient kernels therefore run half of their sums on negated operands (the data gradient:
      half of the waves hold -W2 and the bands alternate in sign; the weight gradient: every other band goes as -dY into a second
      accumulator set), so that the
      floors cancel instead of adding up over the batch.  That leaves them AT the fp32 kernels' level, not below it in every
      case -> asserted <= 3 x (and <= 2e-6 of the largest element wherever the fp32 kernel itself is that exact).  This is why the
      split kernels stay opt-in."""
    n = 8
    res = SC.measure(gpulib, case, n)
    lines = [f"{case} n={n}: quantity, (max, rms) fp32, (max, rms) split, ratios"]
    for q, (e32, es) in res.items():
        lines.append(f"{q:4s} {e32[0]:.3e} {e32[1]:.3e} | {es[0]:.3e} {es[1]:.3e} | {es[0] / max(e32[0], 1e-300):.2f} {es[1] / max(e32[1], 1e-300):.2f}")
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", f"split_error_{case}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    e32, es = res["p2"]
    assert es[0] <= 1.0 * e32[0] and es[1] <= 1.0 * e32[1], ("p2", e32, es)
    for q in ("dw1", "db1", "dw2", "db2"):
        e32, es = res[q]
        assert es[0] <= max(3.0 * e32[0], 2e-6) and es[1] <= max(3.0 * e32[1], 1e-6), (q, e32, es)
        assert es[0] <= 1e-4 or e32[0] > 3e-5, (q, e32, es)       # north_star's tolerance wherever the fp32 kernel keeps it


def test_conv12_block_entries_vs_encoder(gpulib):
    """mlhot_conv12_fwd / _bwd (the encoder's first block on its own) give what the whole-encoder entry keeps and returns."""
    n = 5
    p = _enc_params(7)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, 1, 128, 128, generator=g).to(DEV)
    plist = [t.to(DEV) for t in p.values()]
    f0, _, saved = gpulib.enc_vanilla_fwd(x, None, plist, 64)
    _, p2_ref, am_ref, _ = gpulib.enc_saved_views(saved, n)
    p2, am2, saved12 = gpulib.conv12_fwd(x, *plist[:4])
    assert torch.equal(p2, p2_ref) and torch.equal(am2, am_ref)
    # d p2 of a plain sum of p2 squares; reference through autograd on the CPU under the kernel's routing
    dp2 = (2 * p2).contiguous()
    got = gpulib.conv12_bwd(x, plist[0], plist[1], plist[2], dp2, saved12)
    routes = gpulib.enc_routes(saved12, n)
    _, ref = SC.ref64(x.cpu(), *[t.cpu() for t in plist[:4]], dp2.cpu(), routes)
    for a, r, name in zip(got, ref, ("dw1", "db1", "dw2", "db2")):
        assert U.rel_err(a.cpu(), r.float()) <= 1e-5, name


@pytest.mark.parametrize("name", [n for n in U.resnet_case_names() if n != "r_anpmr_shapenet3d"])   # that one: test_anpmr_shapenet3d_vs_reference
def test_resnet_models_vs_reference(gpulib, name):
    """ResNet-encoder CondNeuralProcess / ANP (ShapeNet3D 64x64x3 quaternions, Distractor 128x128x1)
    through the plugin boundary: run-time-shaped conv kernels, linears, aggregators, FAVOR+ (d=256, m=1419).
    Outputs and loss are held to 1e-4 against the reference's vectors.  Gradients: these models have ~1e6
    ReLU decisions per pass and every batch contains pre-activations within 1e-7 of zero, so the check is
    made with the oracle evaluated under the KERNELS' routing (each disagreement with the oracle's own sign
    must sit on a <=1e-5 tie); when no decision flipped, the reference's gradients are compared as well."""
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = U.resnet_case_inputs(meta, fx)
    from trainer.losses import LossFunc
    model.img_encoder.tap_log, model.decoder.tap_log = [], []
    mu, var, kl = model(cx.to(DEV), cy.to(DEV), qx.to(DEV))
    assert var is None and kl == 0
    loss = LossFunc("mse", meta["cfg"]["task"]).calc_loss(mu, var, qy.to(DEV))
    loss.backward()
    assert U.rel_err(mu, fx["mu"]) <= U.RTOL
    assert abs(loss.item() - float(fx["loss"])) <= U.RTOL * max(1.0, abs(float(fx["loss"])))
    grads = {k: p.grad for k, p in model.named_parameters()}
    # oracle under the kernels' routing
    routes = [[(t.detach().cpu() > 0).float() for t in taps] for taps in model.img_encoder.tap_log + model.decoder.tap_log]
    p = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
    pres = []
    mu_r = O.resnet_np_forward(p, cx, cy, qx, meta["cfg"]["agg_mode"], meta["cfg"]["img_agg"], routes=routes, pres=pres)
    O.calc_loss(meta["cfg"]["task"], mu_r, qy).backward()
    flips = 0
    for masks, pre in zip(routes, pres):
        for m, v in zip(masks, pre):
            bad = (m > 0) != (v > 0)
            flips += int(bad.sum())
            assert not bool((bad & (v.abs() > 1e-5 * v.abs().max())).any()), "routing differs away from a tie"
    decisions = _count_decisions(routes)
    print(f"{name}: {flips} of {decisions} ReLU decisions differ from the oracle's own")
    assert flips <= max(1, FLIP_RATE * decisions)       # these cases hold 2-5 images: one tie at most
    gmax = max(p[k].grad.abs().max().item() for k, _ in model.named_parameters() if p[k].grad is not None)
    for k, prm in model.named_parameters():
        if p[k].grad is None:
            assert grads[k] is None, k
            continue
        assert U.rel_err(grads[k], p[k].grad, floor=U.GRAD_FLOOR * gmax) <= U.RTOL, k
    # the reference's own gradients, always (1e-4; with decisions that sit on a tie and fell the other way: + their measured effect)
    def effect():
        p2 = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
        O.calc_loss(meta["cfg"]["task"], O.resnet_np_forward(p2, cx, cy, qx, meta["cfg"]["agg_mode"], meta["cfg"]["img_agg"]), qy).backward()
        return U.flip_effect({k: p[k].grad for k, _ in model.named_parameters()}, {k: p2[k].grad for k, _ in model.named_parameters()}, U.GRAD_FLOOR * gmax)
    U.check_grads_against_fixture_flipped(grads, fx, meta, flips, name, effect=effect, head=1024, stride_cap=4096)


def _anpmr3d_routed_check(model, cx, cy, qx, qy, fx=None, meta=None, dtype=torch.float32, fx_kw=None):
    """One seeded forward + backward of an ANPMRShapeNet3D on the device against the oracle under the same eps draws and the
    KERNELS' ReLU routing (2 Bayes-by-backprop encoder passes + the decoder ResNet, 9 masks each); returns (mu, kl, loss, flips).
    `dtype`: the oracle's arithmetic.  fp32 is the reference's own; at the full c5 size the stem's weight gradient is a sum over
    245 760 positions with heavy cancellation, where the fp32 CPU sum itself carries ~2e-4 of rounding noise - there the oracle
    runs in fp64 (same eps values, same routing), i.e. the kernels are held to 1e-4 of the exact result."""
    from trainer.losses import LossFunc
    model.img_encoder.tap_log, model.decoder.tap_log = [], []
    torch.manual_seed(99)
    mu, var, kl = model(cx.to(DEV), cy.to(DEV), qx.to(DEV))
    loss = LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy.to(DEV))
    (loss + 1e-7 * kl).backward()
    assert var is None
    grads = {k: p.grad for k, p in model.named_parameters()}
    routes = [[(t.detach().cpu() > 0).float() for t in taps] for taps in model.img_encoder.tap_log + model.decoder.tap_log]
    model.img_encoder.tap_log, model.decoder.tap_log = None, None
    assert len(routes) == 3 and all(len(r) == 9 for r in routes)
    p = {k: v.detach().cpu().to(dtype).requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
    pres = []
    torch.manual_seed(99)
    mu_o, kl_o = O.anpmr3d_forward(p, cx.to(dtype), cy.to(dtype), qx.to(dtype), routes=[[m.to(dtype) for m in r] for r in routes], pres=pres)
    loss_o = O.calc_loss("shapenet_3d", mu_o, qy.to(dtype))
    (loss_o + 1e-7 * kl_o).backward()
    assert U.rel_err(mu, mu_o) <= U.RTOL
    assert abs(kl.item() - kl_o.item()) <= U.RTOL * kl_o.item()
    assert abs(loss.item() - loss_o.item()) <= U.RTOL * max(1.0, abs(loss_o.item()))
    flips = sum(U.relu_flips(m, v, "resnet") for masks, pre in zip(routes, pres) for m, v in zip(masks, pre))
    decisions = _count_decisions(routes)
    print(f"anpmr3d {tuple(cx.shape)}: {flips} of {decisions} ReLU decisions differ from the oracle's own")
    assert flips <= max(1, FLIP_RATE * decisions)
    gmax = max(p[k].grad.abs().max().item() for k, _ in model.named_parameters() if p[k].grad is not None)
    for k, _ in model.named_parameters():
        if p[k].grad is None:
            assert grads[k] is None, k       # decoder.resnet.fc.* never receive a gradient
            continue
        assert U.rel_err(grads[k], p[k].grad, floor=U.GRAD_FLOOR * gmax) <= U.RTOL, k
    def effect():
        p2 = {k: v.detach().cpu().to(dtype).requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
        torch.manual_seed(99)
        mu2, kl2 = O.anpmr3d_forward(p2, cx.to(dtype), cy.to(dtype), qx.to(dtype))
        (O.calc_loss("shapenet_3d", mu2, qy.to(dtype)) + 1e-7 * kl2).backward()
        return U.flip_effect({k: p[k].grad for k, _ in model.named_parameters()}, {k: p2[k].grad for k, _ in model.named_parameters()}, U.GRAD_FLOOR * gmax)
    _anpmr3d_routed_check.effect = effect          # for callers that compare against a fixture themselves (the c5 full-size test)
    if fx is not None:
        U.check_grads_against_fixture_flipped(grads, fx, meta, flips, f"anpmr3d {tuple(cx.shape)} {meta.get('name', '')}", effect=effect, head=1024, stride_cap=4096, **(fx_kw or {}))
    return mu, kl, loss, kl_o, flips


def test_anpmr_shapenet3d_vs_reference(gpulib):
    """BASELINE config c5's model (ANPMRShapeNet3D, Bayes-by-backprop encoder): same seeded eps draws as the
    reference (torch.manual_seed(99) before the forward), mu / kl / loss at 1e-4 against the reference's vectors; every
    gradient of loss + 1e-7*kl at 1e-4 against the oracle under the same draws and the kernels' ReLU routing (each routing
    difference proven a <= 1e-5 tie), and against the reference's own gradients when no decision differs."""
    fx, meta = U.load_case("r_anpmr_shapenet3d")
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = U.resnet_case_inputs(meta, fx)
    mu, kl, loss, _, _ = _anpmr3d_routed_check(model, cx, cy, qx, qy, fx, meta)
    assert U.rel_err(mu, fx["mu"]) <= U.RTOL
    assert abs(kl.item() - float(fx["kl"])) <= U.RTOL * float(fx["kl"])
    assert abs(loss.item() - float(fx["loss"])) <= U.RTOL * max(1.0, abs(float(fx["loss"])))


@pytest.mark.parametrize("name", U.c5_full_case_names())
def test_c5_full_size_forward_backward_vs_oracle(gpulib, name):
    """BASELINE config c5 at its per-GPU size (ANPMRShapeNet3D, 8 tasks x (15 + 15) 3x64x64 images: 240 + 120 encoder images,
    FAVOR+ at d = 256 / m = 1419 over 15 x 15 shots) against (1) the REFERENCE's own vectors at that size
    (tests/golden/c5_anpmr_shapenet3d_t8*.npz, generated by importing /root/reference: mu, kl, the quaternion loss at 1e-4, every
    gradient of loss + 1e-7*kl at 1e-4 - plus, when routing decisions sit on a tie and fell the other way, (flips + 1) x
    U.FLIP_SHARE / 360 images - never skipped), and (2) the CPU oracle evaluated in fp64 (see _anpmr3d_routed_check) under the same seeded eps draws and the kernels'
    ReLU routing (360 images x ~1e5 decisions each) at 1e-4 flat.  `_7_23`: one batch of the reference's TRAINING draw - context
    size ~ U{1..15}, the other 30 - Nc views of the object are the targets (dataset/shapenet_3d.py:110, 200-204); `_survey`:
    SURVEY section 8c's input recipe, whose recorded answers (loss 2.26335859, kl 1383162.5) are asserted as well.
    The stem's weight gradient sums 245 760 positions; the reference's fp32 CPU sum itself carries ~2e-4 of rounding noise there
    (fp32 oracle vs fp64 oracle), so against the fixture the conv1 (stem) tensors get 3e-4, everything else 1e-4."""
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = U.c5_full_case_inputs(meta)
    T, Nq = cx.shape[0], qx.shape[1]
    mu, kl, loss, kl_o, flips = _anpmr3d_routed_check(model, cx, cy, qx, qy, dtype=torch.float64)
    assert mu.shape == (T, Nq, 4)
    assert abs(kl_o.item() - 1383162.5) < 4.0      # SURVEY §8c known answer
    # the reference's own answers at this size
    assert U.rel_err(mu, fx["mu"]) <= U.RTOL
    assert abs(kl.item() - float(fx["kl"])) <= U.RTOL * float(fx["kl"])
    assert abs(loss.item() - float(fx["loss"])) <= U.RTOL * max(1.0, abs(float(fx["loss"])))
    if meta["labels"] == "rand":
        assert abs(loss.item() - 2.26335859) <= U.RTOL * 2.26335859
    grads = {k: p.grad for k, p in model.named_parameters()}
    stem = {k: g for k, g in grads.items() if k.startswith("img_encoder.net.layer1.conv.") or k.startswith("decoder.conv1.")}
    rest = {k: g for k, g in grads.items() if k not in stem}
    eff = None            # (the measured effect would be a second fp64 oracle run at 360 images: ~30 s per case; the bound does not use it)
    gm = U.fixture_gmax(grads, fx)
    w1 = U.check_grads_against_fixture_flipped(rest, fx, meta, flips, name, effect=eff, gmax=gm, head=1024, stride_cap=4096)
    w2 = U.check_grads_against_fixture_flipped(stem, fx, meta, flips, name + " (stem tensors)", tol=3e-4, gmax=gm, head=1024, stride_cap=4096)
    total = sum(float(g.double().norm()) ** 2 for g in grads.values() if g is not None) ** 0.5
    assert abs(total - meta["grad_norm_total"]) <= U.RTOL * meta["grad_norm_total"]
    print(f"{name}: {flips} routing decisions on a tie; vs the reference's vectors: gradients worst {w1[0]:.2e} ({w1[1]}), stem {w2[0]:.2e} ({w2[1]}); "
          f"|grad| {total:.8f} (reference {meta['grad_norm_total']:.8f})")


def _sharpen_resnet_attention(model, forward):
    """Make the FAVOR+ attention of a ResNet-family ANP non-degenerate.  At the seeded weights the query /
    key rows q = W_q x + b have norms of O(10): exp(dd - diag - max) underflows below the +1e-4 floor and the reference's own
    W_q / W_k gradients are 0 .. 4e-4 of the largest.  One recording pass (`forward()` under no_grad) captures the encoder features
    that enter the head projections; every head's projection is then re-centred and scaled,
        W <- s W,  b <- -s W mean(x),   s = 0.25 / std(W (x - mean x)),
    so that the rows have zero mean and 0.25 spread per component: dd has unit spread, diag ~ 0.5 (the regime favor_c5.npz pins
    for the kernels in isolation).  Returns the measured spread of q / k before the change."""
    seen = {}
    mha0 = model._multihead_attention

    def rec(k, v, q):
        for x, mods in ((q, model._W_q), (k, model._W_k), (v, model._W_v)):
            seen[id(mods)] = x.detach().reshape(-1, x.shape[-1]).clone()
        return mha0(k, v, q)
    model._multihead_attention = rec
    try:
        with torch.no_grad():
            forward()
    finally:
        del model._multihead_attention
    before = {}
    with torch.no_grad():
        for name, mods in (("q", model._W_q), ("k", model._W_k)):
            x = seen[id(mods)]
            xm = x.mean(dim=0)
            for m in mods:
                w = m.linear.weight
                rows = (x - xm) @ w.t()
                before[name] = float((x @ w.t() + m.linear.bias).std())
                sc = 0.25 / float(rows.std())
                m.linear.bias.copy_(-(w @ xm) * sc)
                w.mul_(sc)
        # value rows: at the seeded weights of the plain ANP the task encoder's features are tiny (spread 0.06) and with them the
        # query / key gradients (~1e-6 of the model's largest); scaled to unit spread - the common component of the rows, which
        # is what makes the attention backward ill-conditioned (favor2.h B1), stays
        x = seen[id(model._W_v)]
        vs = float(torch.cat([x @ m.linear.weight.t() + m.linear.bias for m in model._W_v]).std())
        before["v"] = vs
        if vs < 1.0:
            for m in model._W_v:
                m.linear.weight.mul_(1.0 / vs)
                m.linear.bias.mul_(1.0 / vs)
    return before


@pytest.mark.parametrize("method,Nc,Nq", [("ANPMRShapeNet3D", 15, 15), ("ANPMRShapeNet3D", 7, 23), ("ANP", 15, 15)])
def test_resnet_anp_with_sharp_attention_vs_oracle(gpulib, favor_impl, method, Nc, Nq):
    """The ResNet-family twin of test_tail_with_sharp_attention_vs_oracle, at c5's per-GPU size (8 tasks, 64x64x3, FAVOR+ at d = 256 /
    m = 1419 - ANPMRShapeNet3D.py:160-183, fast_attention.py:74-99,151-156): with the head projections re-centred and scaled
    (_sharpen_resnet_attention) the W_q / W_k gradients are first-class - asserted: the smallest of them > 1e-5 of the model's
    largest gradient entry - and are held to 2e-4 of their OWN scale against the fp64 oracle under the same eps draws and the
    kernels' ReLU routing; mu, loss and every other gradient at 1e-4 as in the other whole-model tests.  Both FAVOR+
    implementations (favor2.h's two launches per direction, favor.h's chain)."""
    import importlib
    import types
    from trainer.losses import LossFunc
    T = 8
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=T, input_dim=4, output_dim=4,
                                agg_mode="attention", img_agg="reshape" if method == "ANPMRShapeNet3D" else "max", task="shapenet_3d",
                                temperature=0.07)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
    g = torch.Generator().manual_seed(4321)
    cx, qx = torch.rand(T, Nc, 3, 64, 64, generator=g), torch.rand(T, Nq, 3, 64, 64, generator=g)
    cy = F.normalize(torch.randn(T, Nc, 4, generator=g), dim=-1)
    qy = F.normalize(torch.randn(T, Nq, 4, generator=g), dim=-1)
    mr = method == "ANPMRShapeNet3D"

    def forward():
        torch.manual_seed(99)
        return model(cx.to(DEV), cy.to(DEV), qx.to(DEV))
    before = _sharpen_resnet_attention(model, forward)
    model.img_encoder.tap_log, model.decoder.tap_log = [], []
    mu, var, kl = forward()
    loss = LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy.to(DEV))
    (loss + 1e-7 * kl).backward()
    routes = [[(t.detach().cpu() > 0).double() for t in taps] for taps in model.img_encoder.tap_log + model.decoder.tap_log]
    model.img_encoder.tap_log, model.decoder.tap_log = None, None
    p = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
    pres = []
    torch.manual_seed(99)
    if mr:
        mu_o, kl_o = O.anpmr3d_forward(p, cx.double(), cy.double(), qx.double(), routes=routes, pres=pres)
    else:
        mu_o, kl_o = O.resnet_np_forward(p, cx.double(), cy.double(), qx.double(), "attention", cfg.img_agg, routes=routes, pres=pres), 0.0
    loss_o = O.calc_loss("shapenet_3d", mu_o, qy.double())
    (loss_o + 1e-7 * kl_o).backward()
    flips = sum(U.relu_flips(m, v, "resnet") for masks, pre in zip(routes, pres) for m, v in zip(masks, pre))
    assert flips <= max(1, FLIP_RATE * _count_decisions(routes))
    assert U.rel_err(mu, mu_o) <= U.RTOL
    assert abs(loss.item() - loss_o.item()) <= U.RTOL * max(1.0, abs(loss_o.item()))
    named = [(k, prm) for k, prm in model.named_parameters() if p[k].grad is not None]
    gmax = max(p[k].grad.abs().max().item() for k, _ in named)
    qk = {k: p[k].grad.abs().max().item() / gmax for k, _ in named if k.startswith("_W_q") or k.startswith("_W_k")}
    assert len(qk) == 32 and min(qk.values()) > 1e-5, \
        f"attention not sharp enough: query / key gradients at {min(qk.values()):.1e} of the largest"
    worst, worst_qk = (0.0, None), (0.0, None)
    for k, prm in named:
        assert prm.grad is not None, k
        if k in qk:
            e = U.rel_err(prm.grad, p[k].grad)                                  # its OWN scale, no floor
            worst_qk = max(worst_qk, (e, k))
            assert e <= 2e-4, f"{k}: {e:.2e} of its own scale"
        else:
            e = U.rel_err(prm.grad, p[k].grad, floor=U.GRAD_FLOOR * gmax)
            worst = max(worst, (e, k))
            assert e <= U.RTOL, f"{k}: {e:.2e}"
    print(f"sharp resnet attention {method} {Nc}+{Nq} favor2={favor_impl}: q / k row spread {before['q']:.2f} / {before['k']:.2f} -> 0.25, v {before['v']:.2f}; "
          f"W_q / W_k gradients at {min(qk.values()):.1e} .. {max(qk.values()):.1e} of the largest, worst error {worst_qk[0]:.2e} of their "
          f"own scale ({worst_qk[1]}); others {worst[0]:.2e} ({worst[1]}); {flips} routing ties")


@pytest.mark.parametrize("name", U.fcl_case_names())
def test_fcl_models_vs_reference(gpulib, name):
    """Functional-contrastive variants (FCLCNPShapeNet1D, FCLCNPDistractor, FCLANP) through the plugin boundary: the 4-tuple
    forward with the target labels; mu / regression loss / NT-Xent term against the fixtures produced by the reference (NT-Xent
    restated for the absent pytorch_metric_learning, see tests/golden/make_fixtures.py).  Gradients of (loss + term): the
    ResNet-family cases are checked against the oracle under the kernels' ReLU routing (see test_resnet_models_vs_reference) and,
    when no decision flipped, against the reference's gradients; the vanilla-encoder cases directly against the reference's."""
    from trainer.losses import LossFunc
    fx, meta = U.load_case(name)
    c = meta["cfg"]
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = U.resnet_case_inputs(meta, fx)
    resnet = meta["method"] != "FCLCNPShapeNet1D"
    if resnet:
        model.img_encoder.tap_log, model.decoder.tap_log = [], []
    mu, var, kl, contra = model(cx.to(DEV), cy.to(DEV), qx.to(DEV), qy.to(DEV))
    assert var is None and kl == 0
    loss = LossFunc("mse", c["task"]).calc_loss(mu, var, qy.to(DEV))
    (loss + contra).backward()
    assert U.rel_err(mu, fx["mu"]) <= U.RTOL
    assert abs(loss.item() - float(fx["loss"])) <= U.RTOL * max(1.0, abs(float(fx["loss"])))
    assert abs(contra.item() - float(fx["contra"])) <= U.RTOL * max(1.0, abs(float(fx["contra"])))
    grads = {k: p.grad for k, p in model.named_parameters()}
    if not resnet:
        # 3e-4: the NT-Xent term (see below)
        U.check_grads_against_fixture(grads, fx, meta, tol=3e-4, head=1024, stride_cap=4096)
    else:
        routes = [[(t.detach().cpu() > 0).float() for t in taps] for taps in model.img_encoder.tap_log + model.decoder.tap_log]
        p = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
        pres = []
        mu_r, contra_r = O.fcl_resnet_forward(p, cx, cy, qx, qy, c["agg_mode"], c["img_agg"], c.get("temperature", 0.07), routes=routes, pres=pres)
        (O.calc_loss(c["task"], mu_r, qy) + contra_r).backward()
        flips = 0
        for masks, pre in zip(routes, pres):
            for m, v in zip(masks, pre):
                bad = (m > 0) != (v > 0)
                flips += int(bad.sum())
                assert not bool((bad & (v.abs() > 1e-5 * v.abs().max())).any()), "routing differs away from a tie"
        gmax = max(p[k].grad.abs().max().item() for k, _ in model.named_parameters() if p[k].grad is not None)
        for k, prm in model.named_parameters():
            if p[k].grad is None:
                assert grads[k] is None, k
                continue
            # 3e-4: the NT-Xent term divides cosine similarities by the temperature (0.07), which scales the fp32 rounding
            # differences of the embeddings ~14x on their way back (measured worst case 1.4e-4, on the attention queries)
            assert U.rel_err(grads[k], p[k].grad, floor=U.GRAD_FLOOR * gmax) <= 3e-4, k
        def effect():
            p2 = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
            mu2, contra2 = O.fcl_resnet_forward(p2, cx, cy, qx, qy, c["agg_mode"], c["img_agg"], c.get("temperature", 0.07))
            (O.calc_loss(c["task"], mu2, qy) + contra2).backward()
            return U.flip_effect({k: p[k].grad for k, _ in model.named_parameters()}, {k: p2[k].grad for k, _ in model.named_parameters()}, U.GRAD_FLOOR * gmax)
        U.check_grads_against_fixture_flipped(grads, fx, meta, flips, name, tol=3e-4, effect=effect, head=1024, stride_cap=4096)
    with torch.no_grad():
        model.eval()
        if resnet:
            model.img_encoder.tap_log, model.decoder.tap_log = None, None
        mu_t, _, _, contra_t = model(cx.to(DEV), cy.to(DEV), qx.to(DEV), qy.to(DEV), test=True)
    assert contra_t == 0 and U.rel_err(mu_t, fx["mu"]) <= U.RTOL


def test_staged_eps_step_equals_lazy_step_and_captures(gpulib):
    """networks/bbb/eps.py on the device: a Bayes-by-backprop step fed from the pre-drawn eps buffer is bit-identical to the
    reference's lazy per-layer draws, and the staged step replays from a hipGraph with the same result."""
    from networks.bbb.eps import StagedEps
    fx, meta = U.load_case("r_anpmr_shapenet3d")
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = (t.to(DEV) for t in U.resnet_case_inputs(meta, fx))
    from trainer.losses import LossFunc
    loss_fn = LossFunc("mse", "shapenet_3d")

    def step():
        model.zero_grad(set_to_none=True)
        mu, _, kl = model(cx, cy, qx)
        (loss_fn.calc_loss(mu, None, qy) + 1e-7 * kl).backward()
        # detached: a kept autograd graph would pin the parameters' gradient-accumulation nodes to THIS step's stream,
        # and the capture below must not meet nodes created on the default stream
        return mu.detach(), kl.detach()

    st = StagedEps(DEV)
    torch.manual_seed(99)
    with st.recording():
        mu0, kl0 = step()
    g0 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert U.rel_err(mu0, fx["mu"]) <= U.RTOL              # the lazy route is the one pinned to the reference vectors
    torch.manual_seed(99)
    st.stage()
    with st.active():
        mu1, kl1 = step()
    assert torch.equal(mu0, mu1) and torch.equal(kl0, kl1)
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g0[k]), k
    # capture, then replay with the same draws
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), st.active():
        for _ in range(2):
            st.stage()
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    st.stage()
    from mlhot.graphs import capture
    with st.active(), capture(graph, None):
        mu2, kl2 = step()
    torch.manual_seed(99)
    st.stage()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mu2, mu0) and torch.equal(kl2, kl0)
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g0[k]), k


@pytest.mark.parametrize("name", U.mr_case_names())
def test_mr_vanilla_models_vs_reference(gpulib, name):
    """ANPMR / ANPMRShapeNet1D / CNPMR / CNPMRShapeNet1D: Bayes-by-backprop vanilla encoder whose sampled weights
    run the E1 kernels.  Same eps draws as the reference (torch.manual_seed(99) before the forward): mu / kl / loss at
    1e-4 against the reference's vectors; every gradient of loss + 1e-7*kl at 1e-4 against the oracle under the same draws
    and the encoder kernels' own routing (conv1 sign bits, pool arg-max, ReLU masks; each difference proven a tie), and
    against the reference's gradients when no decision differs."""
    from mlhot import ops
    from trainer.losses import LossFunc
    fx, meta = U.load_case(name)
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, qy = U.resnet_case_inputs(meta, fx)
    torch.manual_seed(99)
    ops.saved_taps = []
    try:
        mu, var, kl = model(cx.to(DEV), cy.to(DEV), qx.to(DEV))
    finally:
        taps, ops.saved_taps = ops.saved_taps, None
    assert var is None
    loss = LossFunc("mse", meta["cfg"]["task"]).calc_loss(mu, var, qy.to(DEV))
    (loss + 1e-7 * kl).backward()
    assert U.rel_err(mu, fx["mu"]) <= U.RTOL
    assert abs(kl.item() - float(fx["kl"])) <= U.RTOL * float(fx["kl"])
    assert abs(loss.item() - float(fx["loss"])) <= U.RTOL * max(1.0, abs(float(fx["loss"])))
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert len(taps) == 2 and all(t[0] == "enc" for t in taps)          # two encoder calls, in the reference's order
    routes = [gpulib.enc_routes(saved, n) for _, n, saved in taps]
    p = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
    pres = []
    torch.manual_seed(99)
    mu_o, kl_o = O.vanilla_mr_forward(p, cx, cy, qx, meta["cfg"]["agg_mode"], attention=meta["method"].startswith("ANP"),
                                      tanh=meta["method"].endswith("ShapeNet1D"), routes=routes, pres=pres)
    (O.calc_loss(meta["cfg"]["task"], mu_o, qy) + 1e-7 * kl_o).backward()
    assert U.rel_err(mu, mu_o) <= U.RTOL
    flips = sum(U.encoder_flips(r, q, "encoder call") for r, q in zip(routes, pres))
    gmax = max(p[k].grad.abs().max().item() for k, _ in model.named_parameters() if p[k].grad is not None)
    for k, prm in model.named_parameters():
        if p[k].grad is None:
            assert grads[k] is None, k       # task_encoder / mu / decoder.* never receive a gradient
            continue
        assert U.rel_err(grads[k], p[k].grad, floor=U.GRAD_FLOOR * gmax) <= U.RTOL, k
    def effect():
        p2 = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "projection" not in k) for k, v in model.state_dict().items()}
        torch.manual_seed(99)
        mu2, kl2 = O.vanilla_mr_forward(p2, cx, cy, qx, meta["cfg"]["agg_mode"], attention=meta["method"].startswith("ANP"), tanh=meta["method"].endswith("ShapeNet1D"))
        (O.calc_loss(meta["cfg"]["task"], mu2, qy) + 1e-7 * kl2).backward()
        return U.flip_effect({k: p[k].grad for k, _ in model.named_parameters()}, {k: p2[k].grad for k, _ in model.named_parameters()}, U.GRAD_FLOOR * gmax)
    U.check_grads_against_fixture_flipped(grads, fx, meta, flips, name, effect=effect, head=1024, stride_cap=4096)



# ---- E2 / D2 / B1 trunk kernels in isolation (csrc/resnet_ws.h, resnet_trunk.h) -----------------------------------------
def _trunk_dict(ws):
    d = {"t.conv1.weight": ws[0], "t.conv1.bias": ws[1]}
    for i in range(4):
        q = f"t.resnet.layer{i + 1}.0."
        for j, name in enumerate(("conv1", "conv2", "downsample.0")):
            d[q + name + ".weight"], d[q + name + ".bias"] = ws[2 + 6 * i + 2 * j], ws[3 + 6 * i + 2 * j]
    return d


# (C, H, skip_k, images per pass, one shared weight set?) under the names these cases have always had
_TRUNK_CASES = [(3, 64, 3, (5,), False), (3, 64, 1, (7, 3), True), (3, 64, 3, (33, 2, 9), False),
                (1, 128, 1, (3,), False), (1, 128, 1, (2, 5), True), (3, 64, 1, (120,), False),
                # production-sized image counts for the 1 x 128 x 128 (Distractor) geometries: thousands
                # of bands per launch, so the band loops (band += workgroups), the multi-band
                # weight-gradient slab rows and the stem / 1x1-skip row splitting all run
                (1, 128, 1, (96, 40), True), (1, 128, 3, (70,), False)]


def _trunk_params():
    """The eight cases above (one skip kernel for every weight set, default options), then the route's cases of
    tests/test_trunk_route_gpu.py (a skip kernel per weight set, options away from their defaults)."""
    from tests.test_trunk_route_gpu import CASES
    out = [pytest.param(C, H, (k,) * (1 if share else len(ns)), ns, share, {}, id=f"{C}-{H}-{k}-ns{i}-{share}")
           for i, (C, H, k, ns, share) in enumerate(_TRUNK_CASES)]
    return out + [pytest.param(*case, id=name) for name, case in CASES.items()]


@pytest.mark.parametrize("C,H,skips,ns,share,opts", _trunk_params())
def test_resnet_trunk_fwd_bwd_vs_torch(gpulib, C, H, skips, ns, share, opts):
    """mlhot_trunk_fwd / _bwd: several passes in one call (ragged image counts that end in partial bands; passes that share a
    weight set; the 1x1 and the 3x3 skip convolution, also side by side in one call; both supported image geometries; the trunk's
    options away from their defaults) against torch's conv2d + autograd on the CPU.
    Every saved activation at 1e-5; gradients at 1e-4 with the reference evaluated under the kernels' ReLU routing (each
    differing decision proven a tie)."""
    from tests.test_trunk_route_gpu import _with_options
    g = torch.Generator().manual_seed(C * 1000 + H + sum(ns))
    imgs = [torch.rand(n, C, H, H, generator=g) for n in ns]
    wsets = [_trunk_weights(C, k, 1 + i) for i, k in enumerate(skips)]
    passes = [(i, 0 if share else i) for i in range(len(ns))]
    imgs_d = [t.to(DEV) for t in imgs]
    wsets_d = [([t.to(DEV) for t in ws], k) for ws, k in zip(wsets, skips)]
    dfeats = [torch.randn(n, 64, H // 32, H // 32, generator=g) for n in ns]

    def run():
        acts = gpulib.trunk_fwd([(imgs_d[i], w) for i, w in passes], wsets_d)
        return acts, gpulib.trunk_bwd([(imgs_d[i], w, acts[pi]) for pi, (i, w) in enumerate(passes)], wsets_d, [d.to(DEV) for d in dfeats])
    acts, grads = _with_options(gpulib, opts, run)
    # reference under the kernels' routing
    ref_w = [[t.clone().requires_grad_() for t in ws] for ws in wsets]
    flips = 0
    for pi, (i, w) in enumerate(passes):
        route = [(a.cpu() > 0).float() for a in acts[pi]]
        pre = []
        out = O.resnet_features(imgs[i], _trunk_dict(ref_w[w]), "t.", "reshape", skip_pad=1 if skips[w] == 3 else 0, route=route, pre=pre)
        assert U.rel_err(acts[pi][8].reshape(ns[pi], -1), out) <= 1e-5, pi
        flips += sum(U.relu_flips(m, v, f"pass {pi}") for m, v in zip(route, pre))
        (out * dfeats[pi].reshape(ns[pi], -1)).sum().backward()
    gmax = max(t.grad.abs().max().item() for ws in ref_w for t in ws)
    for w, ws in enumerate(ref_w):
        for k, t in enumerate(ws):
            assert U.rel_err(grads[w][k], t.grad, floor=U.GRAD_FLOOR * gmax) <= U.RTOL, (w, k)


# ---- B1 in isolation: sample + KL and their backward against torch autograd ------------------------------------
@pytest.mark.parametrize("shape", [(7,), (64, 3, 5, 5), (64, 64, 3, 3), (64, 4096)])
@pytest.mark.parametrize("dkl", [0.0, 1e-7, 0.3])
def test_bbb_sample_fwd_bwd_vs_autograd(gpulib, shape, dkl):
    """mlhot_bbb_sample_fwd / _bwd (one tensor): w, kl, d mu, d rho - with and without a KL gradient."""
    g = torch.Generator().manual_seed(len(shape) * 100 + shape[0])
    mu, rho = torch.randn(*shape, generator=g) * 0.1, torch.randn(*shape, generator=g) * 0.5 - 3.0
    eps, wout = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    (w_r,), kl_r, (dmu_r,), (drho_r,) = _bbb_ref([mu], [rho], [eps], [wout], dkl)
    mud, rhod, epsd = dev(mu, rho, eps)
    w, kl = gpulib.bbb_sample_fwd(mud, rhod, epsd)
    assert U.rel_err(w, w_r) <= 1e-6 and abs(kl.item() - kl_r.item()) <= 1e-5 * abs(kl_r.item())
    dmu, drho = gpulib.bbb_sample_bwd(mud, rhod, epsd, wout.to(DEV), torch.tensor(dkl, device=DEV))
    assert U.rel_err(dmu, dmu_r) <= 1e-5 and U.rel_err(drho, drho_r) <= 1e-5


@pytest.mark.parametrize("dkl", [0.0, 1e-7, 0.3])
def test_bbb_sample_multi_fwd_bwd_vs_autograd(gpulib, dkl):
    """mlhot_bbb_sample_multi_fwd / _bwd: 32 tensors of the shapes of one ANPMRShapeNet3D encoder pass (+ ragged extras) in one
    launch pair; some samples receive NO gradient (dw = NULL: only the KL path reaches mu / rho); a 33rd tensor is refused."""
    from mlhot.binding import MlhotError
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 3, 5, 5), (64,)] + [(64, 64, 3, 3), (64,)] * 12 + [(1,), (5, 3), (1023,), (4, 4097), (2, 2, 2), (3,)]
    assert len(shapes) == 32
    mus = [torch.randn(*s_, generator=g) * 0.1 for s_ in shapes]
    rhos = [torch.randn(*s_, generator=g) * 0.5 - 3.0 for s_ in shapes]
    epss = [torch.randn(*s_, generator=g) for s_ in shapes]
    wouts = [None if i % 5 == 3 else torch.randn(*s_, generator=g) for i, s_ in enumerate(shapes)]
    ws_r, kl_r, dmu_r, drho_r = _bbb_ref(mus, rhos, epss, wouts, dkl)
    md, rd, ed = dev(*mus), dev(*rhos), dev(*epss)
    ws, kl = gpulib.bbb_sample_multi_fwd(md, rd, ed)
    assert abs(kl.item() - kl_r.item()) <= 1e-5 * abs(kl_r.item())
    for a, b in zip(ws, ws_r):
        assert U.rel_err(a, b) <= 1e-6
    dmus, drhos = gpulib.bbb_sample_multi_bwd(md, rd, ed, dev(*wouts), torch.tensor(dkl, device=DEV))
    for i in range(32):
        if dkl == 0.0 and wouts[i] is None:
            assert float(dmus[i].abs().max()) == 0.0 and float(drhos[i].abs().max()) == 0.0
            continue
        assert U.rel_err(dmus[i], dmu_r[i]) <= 1e-5 and U.rel_err(drhos[i], drho_r[i]) <= 1e-5, i
    with pytest.raises(MlhotError):
        gpulib.bbb_sample_multi_fwd(md + md[:1], rd + rd[:1], ed + ed[:1])


def test_bbb_two_samples_in_one_launch_vs_autograd(gpulib):
    """The optional second sample of mlhot_bbb_sample_multi (context / target pass of the Bayes-by-backprop encoder): w, w2, one KL,
    and d mu / d rho with both samples' gradients folded in one pass; a sample without gradient (dw2 = NULL) contributes nothing."""
    g = torch.Generator().manual_seed(9)
    shapes = [(64, 3, 5, 5), (64,), (64, 64, 3, 3), (7,)]
    mus = [torch.randn(*s_, generator=g) * 0.1 for s_ in shapes]
    rhos = [torch.randn(*s_, generator=g) * 0.5 - 3.0 for s_ in shapes]
    e1 = [torch.randn(*s_, generator=g) for s_ in shapes]
    e2 = [torch.randn(*s_, generator=g) for s_ in shapes]
    o1 = [torch.randn(*s_, generator=g) for s_ in shapes]
    o2 = [torch.randn(*s_, generator=g) if i != 2 else None for i, s_ in enumerate(shapes)]
    mr = [(m.clone().requires_grad_(), r.clone().requires_grad_()) for m, r in zip(mus, rhos)]
    total, kl_r, w1_r, w2_r = 0.0, 0.0, [], []
    for (m, r), a, b, oa, ob in zip(mr, e1, e2, o1, o2):
        sigma = torch.log1p(torch.exp(r))
        w1_r.append(m + a * sigma); w2_r.append(m + b * sigma)
        kl_r = kl_r + 0.5 * (2 * torch.log(sigma / 0.1) - 1 + (0.1 / sigma).pow(2) + (m / sigma).pow(2)).sum()
        total = total + (w1_r[-1] * oa).sum() + ((w2_r[-1] * ob).sum() if ob is not None else 0.0)
    (total + 0.2 * kl_r).backward()
    md, rd = dev(*mus), dev(*rhos)
    ws, ws2, kl = gpulib.bbb_sample_multi_fwd(md, rd, dev(*e1), dev(*e2))
    assert abs(kl.item() - kl_r.item()) <= 1e-5 * abs(kl_r.item())
    for a, b, c, d_ in zip(ws, w1_r, ws2, w2_r):
        assert U.rel_err(a, b) <= 1e-6 and U.rel_err(c, d_) <= 1e-6
    dmus, drhos = gpulib.bbb_sample_multi_bwd(md, rd, dev(*e1), dev(*o1), torch.tensor(0.2, device=DEV), dev(*e2), dev(*o2))
    for i, (m, r) in enumerate(mr):
        assert U.rel_err(dmus[i], m.grad) <= 1e-5 and U.rel_err(drhos[i], r.grad) <= 1e-5, i


def test_bbb_sample_all_more_than_32_tensors_through_autograd(gpulib):
    """networks.bbb.misc.sample_all over 20 layers (40 tensors: two launch pairs) through torch autograd, under the reference's
    draw order (layer by layer, weight then bias, on the CPU generator): samples, total KL and all 80 gradients."""
    from networks.bbb.BBBConv import BBBConv2d
    from networks.bbb.misc import sample_all
    torch.manual_seed(3)
    layers = [BBBConv2d(4 + i % 3, 6, kernel_size=3, padding=1).to(DEV) for i in range(20)]
    g = torch.Generator().manual_seed(8)
    wouts = [(torch.randn(l.W_mu.shape, generator=g), torch.randn(l.bias_mu.shape, generator=g)) for l in layers]
    torch.manual_seed(17)
    kl = sample_all(layers)
    total = 0.3 * kl
    got_w = []
    for l, (wo, bo) in zip(layers, wouts):
        (w, b), l.presampled = l.presampled, None
        got_w += [w, b]
        total = total + (w * wo.to(DEV)).sum() + (b * bo.to(DEV)).sum()
    total.backward()
    torch.manual_seed(17)
    mus, rhos, epss, wo_flat = [], [], [], []
    for l, (wo, bo) in zip(layers, wouts):
        for prm_mu, prm_rho, o in ((l.W_mu, l.W_rho, wo), (l.bias_mu, l.bias_rho, bo)):
            mus.append(prm_mu.detach().cpu()); rhos.append(prm_rho.detach().cpu()); wo_flat.append(o)
            epss.append(torch.empty(prm_mu.size()).normal_(0, 1))
    ws_r, kl_r, dmu_r, drho_r = _bbb_ref(mus, rhos, epss, wo_flat, 0.3)
    assert abs(kl.item() - kl_r.item()) <= 1e-5 * abs(kl_r.item())
    i = 0
    for l in layers:
        for prm_mu, prm_rho in ((l.W_mu, l.W_rho), (l.bias_mu, l.bias_rho)):
            assert U.rel_err(got_w[i], ws_r[i]) <= 1e-6
            assert U.rel_err(prm_mu.grad, dmu_r[i]) <= 1e-5 and U.rel_err(prm_rho.grad, drho_r[i]) <= 1e-5, i
            i += 1


def _ulps(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai, bi = np.where(ai < 0, -(ai & 0x7fffffff), ai), np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


@pytest.mark.parametrize("parallel", [64, 8, 1], ids=["jump_ahead_64_substreams", "jump_ahead_8_substreams", "one_workgroup"])
@pytest.mark.parametrize("seed", [0, 99])
def test_device_normal_continues_the_cpu_generator(gpulib, seed, parallel):
    """mlhot_mt19937_normal (mlhot.rng.DeviceNormal): the torch CPU generator's stream continued on the device.  Against the
    same `torch.empty(n).normal_()` calls on the CPU: 1.3 M draws across tensor sizes that are / are not multiples of 16 (16, 33,
    100, odd, the c5 model's conv shapes), from a mid-block engine position, two consecutive steps; every normal within 6 ulp of
    torch's - measured: 4 - (the uniforms behind them are bit-identical - a single differing uniform would be a different number altogether),
    and after hand_back() the CPU generator continues EXACTLY where the CPU-only sequence would be."""
    from mlhot.rng import DeviceNormal
    sizes = [16, 33, 64, 100, 4800, 36864, 1000003, 64 * 4096, 48, 17]
    torch.manual_seed(seed)
    torch.rand(5)
    s0 = torch.get_rng_state()
    ref = [[torch.empty(n).normal_(0, 1) for n in sizes] for _ in range(2)]
    after_ref = torch.rand(7)
    torch.set_rng_state(s0)
    dn = DeviceNormal(DEV, sizes, sub_streams=parallel)   # K MT19937 sub-streams positioned by jump-ahead polynomials (mlhot/mt_jump.py)
    assert (dn._polys is not None) == (parallel > 1)
    dn.take_over()
    worst = 0
    for step in range(2):
        flat = dn.draw()
        for r, o, n in zip(ref[step], dn.offsets, sizes):
            got = flat[o:o + n].cpu().numpy()
            d = _ulps(got, r.numpy())
            worst = max(worst, int(d.max()))
            assert d.max() <= 6, (step, n, int(d.max()))
    dn.hand_back()
    assert torch.equal(torch.rand(7), after_ref)
    print(f"device normal_ stream, seed {seed}: {2 * sum(sizes)} draws, worst difference {worst} ulp; generator state handed back bit-exact")


def test_staged_eps_device_source_vs_host_source(gpulib):
    """StagedEps(source="device"): ANPMRShapeNet3D steps fed from the device-side continuation of the CPU generator against the
    same steps fed by the host draws: eps within 6 ulp, mu / kl / every gradient within 1e-5 (the 1e-4 parity bar of the model
    against the reference therefore holds with either source), over three consecutive steps (the look-ahead draw, the double
    buffer); release() leaves the CPU generator exactly where the host-only run leaves it."""
    from networks.bbb.eps import StagedEps
    from trainer.losses import LossFunc
    fx, meta = U.load_case("r_anpmr_shapenet3d")
    cx, qx, cy, qy = (t.to(DEV) for t in U.resnet_case_inputs(meta, fx))
    results = {}
    for source in ("host", "device"):
        model = U.build_model(meta, DEV, fx=fx).to(DEV)
        torch.manual_seed(99)
        eps = StagedEps(DEV, source=source)

        def step():
            model.zero_grad(set_to_none=True)
            mu, var, kl = model(cx, cy, qx)
            (LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy) + 1e-7 * kl).backward()
            return mu.detach().clone(), kl.detach().clone()
        with eps.recording():
            step()                                         # lazy draws: consumes one step of the stream in both runs
        outs = []
        for _ in range(3):
            eps.stage()
            with eps.active():
                mu, kl = step()
            outs.append((eps._dev.clone(), mu, kl, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
        if source == "device":
            eps.release()
        torch.cuda.synchronize()
        results[source] = (outs, torch.rand(4))
    assert torch.equal(results["host"][1], results["device"][1])          # the CPU generator continues identically
    for (eh, muh, klh, gh), (ed, mud, kld, gd) in zip(results["host"][0], results["device"][0]):
        assert _ulps(ed.cpu().numpy(), eh.cpu().numpy()).max() <= 6
        assert U.rel_err(mud, muh) <= 1e-5 and abs(kld.item() - klh.item()) <= 1e-6 * abs(klh.item())
        for k in gh:
            assert U.rel_err(gd[k], gh[k], floor=1e-3 * float(gh[k].abs().max()) + 1e-12) <= 1e-3, k
    # and the first host-fed step is the reference's own (the fixture): the device-fed one within the parity bar
    assert U.rel_err(results["device"][0][0][1], results["host"][0][0][1]) <= U.RTOL


@pytest.mark.parametrize("N,d,div,mod", [(32, 64, 1, 16), (6, 256, 1, 3), (120, 256, 15, 8), (300, 256, 15, 20), (45, 64, 5, 9),
                                         (7, 16, 7, 1), (10, 32, 1, 10), (512, 128, 16, 32),
                                         (580, 256, 29, 20),      # FCLANP's own configuration at its largest: 20 tasks x (30 - 1) views (> 512 rows)
                                         (2048, 64, 64, 32)])     # the kernels' limit: 156 KB of LDS per workgroup
def test_nt_xent_kernel_vs_definition(gpulib, N, d, div, mod):
    """mlhot_nt_xent_fwd / _bwd (trainer/losses.py:82-99): value against the pair-by-pair definition in python floats / float64
    (the published NTXentLoss algorithm; the package itself is absent, so this is what pins the term) at 1e-6, gradient against
    float64 autograd of the same definition at 1e-4.  Shapes: both label structures (pairs: label = row % T; blocks: label =
    row // Nq), row counts that are not multiples of 16, a single group (no negatives: loss and gradient are exactly 0), all
    groups of size one (no positives: 0), the largest supported size."""
    import math
    from trainer.losses import nt_xent
    t = 0.07
    g = torch.Generator().manual_seed(N * 1000 + d)
    z = torch.randn(N, d, generator=g) * (1.0 + torch.rand(N, 1, generator=g))
    labels = [(i // div) % mod for i in range(N)]
    zd = z.double().requires_grad_()
    zn = zd / zd.norm(dim=1, keepdim=True).clamp_min(1e-12)
    sim = zn @ zn.t() / t
    terms = []
    if N <= 512:
        for a in range(N):
            neg = [k for k in range(N) if labels[k] != labels[a]]
            if not neg:
                continue
            for p_ in range(N):
                if p_ == a or labels[p_] != labels[a]:
                    continue
                m = max(sim[a, p_].item(), sim[a, neg].max().item())
                num = torch.exp(sim[a, p_] - m)
                terms.append(-torch.log(num / (torch.exp(sim[a, neg] - m).sum() + num) + torch.finfo(torch.float32).tiny))
    else:
        # the same definition as float64 tensor arithmetic (580 x 28 and 2048 x 63 positive pairs are too many autograd nodes one by
        # one): per anchor the negatives' maximum and exp-sum, per positive pair m = max(s_ap, negmax_a) treated as a constant
        lab = torch.tensor(labels)
        same = lab[:, None] == lab[None, :]
        pos = same & ~torch.eye(N, dtype=torch.bool)
        negmax = sim.masked_fill(same, float("-inf")).max(dim=1).values.detach()
        m = torch.maximum(sim.detach(), negmax[:, None])
        num = torch.exp(sim - m)
        # sum_n exp(s_an - m_ap) = E_a exp(negmax_a - m_ap), E_a = sum_n exp(s_an - negmax_a)   (O(N^2) instead of O(N^3))
        E = (torch.exp(sim - negmax[:, None]) * ~same).sum(dim=1)
        negsum = E[:, None] * torch.exp(negmax[:, None] - m)
        per = -torch.log(num / (negsum + num) + torch.finfo(torch.float32).tiny)
        terms = [per[pos]]
    zg = z.to(DEV).requires_grad_()
    loss = nt_xent(zg, div, mod, t)
    loss.backward()
    if not terms:
        assert loss.item() == 0.0 and float(zg.grad.abs().max()) == 0.0
        return
    want = (torch.stack(terms) if N <= 512 else terms[0]).mean()
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item())), (loss.item(), want.item())
    assert U.rel_err(zg.grad, zd.grad) <= U.RTOL
    if N <= 32:                                    # python floats, term by term
        s = sim.detach()
        tot, cnt = 0.0, 0
        for a in range(N):
            neg = [k for k in range(N) if labels[k] != labels[a]]
            for p_ in range(N):
                if neg and p_ != a and labels[p_] == labels[a]:
                    m = max([s[a, p_].item()] + [s[a, k].item() for k in neg])
                    num = math.exp(s[a, p_].item() - m)
                    tot += -math.log(num / (sum(math.exp(s[a, k].item() - m) for k in neg) + num))
                    cnt += 1
        assert abs(loss.item() - tot / cnt) <= 1e-6 * max(1.0, tot / cnt)


def test_flat_adam_matches_torch_adam(gpulib):
    """mlhot.optim.FlatAdam (parameters re-pointed into ONE flat buffer laid out like the library's
    flat gradient buffer; one mlhot_adam_step launch) against torch.optim.Adam on an identically seeded model, 3 steps.
    On the parameter (of order 0.1, lr 1e-3) 1e-5 passes an update that is wrong by percents, so the MOVEMENT is held as well, by
    tests/flat_adam_cases.py's rule: a float64 torch.optim.Adam on CPU copies takes the same gradients, e32 is the error of the fp32
    torch.optim.Adam's movement against it (relative to the largest entry of the movement, over all parameters), and FlatAdam's may be
    4 x e32."""
    from mlhot.optim import FlatAdam
    from tests.flat_adam_cases import MARGIN
    from trainer.losses import LossFunc
    fx, meta = U.load_case("s_anp_shapenet1d_ragged")
    cx, qx, cy, qy = (t.to(DEV) for t in U.case_inputs(meta))
    models = [U.build_model(meta, DEV, fx=fx).to(DEV) for _ in range(2)]
    ref_opt = torch.optim.Adam(models[0].parameters(), lr=1e-3)
    first = [p.detach().double().cpu().clone() for p in models[0].parameters()]
    p64 = [torch.nn.Parameter(p.clone()) for p in first]
    opt64 = torch.optim.Adam(p64, lr=1e-3)
    flat_opt = FlatAdam(models[1], lr=1e-3, ctx_num=meta["Nc"], test_num=meta["Nq"])
    storages = {p.untyped_storage().data_ptr() for p in models[1].parameters()}
    assert len(storages) == 1                                  # every parameter is a view of the one flat tensor
    loss_fn = LossFunc("mse", meta["cfg"]["task"])
    for _ in range(3):
        for model, opt in zip(models, (ref_opt, flat_opt)):
            opt.zero_grad(set_to_none=True)
            loss_fn.calc_loss(model(cx, cy, qx)[0], None, qy).backward()
        grads = [p.grad for p in models[1].parameters()]
        assert len({g.untyped_storage().data_ptr() for g in grads}) == 1     # backward wrote ONE flat gradient buffer
        # Some gradients are pure rounding residue (the key bias cancels inside the attention normaliser) and Adam turns
        # residue into +-lr updates, so two runs drift apart chaotically.  What is under test is the optimizer: give both
        # the SAME gradient values (in place, the flat buffer stays the flat buffer).
        with torch.no_grad():
            for p0, p1 in zip(models[0].parameters(), models[1].parameters()):
                p1.grad.copy_(p0.grad)
        for q, p0 in zip(p64, models[0].parameters()):
            q.grad = p0.grad.detach().double().cpu()
        ref_opt.step()
        flat_opt.step()
        opt64.step()
    for (k, a), (_, b) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert U.rel_err(b, a) <= 1e-5, k
    moved = [torch.cat([(p.detach().double().cpu() - f).reshape(-1) for p, f in zip(ps, first)])
             for ps in (p64, models[0].parameters(), models[1].parameters())]
    e32, got = U.rel_err(moved[1], moved[0]), U.rel_err(moved[2], moved[0])
    print(f"[flat_adam] parity model, 3 steps, movement: e32 {e32:.3e} got {got:.3e} ({got / e32:.2f}x)")
    assert moved[0].abs().max() > 1e-3 and got <= MARGIN * e32
    assert set(models[1].state_dict().keys()) == set(models[0].state_dict().keys())


def test_conv_embedding_model_vs_reference(gpulib):
    """X1: ConvEmbeddingModel (MMAML task embedding) on one task's shots: the four embedding vectors, every
    gradient and the in-place running-stat update against the reference's vectors."""
    fx = np.load(os.path.join(U.GOLDEN, "conv_embedding.npz"))
    meta = json.loads(str(fx["meta"]))
    from networks.conv_embedding_model import ConvEmbeddingModel
    torch.manual_seed(meta["seed"])
    model = ConvEmbeddingModel(input_size=128 * 128, output_size=2, embedding_dims=[64, 128, 256, 512], hidden_size=128,
                               num_layers=2, convolutional=True, num_conv=4, num_channels=32, rnn_aggregation=False,
                               linear_before_rnn=False, embedding_pooling="avg", batch_norm=True, avgpool_after_conv=True,
                               img_size=(1, 128, 128))
    for k, v in model.state_dict().items():
        assert U.sha(v) == meta["state_sha"][k], k
    assert model.to(DEV) is model
    x = torch.rand(6, 1, 128, 128, generator=torch.Generator().manual_seed(meta["input_seed"]))
    embs = model(x.to(DEV))
    for i, e in enumerate(embs):
        assert U.rel_err(e, fx[f"emb{i}"]) <= U.RTOL
    sum((e * (i + 1)).sum() for i, e in enumerate(embs)).backward()
    grads = dict(model.named_parameters())
    gmax = max(float(np.abs(fx[k]).max()) for k in fx.files if k.startswith("grad/"))
    for k in fx.files:
        if k.startswith("grad/"):
            got = grads[k[5:]].grad
            if k.startswith("grad/conv.conv") and k.endswith(".bias"):      # analytically zero (bias before a batch norm)
                assert got.abs().max().item() <= 1e-4 * gmax
                continue
            assert U.rel_err(got, fx[k], floor=U.GRAD_FLOOR * gmax) <= U.RTOL, k
        if k.startswith("after/"):
            assert U.rel_err(model.state_dict()[k[6:]], fx[k]) <= U.RTOL, k


def test_forward_is_deterministic_and_task_independent(gpulib):
    """Size-independent properties at the full c3 size: bitwise run-to-run determinism, and
    (tasks are independent apart from the FAVOR+ global key stabiliser) a task's output does not
    depend on the other tasks of the batch beyond 1e-6."""
    fx, meta = U.load_case("c3_anp_shapenet1d")
    model = U.build_model(meta, DEV, fx=fx).to(DEV)
    cx, qx, cy, _ = (t.to(DEV) for t in U.case_inputs(meta))
    with torch.no_grad():
        a = model(cx, cy, qx)[0]
        b = model(cx, cy, qx)[0]
        assert torch.equal(a, b)
        perm = torch.arange(15, -1, -1, device=DEV)
        c = model(cx[perm].contiguous(), cy[perm].contiguous(), qx[perm].contiguous())[0]
        assert U.rel_err(c[perm], a) <= 1e-6


def test_model_trainer_loop_on_synthetic_data(gpulib, tmp_path, monkeypatch):
    """T1: the reference's train / validate loop (trainer/model_trainer.py:33-139) end to end on the HIP path,
    with the reference's random context size per iteration (3..15 shots) and Adam."""
    import types
    from mlhot.synth import SyntheticData
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=4, input_dim=3,
                                output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                dim_z=64, task="shapenet_1d", iterations=6, val_freq=3, val_iters=2, bg_gen_freq=1000, gen_bg=False,
                                max_ctx_num=15, beta=0, contrastive=False, save_path=str(tmp_path / "run"), logger=None)
    model = ANPShapeNet1D(cfg).to(cfg.device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    trainer = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=opt, config=cfg, data=SyntheticData())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    trainer.train()
    assert os.path.exists(tmp_path / "run" / "models" / "model_end_6.pt")
    assert os.path.exists(tmp_path / "run" / "models" / "best_validation_model.pt")
    moved = sum(float((v - before[k]).abs().sum()) for k, v in model.state_dict().items() if "projection" not in k)
    assert moved > 0 and all(torch.isfinite(v).all() for v in model.state_dict().values())


class _FixedBatches:
    """A data source with the reference's `get_batch` contract (dataset/shapenet_1d.py:113-196) that hands out a prepared list of
    meta-batches in order: the HIP trainer and the oracle loop of the trajectory tests see the same draws."""

    def __init__(self, batches):
        self.batches, self.i, self.test_counter = batches, 0, 0

    def gen_bg(self, config, data="all"):
        pass

    def get_batch(self, source, tasks_per_batch, shot):
        b = self.batches[self.i]
        self.i += 1
        return b


def _to_dtype(x, dtype):
    """Floating tensors anywhere inside nested dicts / lists / tuples cast to `dtype`; everything else as it is."""
    if isinstance(x, torch.Tensor):
        return x.to(dtype) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: _to_dtype(v, dtype) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_dtype(v, dtype) for v in x)
    return x


def _trajectory_check(model, p0, oracle_step, batches, make_opt, cfg, tmp_path, what, grab_routes, lr=1e-3, seed_eps=None, trainer_out=None,
                      oracle_dtype=torch.float64):
    """T1 (trainer/model_trainer.py:59-93: zero_grad -> forward -> calc_loss + kl * beta -> backward -> optimizer.step): k
    iterations of ModelTrainer on the HIP path against k iterations of the CPU oracle + autograd + torch.optim.Adam on the same
    draws.  Per-iteration loss at 1e-4; final weights at 1e-4 of each tensor's scale.  The oracle runs in `oracle_dtype`, fp64 by
    default (same initial weights, inputs, eps values and routing): an fp32 CPU trajectory carries rounding noise of its own that
    depends on the host's thread count and comes within a factor of two of the tolerance, so the kernels are held to 1e-4 of the
    exact trajectory instead, as _anpmr3d_routed_check does at c5's full size.

    Two things make a naive comparison of two fp32 training runs meaningless, and both are handled the way the rest of this file
    handles them.  (1) ReLU / max-pool routing: with 20 images ONE rounding-level tie that falls the other way moves a conv
    gradient by ~1e-2 of its scale, so the oracle's iteration i runs under the routing decisions the kernels took in THEIR
    iteration i (`grab_routes`, read from the forward's saved buffers), and every decision that differs from the oracle's own
    must sit on a tie of the oracle's pre-activations: |pre| <= 1e-5 of the layer's largest in the first iteration (equal
    weights), later within the band that the weight difference ENTERING the iteration explains (50 x the largest relative
    weight difference, measured, see (2); never below 1e-5).  (2) Adam normalises every element's update to ~lr whatever the
    gradient's size, so an element whose gradient is rounding residue (below RESIDUE of its tensor's largest entry, or a tensor
    whose largest entry is below 1e-4 of the model's largest - the key bias cancels inside the attention normaliser - in some
    iteration: its SIGN differs between any two fp32 evaluation orders, in the reference too) random-walks by +-lr per step in
    both runs; those elements are held to the walk's bound 2 * lr * k instead, and their share is printed."""
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    RESIDUE = 1e-4
    k = len(batches)
    names = [n for n, _ in model.named_parameters()]
    # ---- the HIP trainer's trajectory (recording each iteration's routing and the weights entering it)
    cfg.iterations, cfg.val_freq, cfg.val_iters, cfg.bg_gen_freq, cfg.gen_bg = k, 10 ** 6, 1, 10 ** 6, False
    cfg.save_path, cfg.logger, cfg.contrastive = str(tmp_path / what), None, False
    tr = ModelTrainer(model=model, loss=LossFunc("mse", cfg.task), optimizer=make_opt(model), config=cfg, data=_FixedBatches(list(batches)))
    if trainer_out is not None:
        trainer_out["trainer"] = tr
    losses, routes, entering = [], [], []
    orig = tr._train_iter

    def one_iteration(it):
        entering.append({n: prm.detach().cpu().clone() for n, prm in model.named_parameters()})
        with grab_routes(routes):
            orig(it)
    tr._train_iter = one_iteration
    orig_report = tr._report
    tr._report = lambda it, v: (losses.append(v), orig_report(it, v))[1]      # every iteration's loss, whichever call hands it out (the lagged log: one late)
    if seed_eps is not None:
        torch.manual_seed(seed_eps)
    tr.train()
    assert len(routes) == k
    # ---- the oracle's, under those decisions
    po = {n: _to_dtype(v.clone(), oracle_dtype).requires_grad_(n in names) for n, v in p0.items()}
    opt_o = torch.optim.Adam([po[n] for n in names], lr=lr)
    losses_o, small, flips, bands = [], {n: torch.zeros_like(po[n], dtype=torch.bool) for n in names}, [], []
    if seed_eps is not None:
        torch.manual_seed(seed_eps)
    for i, ((cx, qx, cy, qy), r) in enumerate(zip(batches, routes)):
        # (elements already known as residue-walkers are left out: they are the ones a flip may NOT hide behind)
        wdiff = max(float(((entering[i][n] - po[n].detach()).abs() * (~small[n])).max() / po[n].detach().abs().max()) for n in names)
        assert i > 0 or wdiff == 0.0
        bands.append(max(U.TIE, 50 * wdiff))
        opt_o.zero_grad()
        loss, f = oracle_step(po, *_to_dtype((cx, cy, qx, qy, r), oracle_dtype), bands[-1])
        flips.append(f)
        loss.backward()
        gmax = max(po[n].grad.abs().max().item() for n in names if po[n].grad is not None)
        for n in names:
            g = po[n].grad
            if g is not None:
                tmax = g.abs().max().item()
                small[n] |= ((g.abs() < RESIDUE * tmax) | (tmax < U.GRAD_FLOOR * gmax)) & (g != 0)   # an exact zero moves nothing
        opt_o.step()
        losses_o.append(loss.item())
    print(f"{what}: {k} iterations, losses {losses} (oracle {losses_o}); per iteration: tie band {['%.1e' % b for b in bands]}, "
          f"routing decisions inside it that differ from the oracle's own {flips}")
    for i, (a, b) in enumerate(zip(losses, losses_o)):
        assert abs(a - b) <= U.RTOL * max(1.0, abs(b)), f"{what}: iteration {i + 1} loss {a} vs oracle {b}"
    n_small = n_all = 0
    worst, fails = (0.0, None), []
    for n, prm in model.named_parameters():
        if po[n].grad is None:
            assert torch.equal(prm.detach().cpu(), p0[n]), n      # no gradient, no update (resnet.fc.*)
            continue
        a, b, m = prm.detach().cpu(), po[n].detach(), small[n]
        scale = b.abs().max().item()
        e = ((a - b).abs() * (~m)).max().item() / scale
        worst = max(worst, (e, n))
        if e > U.RTOL:
            fails.append(f"{n}: {e:.2e}")
        assert float(((a - b).abs() * m).max()) <= 2 * lr * k * 1.001, n
        n_small += int(m.sum())
        n_all += m.numel()
    print(f"{what}: worst weight error {worst[0]:.2e} of scale ({worst[1]}), {n_small} of {n_all} elements ({n_small / n_all:.2%}) "
          f"with residue-sized gradients held to the 2*lr*k bound")
    assert not fails, f"{what}: final weights differ by more than 1e-4 of scale: {fails}"
    return losses


@pytest.mark.parametrize("optimizer", ["torch_adam", "torch_adam_unpromoted", "flat_adam", "flat_adam_split"])
def test_trainer_trajectory_vs_oracle(gpulib, tmp_path, monkeypatch, optimizer, request):
    """ANPShapeNet1D, T = 2, fixed 5 + 5 shots, 4 training iterations of trainer.ModelTrainer against the oracle's forward + autograd +
    torch.optim.Adam (see _trajectory_check).  `torch_adam`: the reference's calling sequence as train.py writes it -
    ModelTrainer(model, loss, torch.optim.Adam(model.parameters(), lr), config, data) - which the trainer runs through its promoted
    defaults (round 5): FlatAdam.from_torch_adam, one eager iteration, then capture and hipGraph replays, host batches copied on the
    copy stream; asserted below.  `_unpromoted`: config.promote_optimizer = graph_steps = host_prefetch = False, the plain eager loop with torch's
    optimizer.  `flat_adam`: FlatAdam handed in, eager.  `_split`: the same with all three conv12 kernels on the bf16 pipe over split
    operands (csrc/conv_split.h), same tolerances."""
    unpromoted = optimizer.endswith("_unpromoted")
    if unpromoted:
        optimizer = optimizer[:-len("_unpromoted")]
    if optimizer.endswith("_split"):
        gpulib.set_option("conv2_split", 7)
        request.addfinalizer(lambda: gpulib.set_option("conv2_split", 0))
        optimizer = optimizer[:-len("_split")]
    import contextlib
    import types
    from mlhot import ops
    from mlhot.optim import FlatAdam
    from mlhot.synth import get_batch
    from networks.ANPShapeNet1D import ANPShapeNet1D
    monkeypatch.chdir(tmp_path)
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                dim_z=64, task="shapenet_1d", max_ctx_num=5, beta=0, ingest_u8=False)
    model = ANPShapeNet1D(cfg).to(cfg.device)
    p0 = {n: v.detach().cpu().clone() for n, v in model.state_dict().items()}
    batches = [get_batch("shapenet_1d", 2, 5, 5, seed=100 + i) for i in range(4)]

    @contextlib.contextmanager
    def grab_routes(out):
        ops.saved_taps = []
        try:
            yield
            out.append(_vanilla_routes(gpulib, ops.saved_taps, 2, 5, 5, "attention"))
        finally:
            ops.saved_taps = None

    def oracle_step(p, cx, cy, qx, qy, routes, tie):
        pres = {}
        mu = O.vanilla_np_forward(p, cx, cy, qx, "attention", tanh=True, routes=routes, pres=pres)
        return O.calc_loss("shapenet_1d", mu, qy), _vanilla_flips(routes, pres, tie)
    make = (lambda m: torch.optim.Adam(m.parameters(), lr=1e-3)) if optimizer == "torch_adam" else \
        (lambda m: FlatAdam(m, lr=1e-3, ctx_num=5, test_num=5))
    if unpromoted:
        cfg.promote_optimizer, cfg.graph_steps, cfg.host_prefetch = False, False, False
    elif optimizer == "flat_adam":
        cfg.graph_steps = False                          # a non-capturable FlatAdam: the eager loop
    seen = {}
    _trajectory_check(model, p0, oracle_step, batches, make, cfg, tmp_path, "anp_shapenet1d_" + optimizer + ("_unpromoted" if unpromoted else ""),
                      grab_routes, trainer_out=seen)
    tr = seen["trainer"]
    if optimizer == "torch_adam" and not unpromoted:      # the reference's sequence took the fast path by itself
        assert type(tr.optimizer).__name__ == "FlatAdam" and tr.optimizer.capturable and tr._graph_default and tr._host_prefetch is not None
        assert [isinstance(v, tuple) for v in tr._graphs.values()] == [True] and int(tr.optimizer.step_dev.item()) == 4
        sd = tr.optimizer.state_dict()                    # ... and its optimizer state reads back in torch.optim.Adam's layout
        ref = torch.optim.Adam(model.parameters(), lr=1e-3)
        ref.load_state_dict(sd)
        assert len(sd["state"]) == len(list(model.parameters())) and all(int(v["step"]) == 4 for v in ref.state_dict()["state"].values())
    elif unpromoted:
        assert type(tr.optimizer) is torch.optim.Adam and not tr._graph_default and tr._host_prefetch is None and not tr._graphs


@pytest.mark.parametrize("method,promoted", [("ANPMRShapeNet3D", True), ("ANPMRShapeNet3D", False), ("ANP", True), ("CondNeuralProcess", True)])
def test_trainer_trajectory_vs_oracle_resnet_family(gpulib, tmp_path, monkeypatch, method, promoted):
    """The same for BASELINE config c5's model (ANPMRShapeNet3D, Bayes-by-backprop encoder, loss + 1e-7 * kl) and its deterministic
    relatives (ANP / CondNeuralProcess over the ResNet trunks): T = 2, 4 + 4 shots, 4 iterations of the reference's calling sequence
    - ModelTrainer(model, loss, torch.optim.Adam(model.parameters(), lr), config, data).  Both loops draw their eps from the torch
    CPU generator seeded once before the first iteration, in the reference's order (bbb/BBBConv.py:88), so iteration i of either
    run samples the same eps.  `promoted` (the default since round 5): FlatAdam.from_torch_adam over ResNetNP.flat_layout, the
    gradients in the mirror arena, one eager iteration, then capture and hipGraph replays with the eps staged per step (the
    third and fourth iteration's draws made on host threads under the previous step); unpromoted: the plain eager loop with
    torch's optimizer and lazy per-layer draws."""
    import contextlib
    import importlib
    import types
    from mlhot import binding
    from mlhot.synth import get_batch_3d
    monkeypatch.chdir(tmp_path)
    mr = method == "ANPMRShapeNet3D"
    agg = "attention" if method != "CondNeuralProcess" else "max"
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                agg_mode=agg, img_agg="reshape" if mr else "max", task="shapenet_3d", temperature=0.07, max_ctx_num=4,
                                beta=1e-7 if mr else 0)
    if not promoted:
        cfg.promote_optimizer, cfg.graph_steps, cfg.host_prefetch = False, False, False
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(cfg.device)
    p0 = {n: v.detach().cpu().clone() for n, v in model.state_dict().items()}
    batches = [get_batch_3d(2, 4, 4, seed=200 + i) for i in range(4)]

    @contextlib.contextmanager
    def grab_routes(out):
        model.img_encoder.tap_log, model.decoder.tap_log = [], []
        try:
            yield
            out.append([[(t.detach().cpu() > 0).float() for t in taps] for taps in model.img_encoder.tap_log + model.decoder.tap_log])
        finally:
            model.img_encoder.tap_log, model.decoder.tap_log = None, None

    def oracle_step(p, cx, cy, qx, qy, routes, tie):
        pres = []
        if mr:
            mu, kl = O.anpmr3d_forward(p, cx, cy, qx, routes=routes, pres=pres)
        else:
            mu, kl = O.resnet_np_forward(p, cx, cy, qx, agg, cfg.img_agg, routes=routes, pres=pres), 0.0
        flips = sum(U.relu_flips(m, v, "resnet", tie) for masks, pre in zip(routes, pres) for m, v in zip(masks, pre))
        return O.calc_loss("shapenet_3d", mu, qy) + 1e-7 * kl, flips
    seen = {}
    try:
        _trajectory_check(model, p0, oracle_step, batches, lambda m: torch.optim.Adam(m.parameters(), lr=1e-3), cfg, tmp_path,
                          f"{method}_{'promoted' if promoted else 'unpromoted'}", grab_routes, seed_eps=99, trainer_out=seen)
        tr = seen["trainer"]
        if promoted:        # the reference's sequence took the fast path by itself
            assert type(tr.optimizer).__name__ == "FlatAdam" and tr.optimizer.capturable and tr._graph_default
            assert [isinstance(v, tuple) for v in tr._graphs.values()] == [True] and int(tr.optimizer.step_dev.item()) == 4
            assert tr.optimizer.active < tr.optimizer.flat.numel()                      # resnet.fc.* parked behind the update
            assert all(p.untyped_storage().data_ptr() == tr.optimizer.flat.untyped_storage().data_ptr() for p in model.parameters())
            assert (tr._eps is not None and bool(tr._eps)) == mr
            if mr:
                assert tr._eps._pieces is not None and len(tr._eps._pieces) > 1     # ... and its eps were drawn on several host threads
            sd = tr.optimizer.state_dict()
            ref = torch.optim.Adam(model.parameters(), lr=1e-3)
            ref.load_state_dict(sd)
            stepped = [i for i, (n, _) in enumerate(model.named_parameters()) if ".resnet.fc." not in n]
            assert sorted(sd["state"]) == stepped
        else:
            assert type(tr.optimizer) is torch.optim.Adam and not tr._graph_default and not tr._graphs and tr._eps is None
    finally:
        binding.set_grad_arena(None)


@pytest.mark.parametrize("shape", [(2, 3, 12, 12, 8, 5, 2, 2), (2, 4, 9, 9, 6, 3, 2, 1), (1, 5, 8, 8, 7, 3, 1, 1), (2, 4, 8, 8, 5, 1, 2, 0),
                                   (1, 2, 7, 7, 3, 3, 3, 1), (120, 64, 8, 8, 64, 3, 2, 1), (30, 64, 32, 32, 64, 3, 2, 1), (9, 3, 64, 64, 64, 5, 2, 2)])
@pytest.mark.parametrize("relu", [False, True])
def test_conv2d_runtime_shapes_vs_torch(gpulib, shape, relu):
    """The hoisted / select-free gathers of the run-time-shaped convolution problems (A2 / B2 of ConvFwdRT, ConvWgradRT, ConvDgradRT),
    the 16-row and 128-row tile variants and the batched parity-class launch against F.conv2d and its autograd on the CPU:
    odd sizes, strides 1-3, k = 1 / 3 / 5, row counts on both sides of the tile-choice threshold."""
    N, Cin, H, W, Cout, k, s, p = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, Cin, H, W, generator=g).requires_grad_(True)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).requires_grad_(True)
    b = torch.randn(Cout, generator=g).requires_grad_(True)
    ref = F.conv2d(x, w, b, stride=s, padding=p)
    ref = F.relu(ref) if relu else ref
    xd, wd, bd = dev(x.detach(), w.detach(), b.detach())
    y = gpulib.conv2d_fwd(xd, wd, bd, s, p, relu)
    assert U.rel_err(y, ref) <= 1e-5
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    # the backward masks with sign(forward output): hand it the CPU's output so that a rounding-level tie cannot flip one ReLU
    dx, dw, db = gpulib.conv2d_bwd(xd, wd, ref.detach().to(DEV), dy.to(DEV), s, p, relu)
    assert U.rel_err(dx, x.grad) <= 2e-5 and U.rel_err(dw, w.grad) <= 2e-5 and U.rel_err(db, b.grad) <= 2e-5


# ---- batch ingest: uint8 channel-last -> fp32 channel-first on the device ------------
def test_ingest_kernel_bit_exact_vs_reference_vectors(gpulib):
    fx = np.load(os.path.join(U.GOLDEN, "ingest.npz"))
    for C in (1, 2, 3, 4):
        got = gpulib.ingest_u8_nhwc(torch.from_numpy(fx[f"c{C}/u8"]).to(DEV))
        assert np.array_equal(got.cpu().numpy(), fx[f"c{C}/f32"]), C


@pytest.mark.parametrize("shape", [(16, 15, 128, 128, 1), (8, 15, 64, 64, 4), (2, 3, 64, 64, 3), (3, 1, 7, 5, 3), (1, 2, 9, 9, 1),
                                   (2, 0, 128, 128, 1), (1, 1, 2, 2, 2), (5, 128, 128, 1)])
def test_ingest_kernel_bit_exact_vs_oracle(gpulib, shape):
    """Every byte value, the quad fast path (H*W % 4 == 0, C <= 4) and the any-shape path, an empty batch; full c3 / c5 sizes."""
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    got = gpulib.ingest_u8_nhwc(u8.to(DEV))
    want = O.ingest_images(u8.numpy().reshape((1,) * (5 - len(shape)) + shape)).reshape(got.shape)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)


def test_batch_ingest_pipeline_matches_host_conversion(gpulib):
    """Pinned staging + copy stream + ingest kernel: batches come out bit-identical to the reference's host conversion,
    in ticket order, while later batches are already in flight; slot exhaustion and CPU devices are refused."""
    from mlhot.binding import MlhotError
    from mlhot.ingest import BatchIngest
    from mlhot import synth
    ing = BatchIngest(DEV)
    batches = [synth.get_batch_u8("shapenet_1d", 4, nc, 15, seed=100 + i) for i, nc in enumerate((15, 15, 7, 15, 3))]
    want = [(synth.host_convert(b[0]), synth.host_convert(b[1]), b[2], b[3]) for b in batches]
    ing.stage(*batches[0])
    for i in range(len(batches)):
        if i + 1 < len(batches):
            ing.stage(*batches[i + 1])                     # copy of batch i+1 overlaps with the use of batch i
        got = ing.take()
        junk = torch.randn(512, 512, device=DEV) @ torch.randn(512, 512, device=DEV)   # keep the compute stream busy
        for g_, w_ in zip(got, want[i]):
            assert torch.equal(g_.cpu(), w_), i
        del junk
    t0, t1 = ing.stage(*batches[0]), ing.stage(*batches[1])
    with pytest.raises(MlhotError):
        ing.stage(*batches[3])                             # a third batch of the same shape: both slots are busy
    assert torch.equal(ing.take(t1)[0].cpu(), want[1][0])  # out of order by ticket
    assert torch.equal(ing.take(t0)[0].cpu(), want[0][0])
    with pytest.raises(MlhotError):
        ing.take()
    with pytest.raises(MlhotError):
        BatchIngest("cpu")


@pytest.mark.parametrize("depth", [2, 4])
def test_host_batches_two_ahead_on_the_worker_thread_arrive_in_order_and_intact(gpulib, depth):
    """trainer._HostPrefetch as the trainer drives it since round 6: `depth` batches (config.host_prefetch_depth: the default 2, and 4)
    staged ahead on the worker thread while the owner takes the oldest (BatchIngest's slot choice and queue under a lock, depth + 1
    slots per shape).  300 batches of two alternating shapes, byte images (the byte route) with every 7th batch off the byte grid (the
    fp32 route), each checked bit for bit against the host tensors after the NEXT `depth` have been put on their way."""
    import collections
    from mlhot import synth
    from trainer.model_trainer import _HostPrefetch
    rs = np.random.RandomState(5)

    def host_batch(i):
        nc = 3 + (i % 2)
        xs = synth.host_convert(rs.randint(0, 256, size=(2, nc, 32, 32, 1)).astype(np.uint8))
        xq = synth.host_convert(rs.randint(0, 256, size=(2, 5, 32, 32, 1)).astype(np.uint8))
        if i % 7 == 3:
            xs.view(-1)[i] = 0.5001
        return xs, xq, torch.full((2, nc, 3), float(i)), torch.full((2, 5, 3), float(-i))

    hp = _HostPrefetch(DEV, depth=depth)
    try:
        q = collections.deque()
        n, routes = 300, collections.Counter()
        for i in range(n + depth):
            if i < n:
                hb = host_batch(i)
                q.append((hb, hp.stage(hb)))
            if len(q) > depth or i >= n:
                if not q:
                    break
                hb, ticket = q.popleft()
                got = hp.take(ticket)
                routes["u8" if hp.last_fixed else "fp32"] += 1
                got = [g.clone() for g in got]          # the byte route hands every batch of a shape out in the same device tensors
                torch.cuda.synchronize()
                for g, h in zip(got, hb):
                    assert g.shape == h.shape and torch.equal(g.cpu(), h)
        assert not q and routes["u8"] + routes["fp32"] == n and routes["fp32"] == len([i for i in range(n) if i % 7 == 3])
        assert all(len(ring) <= depth + 1 for ring in hp.u8.ing._slots.values())
    finally:
        hp._pool.shutdown(wait=True)


@pytest.mark.parametrize("C,H,W", [(1, 128, 128), (3, 64, 64)])
def test_exact_u8_feed_round_trip_is_bit_exact(gpulib, C, H, W):
    """mlhot.ingest.ExactU8Feed: a reference-style loader's fp32 channel-first host batch (dataset/shapenet_1d.py:
    189-196, utils/utils.py:26-30: bytes / 255) crosses PCIe as bytes and comes out of the ingest kernel with the SAME fp32 bits as
    `.to(device)` of the host tensors - for one-channel and three-channel images, on several host threads, batch after batch in the
    same device tensors; a batch holding ONE element that is not k / 255 is refused (stage() -> None), and trainer._HostPrefetch then
    ships it as fp32, again bit-identical."""
    from mlhot import synth
    from mlhot.ingest import ExactU8Feed
    from trainer.model_trainer import _HostPrefetch
    T, Nc, Nq = 3, 5, 7
    rs = np.random.RandomState(11)

    def host_batch():
        xs = synth.host_convert(rs.randint(0, 256, size=(T, Nc, H, W, C)).astype(np.uint8))
        xq = synth.host_convert(rs.randint(0, 256, size=(T, Nq, H, W, C)).astype(np.uint8))
        return xs, xq, torch.from_numpy(rs.rand(T, Nc, 3).astype(np.float32)), torch.from_numpy(rs.rand(T, Nq, 3).astype(np.float32))

    feed = ExactU8Feed(DEV, threads=3)
    ptrs = None
    for _ in range(3):
        hb = host_batch()
        ticket = feed.stage(hb)
        assert ticket is not None
        got = feed.take(ticket)
        torch.cuda.synchronize()
        for g, h in zip(got, hb):
            assert g.shape == h.shape and torch.equal(g.cpu(), h)
        assert ptrs is None or ptrs == [g.data_ptr() for g in got]       # fixed addresses per batch shape (graph replay reads them)
        ptrs = [g.data_ptr() for g in got]
    assert feed.shipped == 3 and feed.refused == 0
    hb = host_batch()
    hb[1].view(-1)[12345] = torch.nextafter(hb[1].view(-1)[12345], torch.tensor(2.0))
    assert feed.stage(hb) is None and feed.refused == 1 and feed.ok
    for background in (True, False):          # the copy on the worker thread (default) and on the caller's
        hp = _HostPrefetch(DEV, background=background)
        for batch, route in ((hb, "fp32"), (host_batch(), "u8"), (host_batch(), "u8")):
            ticket = hp.stage(batch)
            assert (ticket[0] == "later") == background
            got = hp.take(ticket)
            assert hp.last_fixed == (route == "u8")
            torch.cuda.synchronize()
            for g, h in zip(got, batch):
                assert torch.equal(g.cpu(), h)
    # a loader that never hands out byte images: after three refusals in a row the check is not attempted any more
    feed = ExactU8Feed(DEV, threads=2)
    noise = (torch.rand(T, Nc, C, H, W), torch.rand(T, Nq, C, H, W), torch.rand(T, Nc, 3), torch.rand(T, Nq, 3))
    for _ in range(3):
        assert feed.stage(noise) is None
    assert not feed.ok and feed.stage(host_batch()) is None


def test_trainer_ingest_path_equals_host_path(gpulib, tmp_path, monkeypatch):
    """The trainer fed through BatchIngest (uint8 over PCIe, prefetched) walks exactly the trajectory of the reference's
    route (host conversion, `.to(device)`): same draws, bit-identical inputs, identical final weights."""
    import types
    from mlhot import synth
    from networks.CNPShapeNet1D import CNPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)

    class HostData(synth.SyntheticData):
        def get_batch(self, source, tasks_per_batch, shot):
            xs, xq, ys, yq = synth.SyntheticData.get_batch_u8(self, source, tasks_per_batch, shot)
            return synth.host_convert(xs), synth.host_convert(xq), ys, yq

    finals = []
    for use_ingest in (True, False):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="mean", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=100,
                                    dim_z=64, task="shapenet_1d", iterations=5, val_freq=2, val_iters=2, bg_gen_freq=1000,
                                    gen_bg=False, max_ctx_num=6, beta=0, contrastive=False, ingest_u8=use_ingest,
                                    save_path=str(tmp_path / f"run{int(use_ingest)}"), logger=None)
        model = CNPShapeNet1D(cfg).to(cfg.device)
        trainer = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3),
                               config=cfg, data=HostData())
        assert (trainer.ingest is not None) == use_ingest
        trainer.train()
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k


@pytest.mark.parametrize("method,agg,max_ctx,nq", [("ANPShapeNet1D", "attention", 5, None), ("CNPShapeNet1D", "max", 5, None),
                                                    ("ANPShapeNet1D", "attention", 25, 30), ("CNPShapeNet1D", "mean", 25, 30)],
                         ids=["anp_1..5", "cnp_max_1..5", "anp_1..25_nq30", "cnp_mean_1..25_nq30"])
def test_evaluator_context_sweep_vs_oracle(gpulib, tmp_path, method, agg, max_ctx, nq):
    """SURVEY §8f rank 3, the eval path (evaluator/model_evaluator.py:95-179): forward-only test-mode batches for every
    context size 1..max_ctx_num, mean / std of the test loss per size against the CPU oracle on the same draws; the ingest
    route and the host route must agree bit for bit.  The `1..25_nq30` cases are the shipped evaluation sizes (max_ctx_num = 25 in
    cfg/evaluation/*, 30 target views per task as dataset/shapenet_3d.py:201-202's eval mode): context sizes above 16 leave the
    specialised tail for the generic one and FAVOR+ runs up to 25 + 30 shots THROUGH THE EVALUATOR; the oracle is evaluated at the
    sizes {1, 5, 16, 17, 25} (both sides of the 16-shot boundary), the kernels at every size."""
    import importlib
    import types
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot import synth
    from trainer.losses import LossFunc

    class HostData(synth.SyntheticData):
        def get_batch_u8(self, source, tasks_per_batch, shot):
            if nq is None:
                return synth.SyntheticData.get_batch_u8(self, source, tasks_per_batch, shot)
            rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
            return synth.get_batch_u8(self.task, tasks_per_batch, shot, nq, seed=int(rng.randint(0, 2 ** 31 - 1)))

        def get_batch(self, source, tasks_per_batch, shot):
            xs, xq, ys, yq = self.get_batch_u8(source, tasks_per_batch, shot)
            return synth.host_convert(xs), synth.host_convert(xq), ys, yq

    results = {}
    for use_ingest in (True, False):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode=agg, img_agg="", dim_w=64, n_hidden_units_r=[100, 100],
                                    dim_r=64 if agg == "attention" else 100, dim_z=64, task="shapenet_1d", iterations=0, val_iters=2,
                                    max_ctx_num=max_ctx, contrastive=False, ingest_u8=use_ingest, logger=None,
                                    save_path=str(tmp_path / f"eval{int(use_ingest)}"))
        model = getattr(importlib.import_module("networks." + method), method)(cfg).to(cfg.device)
        ev = ModelEvaluator(model=model, loss=LossFunc("mse", "shapenet_1d"), config=cfg, data=HostData())
        assert (ev.ingest is not None) == use_ingest
        results[use_ingest] = ev.evaluate()
        table = np.loadtxt(tmp_path / f"eval{int(use_ingest)}" / "test_losses.txt")
        assert table.shape == (max_ctx, 3) and list(table[:, 0]) == list(range(1, max_ctx + 1))
        assert os.path.exists(tmp_path / f"eval{int(use_ingest)}" / "models" / "model.pt")
    assert results[True] == results[False]
    # the oracle on the same draws
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    check = set(range(1, 6)) if max_ctx <= 5 else {1, 5, 16, 17, 25}
    for si, source in enumerate(("validation", "test")):
        for ctx_num in sorted(check):
            data = HostData()
            getattr(data, "test_rng" if source == "test" else "val_rng").seed(42)
            vals, bounds = [], []
            for _ in range(2):
                cx, qx, cy, qy = data.get_batch(source, 2, ctx_num)
                assert cx.shape[1] == ctx_num and qx.shape[1] == (ctx_num if nq is None else nq)
                mu = O.vanilla_np_forward(p, cx, cy, qx, agg, tanh=True)
                vals.append(O.calc_loss("shapenet_1d", mu, qy, test=True).view(1))
                # The tolerance, derived instead of guessed.  mu itself is held to north_star's 1e-4 of its scale everywhere else in
                # this file; the degree error (losses.py:63-76) is acos(mu[0]) in degrees, and acos is the ONE step that amplifies:
                # |d deg| = (180 / pi) |d mu0| / sqrt(1 - mu0^2), unbounded as tanh saturates (|mu0| -> 1), where acos's
                # square-root branch point caps it at (180 / pi) sqrt(2 |d mu0|).  Everything after acos (the 360-degree wrap, abs,
                # the minimum of three, the mean over the rows) is 1-Lipschitz.  So a row may move by the smaller of the two, and a
                # batch's loss by the mean of its rows' allowances.
                dm = 1e-4 * mu.abs().max().item()
                m0 = mu[..., 0].double().clamp(-1.0, 1.0)
                per_row = torch.minimum(dm / torch.sqrt((1.0 - m0 * m0).clamp_min(1e-30)), torch.full_like(m0, (2.0 * dm) ** 0.5)) * (180.0 / np.pi)
                bounds.append(per_row.mean().item())
            vals = torch.cat(vals)
            got_mean, got_std = results[True][si][0][ctx_num - 1], results[True][si][1][ctx_num - 1]
            err_mean, err_std = abs(got_mean - vals.mean().item()), abs(got_std - vals.std().item())
            # mean over two batches: the mean of the allowances; std of two values = |a - b| / sqrt(2): sqrt(2) x the larger allowance;
            # + 1e-5 relative for the fp32 reductions themselves
            tol_mean = sum(bounds) / 2 + 1e-5 * max(1.0, abs(vals.mean().item()))
            tol_std = 2 ** 0.5 * max(bounds) + 1e-5 * max(1.0, abs(vals.std().item()))
            print(f"[evaluator sweep] {source} Nc={ctx_num}: degree-error mean {vals.mean().item():.4f} (kernels off by {err_mean:.2e}, allowed {tol_mean:.2e}), "
                  f"std off by {err_std:.2e} (allowed {tol_std:.2e})")
            assert err_mean <= tol_mean, (source, ctx_num, err_mean, tol_mean)
            assert err_std <= tol_std, (source, ctx_num, err_std, tol_std)


def test_graph_replayed_training_equals_eager_training(gpulib, tmp_path, monkeypatch):
    """config.graph_steps: every training iteration replayed from a per-shape hipGraph (forward, loss, backward and the
    capturable FlatAdam step with its device-side step count) lands on exactly the weights of the same loop run eagerly -
    same draws, same kernels, incl. iterations whose batch shape appears for the first (eager warm-up), second (capture +
    replay) and later (replay) time - and the validation cadence / files are untouched."""
    import types
    from mlhot.optim import FlatAdam
    from mlhot.synth import SyntheticData
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)
    finals, losses = [], []
    for graph in (False, True):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                    dim_z=64, task="shapenet_1d", iterations=12, val_freq=6, val_iters=1, bg_gen_freq=1000, gen_bg=False,
                                    max_ctx_num=5, beta=0, contrastive=False, graph_steps=graph, log_every=1,
                                    save_path=str(tmp_path / f"g{int(graph)}"), logger=None)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        opt = FlatAdam(model, lr=1e-3, ctx_num=5, test_num=5, capturable=True)
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=opt, config=cfg, data=SyntheticData())
        seen = []
        orig = tr._report
        tr._report = lambda it, v, _o=orig, _s=seen: (_s.append(v), _o(it, v))[1]      # every iteration's loss in iteration order (lagged log: handed out one call late)
        tr.train()
        losses.append(seen)
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
        if graph:
            kinds = [isinstance(v, tuple) for v in tr._graphs.values()]
            assert True in kinds                        # context sizes 3..5 over 12 iterations: at least one shape was captured
        assert int(opt.step_dev.item()) == 12
        assert os.path.exists(tmp_path / f"g{int(graph)}" / "models" / "model_end_12.pt")
    assert losses[0] == losses[1]
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k


def test_lagged_loss_log_reports_every_iteration_one_late(gpulib, tmp_path, monkeypatch):
    """config.lagged_loss_log (the default of replayed iterations; False = read behind every step): the replayed loop logs and checks
    EVERY iteration's loss, one iteration late - the same
    (iteration, value) pairs in the same order as the loop that reads `losses.item()` behind every step (model_trainer.py:87-91),
    nothing left behind a validation round or the end of train(), identical final weights."""
    import types
    from mlhot.optim import FlatAdam
    from mlhot.synth import SyntheticData
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)
    reports, finals, returned = [], [], []
    for lag in (False, True):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                    dim_z=64, task="shapenet_1d", iterations=13, val_freq=5, val_iters=1, bg_gen_freq=1000, gen_bg=False,
                                    max_ctx_num=5, beta=0, contrastive=False, graph_steps=True, log_every=1, lagged_loss_log=lag,
                                    save_path=str(tmp_path / f"l{int(lag)}"), logger=None)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=FlatAdam(model, lr=1e-3, ctx_num=5, test_num=5, capturable=True),
                          config=cfg, data=SyntheticData())
        seen, rets = [], []
        orig_report, orig_iter = tr._report, tr._train_iter
        tr._report = lambda it, value, _o=orig_report, _s=seen: (_s.append((it, value)), _o(it, value))[1]
        tr._train_iter = lambda it, _o=orig_iter, _r=rets: _r.append(_o(it))
        tr.train()
        reports.append(seen); returned.append(rets)
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
    assert [it for it, _ in reports[0]] == list(range(1, 14)) and reports[0] == reports[1]
    # what _train_iter hands back: the iteration's own loss / the previous iteration's (None right behind a flush: iterations 1, 6, 11)
    assert returned[0] == [v for _, v in reports[0]]
    want = [None if it in (1, 6, 11) else reports[0][it - 2][1] for it in range(1, 14)]
    assert returned[1] == want
    assert ModelTrainer._lagged(types.SimpleNamespace(config=types.SimpleNamespace())) is True       # a config that does not say: late
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k


def test_lagged_loss_log_does_not_depend_on_the_callers_iteration_numbers(gpulib, tmp_path, monkeypatch):
    """A caller that drives `_train_iter` itself with a stride of two (it = 2, 4, 6, 8): the late log takes its two pinned buffers in
    turn by its own count of calls, so every iteration is reported with ITS loss - the same (iteration, value) pairs as the read
    behind every step on the same draws, the last one through the trainer's flush.  (Indexed by the parity of `it`, all four calls
    shared one buffer and iteration 2 was reported with iteration 4's value.)"""
    import types
    from mlhot.optim import FlatAdam
    from mlhot.synth import SyntheticData
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)
    reports = []
    for lag in (False, True):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                    dim_z=64, task="shapenet_1d", iterations=100, val_freq=1000, val_iters=1, bg_gen_freq=1000, gen_bg=False,
                                    max_ctx_num=5, beta=0, contrastive=False, graph_steps=True, log_every=1, lagged_loss_log=lag,
                                    save_path=str(tmp_path / f"s{int(lag)}"), logger=None)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=FlatAdam(model, lr=1e-3, ctx_num=5, test_num=5, capturable=True),
                          config=cfg, data=SyntheticData())
        seen = []
        orig_report = tr._report
        tr._report = lambda it, value, _o=orig_report, _s=seen: (_s.append((it, value)), _o(it, value))[1]
        try:
            for it in (2, 4, 6, 8):
                tr._train_iter(it)
            tr._flush_loss()
        finally:
            tr.close()
        reports.append(seen)
    print(f"[stride-2 late log] read behind the step {reports[0]}, one call late {reports[1]}")
    assert [it for it, _ in reports[0]] == [2, 4, 6, 8] and len({v for _, v in reports[0]}) == 4
    assert reports[1] == reports[0]


def test_late_loss_read_stops_on_a_non_finite_loss_with_the_same_log_exit_code_and_files(gpulib, tmp_path, monkeypatch):
    """The claim behind `config.lagged_loss_log` being the default: an observer of the reference's loop (trainer/model_trainer.py:87-93:
    log the loss, `sys.exit(1)` when it is not finite) sees the same thing.  A loader whose 7th training batch holds a NaN label, a
    validation round at iteration 5, an (untouched) checkpoint cadence: with the read behind every step and with the read one iteration
    late the logger receives the SAME lines in the same order, the process exits with the same code, and the same files exist."""
    import types
    from mlhot.optim import FlatAdam
    from mlhot.synth import SyntheticData
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)

    class Poisoned(SyntheticData):
        def __init__(self):
            super().__init__()
            self.n_train = 0

        def get_batch_u8(self, source, tasks_per_batch, shot):        # the route the trainer takes for this loader (bytes + labels)
            xs, xq, ys, yq = super().get_batch_u8(source, tasks_per_batch, shot)
            if source == "train":
                self.n_train += 1
                if self.n_train == 7:
                    yq = yq.copy() if isinstance(yq, np.ndarray) else yq.clone()
                    yq[0, 0, 0] = float("nan")
            return xs, xq, ys, yq

    class Lines:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    seen = []
    for lag in (False, True):
        log = Lines()
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                    dim_z=64, task="shapenet_1d", iterations=12, val_freq=5, val_iters=1, bg_gen_freq=1000, gen_bg=False,
                                    max_ctx_num=5, beta=0, contrastive=False, graph_steps=True, log_every=1, lagged_loss_log=lag,
                                    save_path=str(tmp_path / f"n{int(lag)}"), logger=log)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=FlatAdam(model, lr=1e-3, ctx_num=5, test_num=5, capturable=True),
                          config=cfg, data=Poisoned())
        with pytest.raises(SystemExit) as stop:
            tr.train()
        tr.close()
        files = sorted(os.path.relpath(os.path.join(d, f), cfg.save_path) for d, _, fs in os.walk(cfg.save_path) for f in fs if not f.startswith("events."))
        lines = [l for l in log.lines if not l.startswith("mlhot:")]           # (the announcements say which of the two modes runs)
        seen.append((stop.value.code, lines, files))
    assert seen[0][0] == seen[1][0] == 1
    assert any("Train Iteration 6 " in l for l in seen[0][1]) and any("Loss is nan" in l for l in seen[0][1])
    assert not any("Train Iteration 8 " in l for l in seen[0][1] + seen[1][1])
    assert seen[0][1] == seen[1][1]
    assert seen[0][2] == seen[1][2] and not any("model_end" in f for f in seen[0][2])


def test_graph_replayed_multi_rank_training_uses_each_graphs_own_gradients(gpulib, tmp_path, monkeypatch):
    """graph_steps with world > 1: the all-reduce and the optimizer step run OUTSIDE the graphs and read p.grad, which a replay
    does not rebind - with several batch shapes (the context size is drawn per iteration) each captured graph owns different
    gradient tensors.  Two identical ranks are simulated (sum = 2x, then the 1/world scale in FlatAdam's gradient scale - exact in
    fp32), so the graph-replayed multi-rank loop, the eager multi-rank loop and the plain single-rank loop must all land on
    bit-identical weights."""
    import types
    from mlhot import dist as mdist
    from mlhot.optim import FlatAdam
    from mlhot.synth import SyntheticData
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)
    calls = []

    class TwoRanks(mdist.GradBucket):
        def world_size(self):
            return 2

        def _all_reduce(self, flat):
            calls.append(flat.data_ptr())
            flat.mul_(2.0)

    finals = []
    for tag, graph, two in (("single", False, False), ("eager2", False, True), ("graph2", True, True)):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                    dim_z=64, task="shapenet_1d", iterations=14, val_freq=7, val_iters=1, bg_gen_freq=1000, gen_bg=False,
                                    max_ctx_num=5, beta=0, contrastive=False, graph_steps=graph, log_every=1,
                                    save_path=str(tmp_path / tag), logger=None)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        opt = FlatAdam(model, lr=1e-3, ctx_num=5, test_num=5, capturable=True)
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=opt, config=cfg, data=SyntheticData())
        if two:
            tr.bucket = TwoRanks(model.parameters())
        n0 = len(calls)
        tr.train()
        if two:
            assert len(calls) - n0 == 14                       # one collective per iteration
        if graph:
            captured = [v for v in tr._graphs.values() if isinstance(v, tuple)]
            assert len(captured) >= 2                           # several context sizes were captured: several gradient pools
            assert len({v[2][0].data_ptr() for v in captured}) == len(captured)
        assert int(opt.step_dev.item()) == 14
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), ("eager two-rank", k)
        assert torch.equal(finals[0][k], finals[2][k]), ("graph two-rank", k)


def test_promoted_bbb_trainer_keeps_the_generator_order(gpulib, tmp_path, monkeypatch):
    """ANPMRShapeNet3D through trainer.ModelTrainer's promoted defaults: the Bayes-by-backprop eps come from the torch CPU generator in the
    reference's order (bbb/BBBConv.py:86-95) whichever way an iteration runs - lazily inside an eager forward, staged in front of a
    replay, prefetched on host threads under the previous step - and the validation forwards in between draw from the same generator.
    12 iterations with two context sizes (two graphs) and two validation rounds: the eager loop, the replayed loop and the replayed
    loop of two simulated ranks (sum = 2x, 1/world in FlatAdam's gradient scale: exact) land on bit-identical losses and weights."""
    import types
    from mlhot import binding, dist as mdist
    from mlhot.synth import get_batch_3d
    from networks.ANPMRShapeNet3D import ANPMRShapeNet3D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)

    class Data3D:
        def __init__(self):
            self.rng, self.val_rng = np.random.RandomState(3), np.random.RandomState(4)

        def gen_bg(self, *a, **k):
            pass

        def get_batch(self, source, tasks_per_batch, shot):
            rng = self.rng if source == "train" else self.val_rng
            n_ctx = int(rng.randint(3, shot + 1)) if source == "train" else shot
            return get_batch_3d(tasks_per_batch, n_ctx, shot, seed=int(rng.randint(0, 2 ** 31 - 1)))

    class TwoRanks(mdist.GradBucket):
        def world_size(self):
            return 2

        def _all_reduce(self, flat):
            flat.mul_(2.0)

    runs = []
    try:
        for tag, graph, two in (("eager", False, False), ("replayed", None, False), ("replayed_two_ranks", None, True)):
            cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                        agg_mode="attention", img_agg="reshape", task="shapenet_3d", temperature=0.07, max_ctx_num=4, beta=1e-7,
                                        iterations=12, val_freq=6, val_iters=1, bg_gen_freq=1000, gen_bg=False, contrastive=False, log_every=1,
                                        save_path=str(tmp_path / tag), logger=None)
            if graph is not None:
                cfg.graph_steps = graph
            model = ANPMRShapeNet3D(cfg).to(cfg.device)
            tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_3d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3), config=cfg,
                              data=Data3D())
            assert type(tr.optimizer).__name__ == "FlatAdam" and tr._graph_default == (graph is None)
            if two:
                tr.bucket = TwoRanks(model.parameters(), early=model.early_grad_parameters())
            seen = []
            orig = tr._report
            tr._report = lambda it, v, _o=orig, _s=seen: (_s.append(v), _o(it, v))[1]
            torch.manual_seed(31)
            tr.train()
            if graph is None:
                assert 1 <= len([v for v in tr._graphs.values() if isinstance(v, tuple)]) <= 2 and tr._eps._pieces is not None
            assert int(tr.optimizer.step_dev.item()) == 12
            runs.append((seen, {k: v.clone() for k, v in model.state_dict().items()}, torch.get_rng_state()))
            binding.set_grad_arena(None)
    finally:
        binding.set_grad_arena(None)
    for tag, (seen, final, state) in zip(("replayed", "replayed_two_ranks"), runs[1:]):
        assert seen == runs[0][0], tag
        assert torch.equal(state, runs[0][2]), tag                  # the CPU generator ends where the eager loop leaves it
        for k in final:
            assert torch.equal(final[k], runs[0][1][k]), (tag, k)


def test_trainer_ingest_prefetch_keeps_the_reference_draw_order(gpulib, tmp_path, monkeypatch):
    """The reference draws train_k, then the validation / test batches of iteration k, then train_k+1, possibly all from ONE
    shared generator (np.random in its loaders).  The ingest route prefetches train_k+1 while step k computes - but only when
    nothing else draws in between: with a data source that shares one generator across its sources, the ingest route and the
    host route must see the same sequence of draws and reach identical weights."""
    import types
    from mlhot import synth
    from networks.CNPShapeNet1D import CNPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)

    class SharedRng(synth.SyntheticData):
        """every source draws from the same generator, as the reference's loaders do through np.random"""
        def __init__(self):
            super().__init__()
            self.val_rng = self.test_rng = self.rng
            self.log = []

        def get_batch_u8(self, source, tasks_per_batch, shot):
            self.log.append(source)
            return super().get_batch_u8(source, tasks_per_batch, shot)

        def get_batch(self, source, tasks_per_batch, shot):            # the host route (config.ingest_u8 = False)
            xs, xq, ys, yq = self.get_batch_u8(source, tasks_per_batch, shot)
            return synth.host_convert(xs), synth.host_convert(xq), ys, yq

    finals, logs = [], []
    for use_ingest in (True, False):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="mean", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=100,
                                    dim_z=64, task="shapenet_1d", iterations=7, val_freq=3, val_iters=2, bg_gen_freq=1000,
                                    gen_bg=False, max_ctx_num=6, beta=0, contrastive=False, ingest_u8=use_ingest,
                                    save_path=str(tmp_path / f"run{int(use_ingest)}"), logger=None)
        model = CNPShapeNet1D(cfg).to(cfg.device)
        data = SharedRng()
        trainer = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3),
                               config=cfg, data=data)
        assert (trainer.ingest is not None) == use_ingest
        trainer.train()
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
        logs.append(list(data.log))
    want = []
    for it in range(1, 8):
        want.append("train")
        if it % 3 == 0:
            want += ["validation"] * 2 + ["test"] * 2
    assert logs[0] == want and logs[1] == want
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k


def test_trainer_contrastive_model(gpulib, tmp_path, monkeypatch):
    """config.contrastive: the trainer hands the target labels to an FCL* model and adds contrastive_rate x the NT-Xent term
    (trainer/model_trainer.py:72-81 of the reference); validation calls the 4-tuple forward with test=True."""
    import types
    from mlhot.synth import SyntheticData
    from networks.FCLCNPShapeNet1D import FCLCNPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    monkeypatch.chdir(tmp_path)
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=3, input_dim=3, output_dim=2,
                                agg_mode="max", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=100, dim_z=64, task="shapenet_1d",
                                iterations=3, val_freq=3, val_iters=1, bg_gen_freq=1000, gen_bg=False, max_ctx_num=5, beta=0,
                                contrastive=True, contrastive_rate=0.5, save_path=str(tmp_path / "run"), logger=None)
    model = FCLCNPShapeNet1D(cfg).to(cfg.device)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3), config=cfg,
                 data=SyntheticData()).train()
    assert os.path.exists(tmp_path / "run" / "models" / "model_end_3.pt")
    assert sum(float((v - before[k]).abs().sum()) for k, v in model.state_dict().items()) > 0
    assert all(torch.isfinite(v).all() for v in model.state_dict().values())


@pytest.mark.parametrize("workload,tasks", [("c3", 16), ("c5", 8)])
def test_bench_two_rank_control_flow_on_one_gpu(gpulib, workload, tasks):
    """bench.py's N > 1 path (per-rank task shards, hipGraph step, gradient all-reduce outside the graph - for c5 the same eps on
    every rank and the side-stream bucket - max-over-ranks timing, one JSON line from rank 0) driven by two gloo ranks sharing this
    box's only GPU - the RCCL launch itself needs an N-GPU node."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MLHOT_DIST_BACKEND="gloo", MLHOT_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533" if workload == "c3" else "29534", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4",
           "--warmup", "2", "--workload", workload]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["scaling"] == "weak" and out["hipgraph"] is True
    assert out["config"]["global_tasks"] == 2 * tasks and out["cpu_baseline"] is None
    assert abs(out["value"] - 2 * tasks * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]


def test_bench_launches_its_own_ranks_on_one_gpu(gpulib):
    """Plain `python bench.py --gpus 2 --workload c3` - no torchrun, no WORLD_SIZE - starts its two ranks itself (bench.spawn_ranks;
    here both share this box's only GPU through the MLHOT_ONE_DEVICE / gloo hooks, on an 8-GPU node the same command runs one rank
    per GPU over RCCL), relays ONE JSON line and says who launched and what the backend reports."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MLHOT_DIST_BACKEND="gloo", MLHOT_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "c3", "--steps", "4", "--warmup", "2"],
                       capture_output=True, text=True, env=env, cwd=root, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert [ln for ln in r.stdout.splitlines() if ln.strip()] == [ln for ln in r.stdout.splitlines() if ln.startswith("{")] and r.stdout.count("\n") == 1, r.stdout[-2000:]
    out = json.loads(r.stdout)
    assert out["n_gpus"] == 2 and out["config"]["global_tasks"] == 32 and out["hipgraph"] is True and out["scaling"] == "weak"
    assert out["dist"]["ranks_reported_by_backend"] == 2 and out["dist"]["launcher"].startswith("bench.py itself")
    assert "starting 2 rank processes" in r.stderr and "reports 2 ranks" in r.stderr


@pytest.mark.parametrize("workload", ["c3", "c5"])
def test_bench_eight_ranks_on_one_gpu(gpulib, workload):
    """BASELINE configs[3..4]'s control flow before a real node ever sees it: plain `python bench.py --gpus 8` starts EIGHT fresh rank
    processes (bench.spawn_ranks; here all share this box's one GPU through the MLHOT_ONE_DEVICE / gloo hooks, on an 8-GPU node the
    same command is one rank per GPU over RCCL): clean exit codes, ONE JSON line, n_gpus == 8, the gradients every rank holds after
    the last all-reduce identical, the step's collectives as designed (c5: the early bucket between the two graphs, then the rest;
    c3: one flat all-reduce), and the eps draw threads adapted to eight ranks sharing the node's cores."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "LOCAL_WORLD_SIZE", "MLHOT_EPS_THREADS")}
    env.update(MLHOT_DIST_BACKEND="gloo", MLHOT_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--workload", workload, "--steps", "2", "--warmup", "1",
                        "--full", "--prof-steps", "1"], capture_output=True, text=True, env=env, cwd=root, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    out = json.loads(lines[0])
    tasks = 16 if workload == "c3" else 8
    assert out["n_gpus"] == 8 and out["config"]["global_tasks"] == 8 * tasks and out["hipgraph"] is True and out["scaling"] == "weak"
    assert out["dist"]["ranks_reported_by_backend"] == 8 and out["dist"]["launcher"].startswith("bench.py itself")
    assert "starting 8 rank processes" in r.stderr and "reports 8 ranks" in r.stderr
    per = out["dist"]["per_rank"]
    assert len(per["final_loss"]) == 8 and all(np.isfinite(v) and v > 0 for v in per["final_loss"])
    assert len(set(per["grad_sum"])) == 1 and len(set(per["grad_abs_sum"])) == 1 and per["grad_abs_sum"][0] > 0, per
    kinds = [k for k, _ in out["dist"]["collectives_per_step"]]
    if workload == "c5":
        assert kinds == ["early", "rest"] and out["dist"]["step_graphs"] == 2
        assert len(set(per["final_loss"])) == 8            # eight different task shards (the kl term is common, the losses are not)
        from networks.bbb import eps
        want = max(1, min(4, eps.usable_cores() // 16))
        assert out["eps"]["host_threads"] <= want and out["eps"]["ranks_on_node"] == 8, out["eps"]
    else:
        assert kinds == ["all"] and out["dist"]["step_graphs"] == 1
    assert abs(out["value"] - 8 * tasks * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]


def _bucket_cuda_worker(rank, world, port, out):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "what-matters-for-meta-learning_amd"), root]
    import torch.distributed as dist
    from mlhot import dist as mdist
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    mdist.init_from_env("gloo")                     # two ranks sharing the box's one GPU: gloo carries the device tensors
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    late = torch.nn.Linear(256, 256).to(dev)
    head = torch.nn.Sequential(torch.nn.Linear(256, 512), torch.nn.Tanh(), torch.nn.Linear(512, 64)).to(dev)
    params = list(late.parameters()) + list(head.parameters())
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(10 + rank)).to(dev)
    res = {}
    for name, kw, split in (("plain", dict(), False), ("side stream", dict(side_stream=True), False),
                            ("side stream, issue / finish", dict(side_stream=True), True),
                            ("early bucket on the side stream", dict(side_stream=True, early=list(head.parameters())), True)):
        for p in params:
            p.grad = None
        bucket = mdist.GradBucket(params, **kw)
        loss = head(torch.relu(late(x))).pow(2).mean()
        bucket.arm()
        loss.backward()
        if split:
            scale = bucket.sync(defer_scale=True, wait=False)
            busy = torch.ones(1 << 20, device=dev).mul_(2.0).sum()       # compute-stream work that does not read the gradients
            bucket.finish()
            assert scale == 0.5 and float(busy) == 2.0 * (1 << 20)
            grads = [p.grad * scale for p in params]
        else:
            assert bucket.sync() == 1.0
            grads = [p.grad.clone() for p in params]
        torch.cuda.synchronize()
        res[name] = ([g.cpu() for g in grads], list(bucket.issue_log))
    ok = all(torch.equal(a, b) for name in res for a, b in zip(res["plain"][0], res[name][0]))
    out[rank] = (ok, res["early bucket on the side stream"][1], res["side stream"][1])
    dist.barrier()
    dist.destroy_process_group()


def test_grad_bucket_side_stream_and_early_bucket_on_cuda(gpulib):
    """mlhot.dist.GradBucket on DEVICE tensors (two gloo ranks sharing this box's one GPU): the plain collective, the one on the
    communication stream (sync, and issue -> unrelated compute -> finish) and the early bucket issued from inside backward() all
    leave bit-identical averaged gradients; the early variant really issues two collectives."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        procs = [ctx.Process(target=_bucket_cuda_worker, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        assert len(out) == 2
        for ok, early_log, side_log in out.values():
            assert ok
            assert [k for k, _ in early_log] == ["early", "rest"] and [k for k, _ in side_log] == ["all"]


@pytest.mark.parametrize("method", ["ANPMRShapeNet3D", "ANP", "CondNeuralProcess", "ANPDistractor", "CNPDistractor"])
def test_flat_gradient_arena_for_the_resnet_family(gpulib, method):
    """VERDICT r3 item 5 i (train.py:52-56: one optimizer over all parameters): with model.enable_flat_grads() every gradient of a
    ResNet / Bayes-by-backprop model is a view of ONE flat buffer (mlhot/arena.py) - the trunk backward, the linears, the head
    stacks and the Bayes-by-backprop sampling write their slots directly - bit-identical to the separately allocated gradients,
    the early parameters in the buffer's first range; GradBucket then reduces both ranges in place (no _foreach_copy_)."""
    import importlib
    import types
    from mlhot import binding, dist as mdist
    from trainer.losses import LossFunc
    T, Nc, Nq = 2, 5, 6
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=T, input_dim=4, output_dim=4,
                                agg_mode="attention" if method.startswith("ANP") else "max", img_agg="reshape" if method == "ANPMRShapeNet3D" else "max",
                                task="shapenet_3d", temperature=0.07, dim_w=64)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
    g = torch.Generator().manual_seed(7)
    cx, qx = torch.rand(T, Nc, 3, 64, 64, generator=g).to(DEV), torch.rand(T, Nq, 3, 64, 64, generator=g).to(DEV)
    cy = F.normalize(torch.randn(T, Nc, 4, generator=g), dim=-1).to(DEV)
    qy = F.normalize(torch.randn(T, Nq, 4, generator=g), dim=-1).to(DEV)

    def step():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(99)
        mu, var, kl = model(cx, cy, qx)
        (LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy) + 1e-7 * kl).backward()
        return {k: p.grad for k, p in model.named_parameters()}
    try:
        plain = {k: (v.clone() if v is not None else None) for k, v in step().items()}
        arena = model.enable_flat_grads()
        step()                               # first step with the arena: the head stacks' storages may be re-laid, the layout follows
        grads = step()
        base = arena.flat.untyped_storage().data_ptr()
        early = {id(p) for p in model.early_grad_parameters()}
        for k, p in model.named_parameters():
            if plain[k] is None:
                assert grads[k] is None, k
                continue
            assert grads[k].untyped_storage().data_ptr() == base, f"{k}: gradient outside the flat buffer"
            assert torch.equal(grads[k], plain[k]), k
            assert (grads[k].storage_offset() < arena.first_numel) == (id(p) in early), k
        # the bucket reduces both ranges in place: a world of one, collectives replaced by a recorder
        copies = []
        real = torch._foreach_copy_
        log = []

        class Rec(mdist.GradBucket):
            def _single(self):
                return False

            def _all_reduce(self, flat):
                log.append((flat.data_ptr(), flat.numel()))
        bucket = Rec(model.parameters(), early=model.early_grad_parameters())
        model.zero_grad(set_to_none=True)
        torch.manual_seed(99)
        mu, var, kl = model(cx, cy, qx)
        loss = LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy) + 1e-7 * kl
        bucket.arm()
        torch._foreach_copy_ = lambda *a, **k: (copies.append(1), real(*a, **k))[1]
        try:
            loss.backward()
            bucket.sync()
        finally:
            torch._foreach_copy_ = real
        assert [k for k, _ in bucket.issue_log] == ["early", "rest"] and not copies
        (p0, n0), (p1, n1) = log
        assert p0 >= arena.flat.data_ptr() and p0 + 4 * n0 <= arena.flat.data_ptr() + 4 * arena.first_numel <= p1
        for k, p in model.named_parameters():
            if plain[k] is not None:
                assert torch.equal(p.grad, plain[k]), k
    finally:
        binding.set_grad_arena(None)


def _rccl_one_worker(port, out):
    """backend "nccl" (= RCCL on ROCm) at a world of ONE on the box's GPU, collectives forced (MLHOT_FORCE_COLLECTIVES)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "what-matters-for-meta-learning_amd"), root]
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MLHOT_FORCE_COLLECTIVES="1")
    import torch.distributed as dist
    import mlhot
    from mlhot import dist as mdist, ops
    assert mdist.init_from_env() == (0, 0, 1) and dist.get_backend() == "nccl"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    # (1) GradBucket on the communication stream with an early bucket issued from inside backward(): RCCL kernels ordered against
    # the compute stream by events / record_stream; a world of one must hand back exactly the local gradients
    torch.manual_seed(0)
    late = torch.nn.Linear(256, 256).to(dev)
    head = torch.nn.Sequential(torch.nn.Linear(256, 512), torch.nn.Tanh(), torch.nn.Linear(512, 64)).to(dev)
    params = list(late.parameters()) + list(head.parameters())
    x = torch.randn(64, 256, generator=torch.Generator().manual_seed(10)).to(dev)
    head(torch.relu(late(x))).pow(2).mean().backward()
    want = [p.grad.clone() for p in params]
    logs = {}
    for name, kw in (("side stream", dict(side_stream=True)), ("early + side stream", dict(side_stream=True, early=list(head.parameters())))):
        for p in params:
            p.grad = None
        bucket = mdist.GradBucket(params, **kw)
        loss = head(torch.relu(late(x))).pow(2).mean()
        bucket.arm()
        loss.backward()
        scale = bucket.sync(defer_scale=True, wait=False)
        busy = torch.ones(1 << 20, device=dev).mul_(2.0).sum()
        bucket.finish()
        torch.cuda.synchronize()
        assert scale == 1.0 and float(busy) == 2.0 * (1 << 20)
        assert all(torch.equal(p.grad, g) for p, g in zip(params, want)), name
        logs[name] = [k for k, _ in bucket.issue_log]
    # (2) strict sharded parity through RCCL: the staged FAVOR+ entries with StabiliserExchange's two collectives in between
    # (a dedicated process group, as the trainer builds it) reproduce the unstaged pass bit for bit
    L = mlhot.lib()
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(2, n, 8, 64, generator=g).mul(0.5).to(dev) for n in (7, 5, 5))
    proj = torch.randn(266, 64, generator=g).to(dev)
    dout = torch.randn(2, 7, 512, generator=g).to(dev)
    out0, ws0 = L.favor_fwd(q, k, v, proj)
    g0 = L.favor_bwd(q, k, v, proj, out0, dout, ws0)
    ex = mdist.StabiliserExchange(dedicated_group=True)
    xb = torch.zeros(4, device=dev)
    out1, ws1 = L.favor_fwd(q, k, v, proj, exchange=(ex, xb))
    g1 = L.favor_bwd(q, k, v, proj, out1, dout, ws1, exchange=(ex, xb))
    torch.cuda.synchronize()
    same = torch.equal(out0, out1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    out["res"] = (logs, same, list(ex.calls))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_world_of_one_grad_bucket_and_stabiliser_exchange(gpulib):
    """The N > 1 data path meets the real backend before an 8-GPU node does (VERDICT r3 item 5 ii): a process group over
    backend "nccl" - RCCL - at world size 1 on this box's GPU with the world == 1 shortcuts disabled, GradBucket(side_stream=True,
    early=...) issuing its all-reduces from inside backward() on the communication stream, StabiliserExchange on a dedicated
    group between the staged FAVOR+ calls.  Proves that librccl loads, that the event / record_stream ordering against RCCL's
    kernels holds (gradients bit-identical to the un-reduced ones) and that the staged path through RCCL equals the unstaged one."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        p = ctx.Process(target=_rccl_one_worker, args=(port, out))
        p.start()
        p.join(600)
        assert p.exitcode == 0
        logs, same, calls = out["res"]
        assert logs == {"side stream": ["all"], "early + side stream": ["early", "rest"]}
        assert same and calls == ["fwd", "bwd"]


@pytest.mark.parametrize("workload,extra", [("c3", []), ("c5", []), ("c5", ["--one-graph"]), ("c5", ["--strict"])], ids=["c3", "c5", "c5_one_graph", "c5_strict"])
def test_rccl_world_of_one_bench(gpulib, workload, extra):
    """bench.py --gpus 1 with the collectives forced over backend "nccl": the timing protocol's barrier / MAX all-reduce, the
    gradient bucket behind the hipGraph replay and - with --strict - the eager step with the batch-global key stabiliser, all
    through RCCL; the JSON line says which stabiliser form ran.  c5 (ResNet family): the replayed step is TWO graphs with the
    early bucket's all-reduce issued between them (`collectives_per_step` == early, rest); --one-graph keeps the single graph and
    its one collective - same loss either way."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MLHOT_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--workload", workload,
           "--no-cpu-baseline", "--no-extras", "--prof-steps", "1"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root, timeout=600)
    if r.returncode != 0:
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", f"rccl_bench_{workload}{'_strict' if extra else ''}.stderr"), "w") as f:
            f.write(r.stderr)
    assert r.returncode == 0, r.stderr[:3000] + "\n...\n" + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 4
    if extra == ["--strict"]:
        assert out["hipgraph"] is False and out["key_stabiliser"].startswith("batch-global")
    else:
        assert out["hipgraph"] is True and out["key_stabiliser"].startswith("rank-local")
        kinds = [k for k, _ in out["dist"]["collectives_per_step"]]
        if workload == "c5" and not extra:
            assert out["dist"]["step_graphs"] == 2 and kinds == ["early", "rest"], out["dist"]
            sizes = [n for _, n in out["dist"]["collectives_per_step"]]
            assert sizes[0] > 2 * sizes[1]               # the early bucket is the larger part (11.6 of 15.1 MB)
        else:
            assert out["dist"]["step_graphs"] == 1 and kinds == ["all"], out["dist"]
        if workload == "c5":
            _C5_LOSSES[tuple(extra)] = out["final_loss"]
            if len(_C5_LOSSES) == 2:
                a, b = _C5_LOSSES.values()
                assert abs(a - b) <= 1e-6 * abs(a), _C5_LOSSES
    assert "key stabiliser" in r.stderr


_C5_LOSSES = {}


@pytest.mark.parametrize("method", ["ANPMRShapeNet3D", "ANP", "CondNeuralProcess"])
def test_backward_in_two_equals_one_backward(gpulib, method):
    """mlhot.dist.backward_in_two on a forward cut in front of the image trunks (ResNetNP.enable_split_backward): part 1 leaves every
    early-bucket parameter with its FINAL gradient and no trunk parameter with any (that is the moment the caller issues the early
    all-reduce), part 2 adds the trunks' - and the result is bit-identical to the one-piece loss.backward()."""
    import importlib
    import types
    from mlhot import dist as mdist
    from mlhot.ops import add_scaled
    from mlhot.synth import get_batch_3d
    from trainer.losses import LossFunc
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=2, input_dim=4, output_dim=4,
                                agg_mode="attention" if method != "CondNeuralProcess" else "max", img_agg="reshape" if method == "ANPMRShapeNet3D" else "max",
                                task="shapenet_3d", temperature=0.07)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
    cx, qx, cy, qy = (t.to(DEV) for t in get_batch_3d(2, 4, 5, seed=3))
    loss_fn = LossFunc("mse", "shapenet_3d")
    early = {id(p) for p in model.early_grad_parameters()}

    def run(split):
        model.enable_split_backward(split)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7)                              # the Bayes-by-backprop eps
        mu, var, kl = model(cx, cy, qx)
        loss = add_scaled(loss_fn.calc_loss(mu, var, qy), kl, 1e-3)
        seen = {}
        if split:
            def between():
                seen["early"] = {k: p.grad.clone() for k, p in model.named_parameters() if id(p) in early and p.grad is not None}
                seen["late_none"] = all(p.grad is None for p in model.parameters() if id(p) not in early)
            mdist.backward_in_two(loss, model, between=between)
        else:
            loss.backward()
        torch.cuda.synchronize()
        return loss.item(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, seen

    l0, g0, _ = run(False)
    l1, g1, seen = run(True)
    model.enable_split_backward(False)
    assert l0 == l1 and g0.keys() == g1.keys() and len(g0) > 20
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert seen["late_none"] and len(seen["early"]) > 10
    for k, g in seen["early"].items():
        assert torch.equal(g, g1[k]), k                   # complete before the trunks' backward ran


def _strict_worker(rank, world, port, name, opts, out):
    import copy
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "what-matters-for-meta-learning_amd"), root]
    import torch.distributed as dist
    import mlhot
    from mlhot import dist as mdist, ops
    from trainer.losses import LossFunc
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    mdist.init_from_env("gloo")                     # two ranks sharing the box's one GPU: gloo carries the device scalars
    torch.cuda.set_device(0)
    for k, v in opts.items():
        mlhot.lib().set_option(k, v)
    fx, meta = U.load_case(name)
    full = U.build_model(meta, DEV, fx=fx).to(DEV)
    T = meta["cfg"]["tasks_per_batch"]
    smeta = copy.deepcopy(meta)
    smeta["cfg"]["tasks_per_batch"] = T // world
    shard = getattr(importlib.import_module("networks." + meta["method"]), meta["method"])(U.case_config(smeta, DEV)).to(DEV)
    shard.load_state_dict(full.state_dict())
    cx, qx, cy, qy = U.resnet_case_inputs(meta, fx) if name.startswith("r_") else U.case_inputs(meta)
    lossf = LossFunc("mse", meta["cfg"]["task"])

    def run(model, sl, exchange):
        ops.set_stabiliser_exchange(exchange)
        try:
            for p in model.parameters():
                p.grad = None
            mu, var, _ = model(cx[sl].to(DEV), cy[sl].to(DEV), qx[sl].to(DEV))
            loss = lossf.calc_loss(mu, var, qy[sl].to(DEV))
            loss.backward()
        finally:
            ops.set_stabiliser_exchange(None)
        return mu.detach().clone(), loss.detach().clone()

    sl = mdist.task_slice(T, rank, world)
    mu_full, loss_full = run(full, slice(0, T), None)
    gfull = {k: p.grad.clone() for k, p in full.named_parameters() if p.grad is not None}
    floor = U.GRAD_FLOOR * max(float(g.abs().max()) for g in gfull.values())
    res = {}
    for mode, ex in (("rank-local", None), ("strict", mdist.StabiliserExchange())):
        mu, loss = run(shard, sl, ex)
        mdist.GradBucket(shard.parameters()).sync()
        lsum = loss.clone()
        dist.all_reduce(lsum)
        res[mode] = dict(mu_equal=bool(torch.equal(mu, mu_full[sl])), mu_err=U.rel_err(mu, mu_full[sl]),
                         loss_err=abs(float(lsum) / world - float(loss_full)) / max(1.0, abs(float(loss_full))),
                         grad_err=max(U.rel_err(p.grad, gfull[k], floor=floor) for k, p in shard.named_parameters() if k in gfull),
                         calls=list(ex.calls) if ex else [])
    # a world of one through the staged entry points reproduces the unstaged pass bit for bit (x[1] = 1: this rank owns the maximum)
    class Alone(mdist.StabiliserExchange):
        def _world(self):
            return 1
    mu1, _ = run(full, slice(0, T), Alone())
    res["alone"] = bool(torch.equal(mu1, mu_full)) and all(torch.equal(p.grad, gfull[k]) for k, p in full.named_parameters() if k in gfull)
    torch.cuda.synchronize()
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name,opts", [("s_anp_shapenet1d_t2_full", {}), ("s_anp_shapenet1d_ragged", {}), ("s_anp_shapenet1d_ragged", {"tail_spec": 0}),
                                       ("r_anp_shapenet3d", {}), ("r_anp_shapenet3d", {"favor2": 0})],
                         ids=["anp1d_15+15", "anp1d_ragged", "anp1d_ragged_generic_tail", "resnet_anp_favor2", "resnet_anp_favor_chain"])
def test_strict_sharded_parity_on_two_ranks(gpulib, name, opts):
    """config.strict_sharded_parity (fast_attention.py:96-97): two gloo ranks share this box's GPU, each owns one
    of the batch's two tasks.  Through the staged entry points (mlhot_np_vanilla_*_staged for the vanilla ANP's fused tail,
    mlhot_favor_*_staged for the ResNet family - both FAVOR+ implementations) + mlhot.dist.StabiliserExchange the shard's outputs are
    BIT-IDENTICAL to the same tasks' rows of the un-sharded batch and the averaged gradients equal the un-sharded gradients to
    float rounding; with the rank-local stabiliser (the default) the rank that does not hold the batch maximum differs."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        procs = [ctx.Process(target=_strict_worker, args=(r, 2, port, name, opts, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
            assert p.exitcode == 0
        res = {r: dict(out[r]) for r in range(2)}
    print(f"{name} {opts}: " + "; ".join(
        f"rank {r} {m}: mu {'==' if res[r][m]['mu_equal'] else '%.1e' % res[r][m]['mu_err']} loss {res[r][m]['loss_err']:.1e} "
        f"grad {res[r][m]['grad_err']:.1e}" for r in range(2) for m in ("rank-local", "strict")))
    for r in range(2):
        assert res[r]["alone"]
        st = res[r]["strict"]
        assert st["mu_equal"] and st["loss_err"] <= 1e-6 and st["grad_err"] <= 2e-6, (r, st)
        assert st["calls"] == ["fwd", "bwd"]
    # the default: exactly one rank (the one without the batch's largest key) computes with another stabiliser
    assert sorted(res[r]["rank-local"]["mu_equal"] for r in range(2)) == [False, True]
    assert max(res[r]["rank-local"]["mu_err"] for r in range(2)) <= 1e-4        # ... a small effect, as SURVEY 8e(i) says


def test_cpu_tensors_are_refused(gpulib):
    from mlhot.binding import MlhotError
    from mlhot.ops import LinearFunction
    with pytest.raises(MlhotError):
        LinearFunction.apply(torch.randn(2, 3), torch.randn(4, 3), None, "none")
