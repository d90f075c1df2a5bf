"""One case per torch.autograd.Function of mlhot.ops (a few have two or three), shared by tests/test_autograd_seam_cpu.py (the
completeness guard) and tests/test_autograd_seam_gpu.py (the variants: views, frozen inputs, twice, shared leaves, ...).

A case lists the tensor inputs of one smallest call that still reaches the Function's kernels, how to call the Function on them, and
a float64 torch composition of the same operation on the same float32 values (`ref`; None for the three whole-model Functions, whose
values the parity tests hold: their variants are compared bit for bit with their own plain run only).  Inputs, references and bounds
are the families' own (favor_cases, agg_loss_cases, ntx_cases, glue_ops, conv_cases' rule, the Bayes-by-backprop and chain
references and the trunk's weight recipe that used to live in test_gpu_parity.py); anything without a family bound is held at util.RTOL.

Case fields:
  function   name of the class in mlhot.ops
  tensors    [(name, float32 CPU tensor, differentiable)]
  call       (ops module, tensors on the device in that order) -> tuple of output tensors
  ref        (float64 tensors in that order) -> tuple of float64 outputs, or None
  judge      {quantity: (got, want) -> (error, bound)}; quantities are "out<i>" and "d<input name>"; default rel_err at util.RTOL.
             ("e32", tol) stands for rel_err at tol + 2 x the error of the float32 run of `ref` against its float64 run (judge_of)
  nondiff    indices of outputs that carry no gradient
  fixed      inputs whose contract is a contiguous buffer of the caller's (stacked head weights, the projection): never made views
  mutable    inputs the Function updates in place by contract (batch norm's running statistics)
  flags      inputs whose gradient the binding can skip by launching less (a need_* flag of the entry): freezing them changes the launches
  job_flags  inputs whose need_* flag is a field of a job inside ONE launch that also computes the other gradients: the launches stay
  offset     the entry takes operands that are only 4-byte aligned (include/mlhot.h); every other entry demands 16 bytes"""
import functools
import types

import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import agg_loss_cases as AL
from tests import favor_cases as FC
from tests import glue_ops as G
from tests import ntx_cases as NC
from tests import util as U


# ---- references shared with tests/test_gpu_parity.py ------------------------------------------------------------------------
def _chain_reference(x0, layers):
    """torch autograd restatement of a chain: layers = [(w, b, act, side | None, side_first)]."""
    h = x0
    for w, b, act, side, side_first in layers:
        if side is not None:
            h = torch.cat([side, h] if side_first else [h, side], dim=-1)
        h = F.linear(h, w, b)
        h = torch.relu(h) if act == "relu" else torch.tanh(h) if act == "tanh" else h
    return h


def _bbb_ref(mus, rhos, epss, wouts, dkl):
    """autograd of sum_i <w_i, wout_i> + dkl * kl with w = mu + eps * softplus(rho), kl as bbb/BBBConv.py:33-35,100-108."""
    mr = [(m.clone().requires_grad_(), r.clone().requires_grad_()) for m, r in zip(mus, rhos)]
    ws, kl = [], 0.0
    for (m, r), e in zip(mr, epss):
        sigma = torch.log1p(torch.exp(r))
        ws.append(m + e * sigma)
        kl = kl + 0.5 * (2 * torch.log(sigma / 0.1) - 1 + (0.1 / sigma).pow(2) + (m / sigma).pow(2)).sum()
    total = dkl * kl
    for w, wo in zip(ws, wouts):
        if wo is not None:
            total = total + (w * wo).sum()
    total.backward()
    return [w.detach() for w in ws], kl.detach(), [m.grad for m, _ in mr], [r.grad for _, r in mr]


def _trunk_weights(C, skip_k, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(64, C, 5, 5)] + [s_ for _ in range(4) for s_ in ((64, 64, 3, 3), (64, 64, 3, 3), (64, 64, skip_k, skip_k))]
    out = []
    for sh in shapes:
        fan = sh[1] * sh[2] * sh[3]
        out += [torch.randn(*sh, generator=g) * (1.5 / fan) ** 0.5, torch.randn(sh[0], generator=g) * 0.1]
    return out


def _bbb_draw(mu, rho, eps):
    """One sample and its KL term, the formulas of _bbb_ref as a differentiable composition."""
    sigma = torch.log1p(torch.exp(rho))
    return mu + eps * sigma, 0.5 * (2 * torch.log(sigma / 0.1) - 1 + (0.1 / sigma).pow(2) + (mu / sigma).pow(2)).sum()


# ---- judges -----------------------------------------------------------------------------------------------------------------
def rtol(got, want):
    return U.rel_err(got, want), U.RTOL


def at(bound, floor=0.0):
    return lambda got, want: (U.rel_err(got, want, floor), bound)


def _act(act, t):
    return torch.relu(t) if act == "relu" else torch.tanh(t) if act == "tanh" else t


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(function, name, tensors, call, ref, judge=None, nondiff=(), fixed=(), mutable=(), flags=(), job_flags=(), offset=False):
    return types.SimpleNamespace(function=function, name=name, tensors=tensors, call=call, ref=ref, judge=judge or {}, nondiff=tuple(nondiff),
                                 fixed=tuple(fixed), mutable=tuple(mutable), flags=tuple(flags), job_flags=tuple(job_flags), offset=offset)


# ---- the Linear family: M = 7, K = 16 / 20, N = 12 ----------------------------------------------------------------------------
def _linear():
    g = _gen(1)
    x, w, b = torch.randn(1, 7, 20, generator=g), torch.randn(12, 20, generator=g) * 20 ** -0.5, torch.randn(12, generator=g) * 0.1
    return _case("LinearFunction", "linear_7x20x12_tanh", [("x", x, True), ("w", w, True), ("b", b, True)],
                 lambda ops, t: (ops.LinearFunction.apply(t[0], t[1], t[2], "tanh"),), lambda t: (torch.tanh(F.linear(t[0], t[1], t[2])),),
                 flags=("x",), offset=True)


def _heads(g, n_stacks, h=2, n=6, k=16):
    """Per stack: x [1, 7, k], the stacked weight [h n, k] and bias [h n], then the heads' own tensors holding the same values."""
    xs = [torch.randn(1, 7, k, generator=g) for _ in range(n_stacks)]
    ws = [torch.randn(h * n, k, generator=g) * k ** -0.5 for _ in range(n_stacks)]
    bs = [torch.randn(h * n, generator=g) * 0.1 for _ in range(n_stacks)]
    return xs, ws, bs


def _stacked_linear():
    (x,), (w,), (b,) = _heads(_gen(2), 1)
    tensors = [("x", x, True), ("stack_w", w, False), ("stack_b", b, False)]
    tensors += [(f"w{i}", w.view(2, 6, 16)[i].clone(), True) for i in range(2)] + [(f"b{i}", b.view(2, 6)[i].clone(), True) for i in range(2)]
    return _case("StackedLinearFunction", "stacked_linear_7x16_2x6", tensors,
                 lambda ops, t: (ops.StackedLinearFunction.apply(t[0], t[1], t[2], 2, *t[3:]),),
                 lambda t: (F.linear(t[0], torch.cat(t[3:5]), torch.cat(t[5:7])),), fixed=("stack_w", "stack_b"), flags=("x",), offset=True)


def _linear2():
    g = _gen(3)
    xa, xb = torch.randn(7, 16, generator=g), torch.randn(7, 4, generator=g)
    w, b = torch.randn(12, 20, generator=g) * 20 ** -0.5, torch.randn(12, generator=g) * 0.1
    return _case("Linear2Function", "linear2_7x16+4x12_relu", [("xa", xa, True), ("xb", xb, True), ("w", w, True), ("b", b, True)],
                 lambda ops, t: (ops.Linear2Function.apply(t[0], t[1], t[2], t[3], "relu"),),
                 lambda t: (torch.relu(F.linear(torch.cat([t[0], t[1]], -1), t[2], t[3])),), job_flags=("xa", "xb"))


def _mlp_chain():
    g = _gen(4)
    x0, side = torch.randn(7, 16, generator=g), torch.randn(7, 4, generator=g)
    w0, b0 = torch.randn(12, 20, generator=g) * 20 ** -0.5, torch.randn(12, generator=g) * 0.1
    w1 = torch.randn(8, 12, generator=g) * 12 ** -0.5
    spec = (("relu", True, True, False), ("tanh", False, False, False))
    return _case("MlpChainFunction", "mlp_chain_7x16+4_12_8", [("x0", x0, True), ("w0", w0, True), ("b0", b0, True), ("side", side, True), ("w1", w1, True)],
                 lambda ops, t: (ops.MlpChainFunction.apply(spec, t[0], t[1], t[2], t[3], t[4]),),
                 lambda t: (_chain_reference(t[0], [(t[1], t[2], "relu", t[3], False), (t[4], None, "tanh", None, False)]),), job_flags=("x0", "side"))


def _head_stacks():
    xs, ws, bs = _heads(_gen(5), 2)
    tensors = []
    for i in range(2):
        tensors += [(f"x{i}", xs[i], True), (f"stack_w{i}", ws[i], False), (f"stack_b{i}", bs[i], False)]
    for i in range(2):
        tensors += [(f"w{i}{k}", ws[i].view(2, 6, 16)[k].clone(), True) for k in range(2)] + [(f"b{i}{k}", bs[i].view(2, 6)[k].clone(), True) for k in range(2)]

    def ref(t):
        return tuple(F.linear(t[3 * i], torch.cat(t[6 + 4 * i:8 + 4 * i]), torch.cat(t[8 + 4 * i:10 + 4 * i])).view(1, 7, 2, 6) for i in range(2))
    return _case("HeadStacksFunction", "head_stacks_2x(7x16_2x6)", tensors, lambda ops, t: tuple(ops.HeadStacksFunction.apply(2, 2, *t)), ref,
                 fixed=("stack_w0", "stack_b0", "stack_w1", "stack_b1"))


def _scaled_add():
    g = _gen(6)
    a, x = torch.randn(5, 3, generator=g), torch.randn(5, 3, generator=g)
    alpha = float(torch.tensor(0.37, dtype=torch.float32))
    return _case("ScaledAddFunction", "scaled_add_5x3", [("a", a, True), ("x", x, True)], lambda ops, t: (ops.ScaledAddFunction.apply(t[0], t[1], alpha),),
                 lambda t: (t[0] + alpha * t[1],), flags=("x",))


# ---- aggregators: T 2, Nc 3, R 64 -------------------------------------------------------------------------------------------
def _column(got, want):
    return AL.column_err(got, want), U.RTOL


def _agg(mode):
    shape = (2, 3, 64)
    if mode == "baco":
        rs, lv, _ = AL.baco_inputs(shape, "randn2")
        return _case("AggFunction", "agg_baco_2x3x64", [("rs", rs, True), ("lv", lv, True)], lambda ops, t: tuple(ops.AggFunction.apply("baco", t[0], t[1])),
                     lambda t: tuple(O.agg_baco(t[0], 1e-5 + F.softplus(t[1]))), judge={"out0": _column, "out1": _column, "drs": _column, "dlv": _column},
                     nondiff=(1,))
    rs, _ = AL.mean_inputs(shape) if mode == "mean" else AL.max_inputs(shape)
    arg = AL.first_greater_scan(rs)[1].long().unsqueeze(1)          # the stored convention: the first maximum in shot order wins

    def ref(t):
        return (t[0].mean(dim=1) if mode == "mean" else t[0].gather(1, arg).squeeze(1),)
    return _case("AggFunction", f"agg_{mode}_2x3x64", [("rs", rs, True)], lambda ops, t: (ops.AggFunction.apply(mode, t[0], None)[0],), ref,
                 judge={"out0": _column, "drs": _column})


# ---- FAVOR+: both sides <= 32 (two launches) and Nc = 33 (the chain) ----------------------------------------------------------
def _favor(name):
    c = FC.BY_NAME[name]
    q, k, v, _, proj = FC.kernel_layout(FC.inputs(name))
    bound = FC.bounds(c)

    def ref(t):
        out = O.favor_attention(t[0].permute(0, 2, 1, 3), t[1].permute(0, 2, 1, 3), t[2].permute(0, 2, 1, 3), t[3])
        return (out.permute(0, 2, 3, 1).reshape(c.T, c.Nq, c.d * c.H),)
    return _case("FavorFunction", "favor_" + name, [("q", q, True), ("k", k, True), ("v", v, True), ("proj", proj, False)],
                 lambda ops, t: (ops.FavorFunction.apply(*t),), ref,
                 judge={"out0": at(bound["out"]), "dq": at(bound["dq"]), "dk": at(bound["dk"]), "dv": at(bound["dv"])}, fixed=("proj",))


# ---- losses: every kind LossFunc has ------------------------------------------------------------------------------------------
LOSS_ROWS = 5


def _value(got, want):
    return abs(float(got) - float(want)), AL.value_bound(float(want))


def _loss_ref(case):
    task, test = AL.TASK[case[0]]

    def ref(t):
        value = O.calc_loss(task, t[0], t[1], test=test)
        return (value.detach() + 0.0 * t[0].sum() if test else value,)      # the degree error is evaluation-only: its gradient is all zeros
    return ref


def _loss(case):
    mu, gt = AL.loss_inputs(case, LOSS_ROWS)
    return _case("LossFunction", "loss_" + AL.ids(case), [("mu", mu[0], True), ("gt", gt, False)], lambda ops, t: (ops.LossFunction.apply(case[0], t[0], t[1]),),
                 _loss_ref(case), judge={"out0": _value})


def _loss_plus():
    case = ("mse", 3, 3)
    mu, gt = AL.loss_inputs(case, LOSS_ROWS)
    x, alpha = torch.tensor(3.0), 0.5
    inner = _loss_ref(case)
    return _case("LossPlusFunction", "loss_plus_mse", [("mu", mu[0], True), ("gt", gt, False), ("x", x, True)],
                 lambda ops, t: (ops.LossPlusFunction.apply("mse", t[0], t[1], t[2], alpha),), lambda t: (inner(t)[0] + alpha * t[2],),
                 judge={"out0": _value}, job_flags=("x",))


def _ntxent():
    c = NC.BY_NAME["d16_N17"]
    z = NC.inputs(c.name)

    def ref(t):
        zn = t[0] / t[0].norm(dim=1, keepdim=True).clamp_min(NC.NORM_FLOOR)
        return (NC._loss_of_zn(zn, NC.labels(c), c.t)[0],)
    return _case("NTXentFunction", "nt_xent_" + c.name, [("z", z, True)], lambda ops, t: (ops.NTXentFunction.apply(t[0], c.div, c.mod, c.t),), ref,
                 judge={"out0": lambda got, want: (abs(float(got) - float(want)), NC.loss_bound(c, want)), "dz": lambda got, want: (NC.dz_err(c, got, want), U.RTOL)})


# ---- the ResNet family's pieces -------------------------------------------------------------------------------------------------
CONV = dict(N=2, Cin=3, H=9, W=9, Cout=6, k=3, s=2, p=1)
CONV_TOL = dict(out0=1e-5, dx=2e-5, dw=2e-5, db=2e-5)           # tests/conv_cases.py TOL


def _conv_inputs():
    g = _gen(7)
    c = CONV
    x = torch.randn(c["N"], c["Cin"], c["H"], c["W"], generator=g)
    w = torch.randn(c["Cout"], c["Cin"], c["k"], c["k"], generator=g) / (c["Cin"] * c["k"] * c["k"]) ** 0.5
    return x, w, torch.randn(c["Cout"], generator=g)


def _conv2d():
    x, w, b = _conv_inputs()
    # conv_cases' rule for a shape outside its table: its tolerance plus twice the error of the float32 run of the reference
    judge = {n: ("e32", tol) for n, tol in CONV_TOL.items()}
    return _case("Conv2dFunction", "conv2d_2x3x9x9_O6_k3_s2_p1_relu", [("x", x, True), ("w", w, True), ("b", b, True)],
                 lambda ops, t: (ops.Conv2dFunction.apply(t[0], t[1], t[2], CONV["s"], CONV["p"], True),),
                 lambda t: (torch.relu(F.conv2d(t[0], t[1], t[2], stride=CONV["s"], padding=CONV["p"])),), judge=judge, flags=("x",))


def _add_relu():
    a, b = G.add_relu_inputs(35)
    return _case("AddReluFunction", "add_relu_5x7", [("a", a.view(5, 7).clone(), True), ("b", b.view(5, 7).clone(), True)],
                 lambda ops, t: (ops.AddReluFunction.apply(t[0], t[1]),), lambda t: (torch.relu(t[0] + t[1]),))


def _max_pool2():
    x = G.POOL_VALUES[torch.randint(0, 5, (1, 3, 4, 6), generator=_gen(8))]
    return _case("MaxPool2Function", "max_pool2_1x3x4x6", [("x", x, True)], lambda ops, t: (ops.MaxPool2Function.apply(t[0]),),
                 lambda t: (F.max_pool2d(t[0], 2),))


def _bbb_inputs(shapes, seed):
    g = _gen(seed)
    return ([torch.randn(*s, generator=g) * 0.1 for s in shapes], [torch.randn(*s, generator=g) * 0.5 - 3.0 for s in shapes],
            [torch.randn(*s, generator=g) for s in shapes])


BBB_JUDGE = dict(w=at(1e-6), kl=at(1e-5), grad=at(1e-5))        # the bounds of test_bbb_sample_*_vs_autograd


def _bbb_sample():
    (mu,), (rho,), (eps,) = _bbb_inputs([(7,)], 9)
    return _case("BBBSampleFunction", "bbb_sample_7", [("mu", mu, True), ("rho", rho, True), ("eps", eps, False)],
                 lambda ops, t: tuple(ops.BBBSampleFunction.apply(*t)), lambda t: _bbb_draw(*t),
                 judge={"out0": BBB_JUDGE["w"], "out1": BBB_JUDGE["kl"], "dmu": BBB_JUDGE["grad"], "drho": BBB_JUDGE["grad"]})


def _bbb_sample_multi():
    mus, rhos, epss = _bbb_inputs([(7,), (5, 3)], 10)
    tensors = [("mu0", mus[0], True), ("rho0", rhos[0], True), ("mu1", mus[1], True), ("rho1", rhos[1], True), ("eps0", epss[0], False), ("eps1", epss[1], False)]

    def ref(t):
        (w0, k0), (w1, k1) = _bbb_draw(t[0], t[1], t[4]), _bbb_draw(t[2], t[3], t[5])
        return w0, w1, k0 + k1
    judge = {"out0": BBB_JUDGE["w"], "out1": BBB_JUDGE["w"], "out2": BBB_JUDGE["kl"]}
    judge.update({"d" + n: BBB_JUDGE["grad"] for n in ("mu0", "rho0", "mu1", "rho1")})
    return _case("BBBSampleMultiFunction", "bbb_sample_multi_7_5x3", tensors, lambda ops, t: tuple(ops.BBBSampleMultiFunction.apply([t[4], t[5]], *t[:4])), ref,
                 judge=judge)


BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def _batch_norm():
    x, gamma, beta, rm, rv, _ = G.bn_inputs((6, 8, 16))
    x = x.view(6, 8, 4, 4).clone()
    tensors = [("x", x, True), ("gamma", gamma, True), ("beta", beta, True), ("run_mean", rm, False), ("run_var", rv, False)]
    return _case("BatchNormReluFunction", "bn_relu_6x8x4x4", tensors, lambda ops, t: (ops.BatchNormReluFunction.apply(*t, BN_MOMENTUM, BN_EPS),),
                 lambda t: (torch.relu(F.batch_norm(t[0], None, None, t[1], t[2], training=True, momentum=BN_MOMENTUM, eps=BN_EPS)),),
                 fixed=("run_mean", "run_var"), mutable=("run_mean", "run_var"))


def _spatial_mean():
    x = 3.0 + torch.randn(2, 5, 3, 3, generator=_gen(11))
    return _case("SpatialMeanFunction", "spatial_mean_2x5x3x3", [("x", x, True)], lambda ops, t: (ops.SpatialMeanFunction.apply(t[0]),),
                 lambda t: (t[0].mean(dim=(2, 3)),))


# ---- the three whole-model Functions at one task, one or two images per pass: no float64 leg -----------------------------------
def _enc_vanilla():
    p = U.enc_params(64)
    img = torch.rand(2, 1, 128, 128, generator=_gen(12))
    tensors = [("img", img, False)] + [(k.split("encoder_w0.")[1], v, True) for k, v in p.items()]
    return _case("EncVanillaFunction", "enc_vanilla_2_images", tensors, lambda ops, t: (ops.EncVanillaFunction.apply(*t),), None)


def _vanilla_np(agg):
    import importlib
    method = "ANPShapeNet1D" if agg == "attention" else "CNPShapeNet1D"
    cfg = types.SimpleNamespace(device=torch.device("cpu"), seed=2578, img_size=[128, 128, 1], tasks_per_batch=1, input_dim=3, output_dim=2,
                                agg_mode=agg, img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d")
    with torch.random.fork_rng(devices=[]):
        model = getattr(importlib.import_module("networks." + method), method)(cfg)
    keys = tuple(k for k, _ in model.named_parameters())
    proj = model.attn.projection_matrix.detach().clone() if agg == "attention" else None
    g = _gen(13)
    Nc, Nq = 2, 1
    tensors = [("ctx_x", torch.rand(1, Nc, 1, 128, 128, generator=g), False), ("ctx_y", torch.rand(1, Nc, 3, generator=g), False),
               ("qry_x", torch.rand(1, Nq, 1, 128, 128, generator=g), False)]
    tensors += [(k, p.detach().clone(), True) for k, p in model.named_parameters()]
    if proj is not None:
        tensors.append(("proj", proj, False))
    n = 3 + len(keys)

    def call(ops, t):
        from mlhot import lib
        dims = lib().np_dims(1, Nc, Nq, 3, 2, 64, 64, 64, [100, 100], 100, agg, True, proj.shape[0] if proj is not None else 0)
        return (ops.VanillaNPFunction.apply(dims, keys, t[n] if proj is not None else None, t[0], t[1], t[2], *t[3:n]),)
    return _case("VanillaNPFunction", f"vanilla_np_{agg}_T1_Nc{Nc}_Nq{Nq}", tensors, call, None, fixed=("proj",) if proj is not None else ())


def _resnet_trunk():
    g = _gen(14)
    skips = (1, 3)
    imgs = [torch.rand(1, 3, 64, 64, generator=g) for _ in skips]
    tensors = [(f"img{i}", t, False) for i, t in enumerate(imgs)]
    for i, k in enumerate(skips):
        tensors += [(f"ws{i}.{j}", t, True) for j, t in enumerate(_trunk_weights(3, k, 1 + i))]
    spec = (((0, 0), (1, 1)), skips, 2, None)
    return _case("ResNetTrunkFunction", "resnet_trunk_C3_H64_skip1_skip3", tensors, lambda ops, t: tuple(ops.ResNetTrunkFunction.apply(spec, *t)), None)


BUILDERS = [
    ("LinearFunction", _linear), ("StackedLinearFunction", _stacked_linear), ("Linear2Function", _linear2), ("MlpChainFunction", _mlp_chain),
    ("HeadStacksFunction", _head_stacks), ("ScaledAddFunction", _scaled_add),
    ("AggFunction", lambda: _agg("mean")), ("AggFunction", lambda: _agg("max")), ("AggFunction", lambda: _agg("baco")),
    ("FavorFunction", lambda: _favor("T1_H2_Nq16_Nc16_d32_m110")), ("FavorFunction", lambda: _favor("T2_H2_Nq12_Nc33_d64_m266")),
] + [("LossFunction", functools.partial(_loss, c)) for c in AL.TRAIN_KINDS + [("degree", 2, 1)]] + [
    ("LossPlusFunction", _loss_plus), ("NTXentFunction", _ntxent), ("Conv2dFunction", _conv2d), ("AddReluFunction", _add_relu),
    ("MaxPool2Function", _max_pool2), ("BBBSampleFunction", _bbb_sample), ("BBBSampleMultiFunction", _bbb_sample_multi),
    ("BatchNormReluFunction", _batch_norm), ("SpatialMeanFunction", _spatial_mean), ("EncVanillaFunction", _enc_vanilla),
    ("VanillaNPFunction", lambda: _vanilla_np("attention")), ("VanillaNPFunction", lambda: _vanilla_np("max")), ("ResNetTrunkFunction", _resnet_trunk),
]
FUNCTIONS = sorted({f for f, _ in BUILDERS})


@functools.lru_cache(maxsize=None)
def _built(i):
    c = BUILDERS[i][1]()
    assert c.function == BUILDERS[i][0], (c.function, BUILDERS[i][0])
    return c


def cases():
    """Every case, built once; callers must not write into the tensors."""
    return [_built(i) for i in range(len(BUILDERS))]


@functools.lru_cache(maxsize=None)
def reference(i, dtype=torch.float64):
    """(outputs, {input name: gradient}) of case i's composition run in `dtype` for the upstream gradients upstream(case, outputs), or
    None.  Computed once; callers must not write into them."""
    c = _built(i)
    if c.ref is None:
        return None
    t = [v.to(dtype).clone().requires_grad_(d) for _, v, d in c.tensors]
    outs = c.ref(t)
    ups = upstream(c, outs)
    live = [(o, u.to(dtype)) for k, (o, u) in enumerate(zip(outs, ups)) if k not in c.nondiff]
    wrt = [v for v, (_, _, d) in zip(t, c.tensors) if d]
    grads = torch.autograd.grad([o for o, _ in live], wrt, [u for _, u in live], allow_unused=True)
    names = [n for n, _, d in c.tensors if d]
    return [o.detach() for o in outs], dict(zip(names, grads))


def judge_of(i, quantity):
    """The judge of one quantity of case i: (got, want) -> (error, bound)."""
    j = _built(i).judge.get(quantity, rtol)
    if not isinstance(j, tuple):
        return j
    (o32, g32), (o64, g64) = reference(i, torch.float32), reference(i)
    pick = (lambda o, g: o[int(quantity[3:])]) if quantity.startswith("out") else (lambda o, g: g[quantity[1:]])
    return at(j[1] + 2.0 * U.rel_err(pick(o32, g32), pick(o64, g64)))


def upstream(case, outs):
    """One float32 N(0, 1) upstream gradient per output, a function of the case's name and the outputs' shapes alone."""
    g = _gen(sum(map(ord, case.name)))
    return [torch.randn(tuple(o.shape), generator=g) for o in outs]
