"""The autograd seam on the MI355X: every torch.autograd.Function of mlhot.ops (tests/autograd_cases.py) the way callers may use it, not
only the way the shipped models do - inputs that are views, inputs without a gradient, a second backward, leaves shared by two
nodes - and the gradient arena (mlhot/arena.py) under the calling patterns autograd allows.

plain    contiguous inputs, every differentiable input requires grad: against the float64 composition at the family's bound
views    every input a non-contiguous view of a larger buffer, the upstream gradient a transposed view and (second run) the
         stride-0 expansion of out.sum().backward(): bit-equal to plain, gradients of the inputs' shapes, no buffer changed
offset   contiguous operands one float into their buffer (is_contiguous() true, not 16-byte aligned).  The Linear pair's entries take
         4-byte alignment and may run another route: judged against float64.  Every other entry demands 16 bytes: the Function copies
         such an operand (bit-equal to plain, plain's launches) or, where it cannot - a buffer updated in place, a stacked weight the
         heads are views of - refuses with MlhotError before any launch.  No kernel ever runs on a misaligned pointer
frozen   each differentiable input in turn without a gradient: .grad stays None, the others bit-equal to plain; the launch labels
         change where the binding's need_* flag for that input drops a launch, and are unchanged where the flag is a field of a
         one-launch job (Linear2, MlpChain, LossPlus: the label cannot show it) or the entry has no flag
one_live every differentiable input but one frozen (the Functions with several inputs)
twice    backward(retain_graph=True) and a second backward on the same graph: plain + plain
shared   one leaf under two nodes of one graph"""
import pytest
import torch
import torch.nn.functional as F

from tests import autograd_cases as AC
from tests import util as U
from tests.glue_ops import bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = AC.cases()
IDS = [c.name for c in CASES]
INDEX = {c.name: i for i, c in enumerate(CASES)}
_PLAIN = {}


def _log(line):
    print(line)
    U.parity_log("autograd_seam " + line)


# ---- building the inputs --------------------------------------------------------------------------------------------------------
def _contiguous(t):
    return t.clone().to(DEV), None


def _view(t):
    """A non-contiguous view holding t's values and the larger, sentinel-filled buffer it lives in: the last two dims transposed AND
    every second row of a buffer twice as tall (no stride of the view is 1, half of the buffer lies outside it); a vector as a column
    of a matrix; a scalar as an element of a vector (a scalar has no strides to break)."""
    if t.dim() >= 2:
        rows, cols = t.shape[-2:]
        buf = torch.full((*t.shape[:-2], cols, 2 * rows), -777.25, device=DEV)
        buf[..., ::2] = t.transpose(-1, -2).to(DEV)
        return buf[..., ::2].transpose(-1, -2), buf
    if t.dim() == 1:
        buf = torch.full((t.numel(), 3), -777.25, device=DEV)
        buf[:, 1] = t.to(DEV)
        return buf[:, 1], buf
    buf = torch.full((3,), -777.25, device=DEV)
    buf[1] = t.to(DEV)
    return buf[1], buf


def _offset(t):
    buf = torch.full((t.numel() + 1,), -777.25, device=DEV)
    buf[1:] = t.reshape(-1).to(DEV)
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v, buf


def _uncopyable(case):
    """The inputs a Function must be handed as they are (it updates them in place, or the caller's parameters are views of them);
    the read-only projection is `fixed` only in that nothing differentiates through it: it is copied like any other operand."""
    return [n for n in case.fixed if n != "proj"]


def _inputs(case, how=_contiguous, frozen=(), fixed=None):
    ts, bufs = [], []
    for name, t, diff in case.tensors:
        v, buf = (_contiguous if name in (case.fixed if fixed is None else fixed) else how)(t)
        v = v.detach()
        if diff and name not in frozen:
            v.requires_grad_()
        ts.append(v)
        bufs.append(buf if buf is not None else v)
    return ts, bufs


def _upstream(case, outs, kind):
    if kind == "ones":
        return [torch.ones((), device=DEV).expand(o.shape) for o in outs]
    ups = AC.upstream(case, outs)
    return [_view(u)[0] for u in ups] if kind == "views" else [u.to(DEV) for u in ups]


def _run(case, ts, up="w", backwards=1):
    """-> (outputs, {input name: .grad or None}) after `backwards` backward passes over one graph."""
    from mlhot import ops
    outs = case.call(ops, ts)
    ups = _upstream(case, outs, up)
    live = [k for k in range(len(outs)) if k not in case.nondiff and outs[k].requires_grad]
    for n in range(backwards if live else 0):
        torch.autograd.backward([outs[k] for k in live], [ups[k] for k in live], retain_graph=n + 1 < backwards)
    torch.cuda.synchronize()
    return [o.detach() for o in outs], {name: t.grad for (name, _, _), t in zip(case.tensors, ts)}


def _plain(gpulib, case, up="w"):
    """The plain run of a case, once per upstream kind; with the launch labels of its forward + backward."""
    key = (case.name, up)
    if key not in _PLAIN:
        ts, _ = _inputs(case)
        labels, (outs, grads) = U.launch_labels(gpulib, lambda: _run(case, ts, up))
        _PLAIN[key] = (outs, grads, labels)
    return _PLAIN[key]


def _same(case, what, outs, grads, want_outs, want_grads, skip=()):
    for k, (a, b) in enumerate(zip(outs, want_outs)):
        assert bits_equal(a, b), f"{case.name} {what}: output {k} differs from the plain run"
    for (name, t, diff) in case.tensors:
        if name in skip or not diff:
            continue
        assert grads[name] is not None and tuple(grads[name].shape) == tuple(t.shape), f"{case.name} {what}: d{name} has shape {None if grads[name] is None else tuple(grads[name].shape)}"
        assert bits_equal(grads[name], want_grads[name]), f"{case.name} {what}: d{name} differs from the plain run"


def _judge(case, what, outs, grads):
    ref = AC.reference(INDEX[case.name])
    if ref is None:
        return
    want_outs, want_grads = ref
    parts, bad = [], []
    quantities = [(f"out{k}", o, want_outs[k]) for k, o in enumerate(outs)] + [("d" + n, grads[n], want_grads[n]) for n, _, d in case.tensors if d]
    for q, got, want in quantities:
        assert got is not None and tuple(got.shape) == tuple(want.shape), f"{case.name} {what}: {q} has shape {None if got is None else tuple(got.shape)}, want {tuple(want.shape)}"
        assert bool(torch.isfinite(got).all()), f"{case.name} {what}: {q} is not finite"
        err, bound = AC.judge_of(INDEX[case.name], q)(got.cpu(), want)
        parts.append(f"{q}={err:.2e}/{bound:.2e}")
        if not err <= bound:
            bad.append(f"{q}: {err:.3e} > {bound:.3e}")
    _log(f"{case.name} {what}: " + " ".join(parts))
    assert not bad, f"{case.name} {what}: " + "; ".join(bad)


# ---- the variants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plain_against_float64(gpulib, case):
    outs, grads, _ = _plain(gpulib, case)
    for name, t, diff in case.tensors:
        assert (grads[name] is not None) == diff, f"{case.name}: d{name}"
        if diff:
            assert tuple(grads[name].shape) == tuple(t.shape), (case.name, name)
    _judge(case, "plain", outs, grads)
    if case.ref is None:
        _log(f"{case.name} plain: no float64 leg (held by the parity tests)")


@pytest.mark.parametrize("up", ["views", "ones"], ids=["upstream_transposed", "upstream_expanded"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_views_are_bit_equal_to_plain_and_leave_their_buffers_alone(gpulib, case, up):
    want_outs, want_grads, _ = _plain(gpulib, case, "w" if up == "views" else "ones")
    ts, bufs = _inputs(case, _view, fixed=_uncopyable(case))
    assert all(not t.is_contiguous() or name in _uncopyable(case) or t.numel() <= 1 or (t.dim() >= 2 and min(t.shape[-2:]) == 1)
               for (name, _, _), t in zip(case.tensors, ts)), case.name
    before = [b.clone() for b in bufs]
    outs, grads = _run(case, ts, up)
    _same(case, f"views/{up}", outs, grads, want_outs, want_grads)
    for (name, _, _), b, b0 in zip(case.tensors, bufs, before):
        if name not in case.mutable:
            assert bits_equal(b, b0), f"{case.name} views/{up}: the buffer of {name} changed"
    _log(f"{case.name} views/{up}: bit-equal")


@pytest.mark.parametrize("case", [c for c in CASES if c.offset], ids=[c.name for c in CASES if c.offset])
def test_offset_operands_against_float64(gpulib, case):
    ts, bufs = _inputs(case, _offset)
    before = [b.clone() for b in bufs]
    outs, grads = _run(case, ts)
    _judge(case, "offset", outs, grads)
    assert all(bits_equal(b, b0) for b, b0 in zip(bufs, before)), case.name


ALIGNED = [c for c in CASES if not c.offset]


@pytest.mark.parametrize("case", ALIGNED, ids=[c.name for c in ALIGNED])
def test_offset_operands_never_reach_an_entry_that_demands_alignment(gpulib, case):
    """The entries behind these Functions demand 16-byte aligned pointers (include/mlhot.h).  An operand one float into its buffer
    is copied on the way in - the kernels see aligned storage holding the same bytes, so everything is bit-equal to plain, with
    plain's launches - and an operand that cannot be copied (a buffer updated in place, a stacked weight the heads are views of) is
    refused with MlhotError before anything is launched.  Either way no kernel runs on a misaligned pointer."""
    from mlhot.binding import MlhotError
    want_outs, want_grads, plain_labels = _plain(gpulib, case)
    refused = _uncopyable(case)
    ts, bufs = _inputs(case, _offset, fixed=refused)
    assert all(t.data_ptr() % 16 == 4 for (name, _, _), t in zip(case.tensors, ts) if name not in refused)
    before = [b.clone() for b in bufs]
    labels, (outs, grads) = U.launch_labels(gpulib, lambda: _run(case, ts))
    _same(case, "offset", outs, grads, want_outs, want_grads)
    assert labels == plain_labels, f"{case.name} offset: launches {plain_labels} -> {labels}"
    for (name, _, _), b, b0 in zip(case.tensors, bufs, before):
        if name not in case.mutable:
            assert bits_equal(b, b0), f"{case.name} offset: the buffer of {name} changed"
    for name in refused:
        ts, _ = _inputs(case)
        k = [n for n, _, _ in case.tensors].index(name)
        ts[k] = _offset(case.tensors[k][1])[0]
        gpulib.prof_begin(256)
        try:
            with pytest.raises(MlhotError):
                _run(case, ts)
        finally:
            recorded = gpulib.prof_end()
        assert not recorded, f"{case.name}: {name} one float into its buffer was refused after launching {recorded}"
    _log(f"{case.name} offset: operands copied to aligned storage, bit-equal to plain with plain's launches"
         + (f"; {', '.join(refused)} refused before any launch" if refused else ""))


def _frozen_pairs():
    return [pytest.param(c, n, id=f"{c.name}-{n}") for c in CASES if c.ref is not None for n, _, d in c.tensors if d]


@pytest.mark.parametrize("case,name", _frozen_pairs())
def test_a_frozen_input_gets_no_gradient_and_changes_no_other(gpulib, case, name):
    want_outs, want_grads, plain_labels = _plain(gpulib, case)
    ts, _ = _inputs(case, frozen=(name,))
    labels, (outs, grads) = U.launch_labels(gpulib, lambda: _run(case, ts))
    assert grads[name] is None, f"{case.name}: the frozen {name} has a gradient"
    _same(case, f"frozen {name}", outs, grads, want_outs, want_grads, skip=(name,))
    if not any(t.requires_grad for t in ts):
        assert not any(o.requires_grad for o in outs)
        _log(f"{case.name} frozen {name}: its only differentiable input - the output carries no graph, outputs bit-equal")
    elif name in case.flags:
        assert labels != plain_labels, f"{case.name}: freezing {name} (a need_* flag of the binding) launches what the plain run launches: {labels}"
        _log(f"{case.name} frozen {name}: bit-equal; need flag: launches {plain_labels} -> {labels}")
    else:
        assert labels == plain_labels, f"{case.name}: freezing {name} changed the launches {plain_labels} -> {labels}"
        why = "need flag inside a one-launch job" if name in case.job_flags else "no need flag"
        _log(f"{case.name} frozen {name}: bit-equal; {why}: launches unchanged ({len(labels)})")


HEAVY = [c for c in CASES if c.ref is None]


@pytest.mark.parametrize("case", HEAVY, ids=[c.name for c in HEAVY])
def test_whole_model_functions_with_each_input_frozen_in_turn(gpulib, case):
    want_outs, want_grads, plain_labels = _plain(gpulib, case)
    for name, _, diff in case.tensors:
        if not diff:
            continue
        ts, _ = _inputs(case, frozen=(name,))
        labels, (outs, grads) = U.launch_labels(gpulib, lambda: _run(case, ts))
        assert grads[name] is None, f"{case.name}: the frozen {name} has a gradient"
        _same(case, f"frozen {name}", outs, grads, want_outs, want_grads, skip=(name,))
        assert labels == plain_labels, f"{case.name}: freezing {name} changed the launches"
    _log(f"{case.name} frozen, each of {sum(d for _, _, d in case.tensors)} inputs in turn: bit-equal; no need flag: launches unchanged ({len(plain_labels)})")


MULTI = [c for c in CASES if sum(d for _, _, d in c.tensors) > 1]


@pytest.mark.parametrize("case", MULTI, ids=[c.name for c in MULTI])
def test_all_inputs_frozen_but_one(gpulib, case):
    want_outs, want_grads, _ = _plain(gpulib, case)
    diff = [n for n, _, d in case.tensors if d]
    picks = diff if case.ref is not None else [diff[0], diff[len(diff) // 2], diff[-1]]
    for keep in picks:
        ts, _ = _inputs(case, frozen=tuple(n for n in diff if n != keep))
        outs, grads = _run(case, ts)
        assert all(grads[n] is None for n in diff if n != keep), (case.name, keep)
        _same(case, f"only {keep} live", outs, grads, want_outs, want_grads, skip=tuple(n for n in diff if n != keep))
    _log(f"{case.name} one_live ({len(picks)} inputs in turn): bit-equal")


def test_unused_outputs_reach_the_backward_as_none(gpulib):
    """BBBSampleMultiFunction with one sample unused (its dw arrives as None) and the trunk with one pass's output unused (dfeat None):
    the gradients of what IS used equal the float64 reference's / the plain run's."""
    from mlhot import ops
    case = CASES[INDEX["bbb_sample_multi_7_5x3"]]
    ts, _ = _inputs(case)
    w0, w1, kl = case.call(ops, ts)
    up = AC.upstream(case, [w0, w1, kl])
    torch.autograd.backward([w0, kl], [up[0].to(DEV), up[2].to(DEV)])
    t64 = [v.double().clone().requires_grad_(d) for _, v, d in case.tensors]
    r0, r1, rkl = case.ref(t64)
    torch.autograd.backward([r0, rkl], [up[0].double(), up[2].double()])
    for k, (n, _, d) in enumerate(case.tensors):
        if d:
            err, bound = AC.judge_of(INDEX[case.name], "d" + n)(ts[k].grad.cpu(), t64[k].grad)
            _log(f"{case.name} w1 unused: d{n}={err:.2e}/{bound:.2e}")
            assert err <= bound, (n, err)
    case = CASES[INDEX["resnet_trunk_C3_H64_skip1_skip3"]]
    _, want_grads, _ = _plain(gpulib, case)
    ts, _ = _inputs(case)
    outs = case.call(ops, ts)
    up = AC.upstream(case, outs)
    outs[0].backward(up[0].to(DEV))
    for k, (n, _, d) in enumerate(case.tensors):
        if d and n.startswith("ws0."):
            assert bits_equal(ts[k].grad, want_grads[n]), n
        elif d:
            assert ts[k].grad is not None and int(torch.count_nonzero(ts[k].grad)) == 0, f"{n}: the unused pass's weights get zeros"
    _log(f"{case.name} pass 1 unused (dfeat None): pass 0's gradients bit-equal to plain, pass 1's all zero")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_second_backward_on_the_same_graph_adds_the_same_gradients(gpulib, case):
    _, want_grads, _ = _plain(gpulib, case)
    ts, _ = _inputs(case)
    _, grads = _run(case, ts, backwards=2)
    for name, _, diff in case.tensors:
        if diff:
            assert bits_equal(grads[name], want_grads[name] + want_grads[name]), f"{case.name} twice: d{name} is not plain + plain"
    _log(f"{case.name} twice: bit-equal to plain + plain")


@pytest.mark.parametrize("deferred", [False, True], ids=["loss_gradient_from_the_loss", "loss_gradient_in_the_models_backward"])
@pytest.mark.parametrize("agg", ["attention", "max"])
def test_loss_on_the_vanilla_model_backward_twice(gpulib, agg, deferred):
    """LossFunction -> VanillaNPFunction under loss_grad_in_backward on and off: two backwards over one graph give twice the gradients
    of one (ctx.scratch and ctx.loss are given up by the first), nothing raises, and both settings agree bit for bit."""
    from mlhot import ops
    case = next(c for c in CASES if c.name.startswith(f"vanilla_np_{agg}"))
    gt = torch.rand(1, 1, 3, generator=torch.Generator().manual_seed(3)).to(DEV)

    def run(backwards, on):
        ts, _ = _inputs(case)
        with ops.loss_grad_in_backward(on):
            loss = ops.LossFunction.apply("azimuth", case.call(ops, ts)[0], gt)
            for n in range(backwards):
                loss.backward(retain_graph=n + 1 < backwards)
        torch.cuda.synchronize()
        return loss.detach(), [t.grad for t in ts]
    l1, g1 = run(1, False)
    l2, g2 = run(2, deferred)
    assert bits_equal(l1, l2)
    for (name, _, diff), a, b in zip(case.tensors, g1, g2):
        if diff:
            assert bits_equal(b, a + a), f"{case.name} deferred={deferred}: d{name} after two backwards is not twice one backward's"
    _log(f"{case.name} loss twice, deferred={deferred}: bit-equal to plain + plain")


# ---- shared leaves --------------------------------------------------------------------------------------------------------------
def test_shared_weight_under_two_linears(gpulib):
    from mlhot.ops import LinearFunction
    case = CASES[INDEX["linear_7x20x12_tanh"]]
    (x, w, b), _ = _inputs(case)
    x2 = torch.randn(3, 20, generator=torch.Generator().manual_seed(5))
    x2d = x2.to(DEV).requires_grad_()
    (LinearFunction.apply(x, w, b, "tanh").sum() + LinearFunction.apply(x2d, w, b, "none").pow(2).sum()).backward()
    t = [v.double().clone().requires_grad_() for _, v, _ in case.tensors] + [x2.double().requires_grad_()]
    (torch.tanh(F.linear(t[0], t[1], t[2])).sum() + F.linear(t[3], t[1], t[2]).pow(2).sum()).backward()
    errs = {n: U.rel_err(a.grad, r.grad) for n, a, r in zip(("x", "w", "b", "x2"), (x, w, b, x2d), t)}
    _log("linear shared w, b under two nodes: " + " ".join(f"d{n}={e:.2e}/{U.RTOL:.0e}" for n, e in errs.items()))
    assert max(errs.values()) <= U.RTOL, errs


def test_add_relu_of_a_tensor_with_itself_and_its_two_gradients(gpulib):
    from mlhot.ops import AddReluFunction
    case = CASES[INDEX["add_relu_5x7"]]
    (a, b), _ = _inputs(case)
    up = AC.upstream(case, [a])[0]
    AddReluFunction.apply(a, a).backward(up.to(DEV))
    a64 = case.tensors[0][1].double().requires_grad_()
    torch.relu(a64 + a64).backward(up.double())
    assert U.rel_err(a.grad, a64.grad) <= U.RTOL
    a.grad = None
    AddReluFunction.apply(a, b).backward(up.to(DEV))
    assert bits_equal(a.grad, b.grad)
    assert a.grad.untyped_storage().data_ptr() != b.grad.untyped_storage().data_ptr(), "a.grad and b.grad share their storage"
    kept = b.grad.clone()
    a.grad.add_(1)
    assert bits_equal(b.grad, kept), "an in-place update of a.grad reached b.grad"
    _log("add_relu shared: apply(a, a) at RTOL of float64; a.grad and b.grad of apply(a, b) own their storage")


def test_favor_with_one_tensor_as_key_and_value(gpulib):
    """k.grad = dk + dv: held against the float64 dk + dv with each share at its own family bound of its own scale,
    |error| <= bound_dk max|dk| + bound_dv max|dv| (no bound of its own)."""
    from mlhot.ops import FavorFunction
    name = "T1_H2_Nq16_Nc16_d32_m110"
    case = CASES[INDEX["favor_" + name]]
    (q, k, _, proj), _ = _inputs(case)
    out = FavorFunction.apply(q, k, k, proj)
    up = AC.upstream(case, [out])[0]
    out.backward(up.to(DEV))
    t = [v.double().clone().requires_grad_(d) for _, v, d in case.tensors]
    t[2] = t[1].detach().clone().requires_grad_()               # the same values as a leaf of its own: dk and dv apart
    out64 = case.ref(t)[0]
    out64.backward(up.double())
    bound = AC.FC.bounds(AC.FC.BY_NAME[name])
    dk, dv = t[1].grad, t[2].grad
    share = bound["dk"] * dk.abs().max().item() + bound["dv"] * dv.abs().max().item()
    errs = {"out": (U.rel_err(out, out64), bound["out"]), "dq": (U.rel_err(q.grad, t[0].grad), bound["dq"]),
            "dk+dv (absolute)": ((k.grad.double().cpu() - (dk + dv)).abs().max().item(), share)}
    _log("favor shared k is v: " + " ".join(f"{n}={e:.2e}/{b:.2e}" for n, (e, b) in errs.items()))
    assert all(e <= b for e, b in errs.values()), errs


# ---- the gradient arena on the device -------------------------------------------------------------------------------------------
def _linear_situation(situation, with_arena):
    from mlhot import binding
    from mlhot.arena import GradArena
    from mlhot.ops import LinearFunction
    case = CASES[INDEX["linear_7x20x12_tanh"]]
    (x, w, b), _ = _inputs(case)
    xs = [x.detach(), (x.detach() * 0.5 + 0.25)]
    arena = GradArena([w, b]).refresh() if with_arena else None
    binding.set_grad_arena(arena)
    try:
        def backward(k, consumers=1):
            sum(LinearFunction.apply(xs[(k + c) % 2], w, b, "tanh").pow(2).sum() for c in range(consumers)).backward()
        if situation == "zeroed_in_place":
            backward(0)
            w.grad.zero_(), b.grad.zero_()
            backward(1)
        elif situation == "two_backwards":
            backward(0), backward(1)
        elif situation == "two_consumers":
            backward(0, consumers=2)
        else:
            for k in range(3):
                w.grad = b.grad = None
                backward(k)
                if arena is not None:
                    assert w.grad.data_ptr() == arena.slot(w).data_ptr() and b.grad.data_ptr() == arena.slot(b).data_ptr(), "shipped: a gradient left its slot"
        torch.cuda.synchronize()
    finally:
        binding.set_grad_arena(None)
    return w.grad.clone(), b.grad.clone()


@pytest.mark.parametrize("situation", ["zeroed_in_place", "two_backwards", "two_consumers", "shipped"])
def test_linear_gradients_with_an_arena_equal_gradients_without(gpulib, situation):
    plain, got = _linear_situation(situation, False), _linear_situation(situation, True)
    assert bits_equal(got[0], plain[0]) and bits_equal(got[1], plain[1]), f"{situation}: the arena changes the gradients"
    _log(f"arena LinearFunction {situation}: bit-equal to the run without an arena")


@pytest.mark.parametrize("situation", ["zeroed_in_place", "two_backwards"])
def test_model_gradients_with_an_arena_equal_gradients_without(gpulib, situation):
    """CondNeuralProcess at T 2, Nc 5, Nq 6 (test_flat_gradient_arena_for_the_resnet_family's configuration): zero_grad(set_to_none=False)
    between two steps, and two backwards accumulated, with enable_flat_grads() against the same run without."""
    import types
    from mlhot import binding
    from networks.CondNeuralProcess import CondNeuralProcess
    from trainer.losses import LossFunc
    T, Nc, Nq = 2, 5, 6
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=T, input_dim=4, output_dim=4, agg_mode="max",
                                img_agg="max", task="shapenet_3d", temperature=0.07)
    g = torch.Generator().manual_seed(7)
    batches = []
    for _ in range(2):
        cx, qx = torch.rand(T, Nc, 3, 64, 64, generator=g).to(DEV), torch.rand(T, Nq, 3, 64, 64, generator=g).to(DEV)
        cy = F.normalize(torch.randn(T, Nc, 4, generator=g), dim=-1).to(DEV)
        batches.append((cx, cy, qx, F.normalize(torch.randn(T, Nq, 4, generator=g), dim=-1).to(DEV)))

    def run(with_arena):
        model = CondNeuralProcess(cfg).to(DEV)
        try:
            if with_arena:
                model.enable_flat_grads()
            for k, (cx, cy, qx, qy) in enumerate(batches):
                if k and situation == "zeroed_in_place":
                    model.zero_grad(set_to_none=False)
                torch.manual_seed(99)
                mu, var, kl = model(cx, cy, qx)
                (LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy) + 1e-7 * kl).backward()
            torch.cuda.synchronize()
            return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
        finally:
            binding.set_grad_arena(None)
    plain, got = run(False), run(True)
    assert plain.keys() == got.keys() and sum(v is not None for v in plain.values()) > 20
    for k, v in plain.items():
        assert (v is None) == (got[k] is None), k
        if v is not None:
            assert bits_equal(got[k], v), f"{situation}: {k} differs with the arena"
    _log(f"arena CondNeuralProcess {situation}: every gradient bit-equal to the run without an arena")


@pytest.mark.parametrize("situation", ["shipped", "zeroed_in_place", "two_backwards"])
@pytest.mark.parametrize("method", ["FCLANP", "FCLCNPDistractor"])
def test_contrastive_model_gradients_with_an_arena_equal_gradients_without(gpulib, method, situation):
    """The two plugin classes that inherit enable_flat_grads() and whose forward takes the target labels and returns the NT-Xent term
    as a fourth value (so test_flat_gradient_arena_for_the_resnet_family's body does not fit them), at its T 2, Nc 5, Nq 6: the
    gradients of loss + term with the arena equal those without, and in the shipped pattern every gradient with one consumer sits in
    arena.flat."""
    import importlib
    import types
    from mlhot import binding
    from trainer.losses import LossFunc
    T, Nc, Nq = 2, 5, 6
    cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[64, 64, 4], tasks_per_batch=T, input_dim=4, output_dim=4,
                                agg_mode="attention" if method == "FCLANP" else "max", img_agg="max", task="shapenet_3d", temperature=0.07, dim_w=64)
    g = torch.Generator().manual_seed(7)
    batches = []
    for _ in range(2):
        cx, qx = torch.rand(T, Nc, 3, 64, 64, generator=g).to(DEV), torch.rand(T, Nq, 3, 64, 64, generator=g).to(DEV)
        cy = F.normalize(torch.randn(T, Nc, 4, generator=g), dim=-1).to(DEV)
        batches.append((cx, cy, qx, F.normalize(torch.randn(T, Nq, 4, generator=g), dim=-1).to(DEV)))

    def run(with_arena):
        model = getattr(importlib.import_module("networks." + method), method)(cfg).to(DEV)
        try:
            arena = model.enable_flat_grads() if with_arena else None
            for k, (cx, cy, qx, qy) in enumerate(batches):
                if situation == "shipped":
                    model.zero_grad(set_to_none=True)
                elif k and situation == "zeroed_in_place":
                    model.zero_grad(set_to_none=False)
                mu, var, kl, contra = model(cx, cy, qx, qy)
                (LossFunc("mse", "shapenet_3d").calc_loss(mu, var, qy) + contra).backward()
            torch.cuda.synchronize()
            if arena is not None and situation == "shipped":
                base = arena.flat.untyped_storage().data_ptr()
                outside = [k for k, p in model.named_parameters() if p.grad is not None and p.grad.untyped_storage().data_ptr() != base]
                # FCLCNPDistractor's contrastive term runs the label transform, the task encoder and the `mu` layer on the targets
                # as well (networks/_resnet_np.py, contra_cnp): those parameters have two consumers in one backward, the second
                # kernel writes a fresh tensor and autograd's sum is a tensor of its own (GradBucket then packs).  Everything
                # with one consumer stays in the buffer.
                twice = ("transform_y.", "task_encoder.", "mu.") if method == "FCLCNPDistractor" else ()
                assert all(k.startswith(twice) for k in outside) if twice else not outside, f"{method}: gradients outside the flat buffer: {outside}"
                assert sum(p.grad is not None for p in model.parameters()) - len(outside) > 20
            return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
        finally:
            binding.set_grad_arena(None)
    plain, got = run(False), run(True)
    assert plain.keys() == got.keys() and sum(v is not None for v in plain.values()) > 20
    for k, v in plain.items():
        assert (v is None) == (got[k] is None), k
        if v is not None:
            assert bits_equal(got[k], v), f"{method} {situation}: {k} differs with the arena"
    _log(f"arena {method} {situation}: every gradient bit-equal to the run without an arena" + (", every single-consumer gradient inside arena.flat" if situation == "shipped" else ""))
