"""mlhot.optim.FlatAdam's HOST logic against a plain float64 Adam - shared by tests/test_flat_adam_cpu.py (the host build of the two
Adam entries, CPU tensors) and tests/test_flat_adam_gpu.py (the device).  The two kernels have tests of their own (tests/glue_ops.py,
tests/test_hostsim.py); here it is what FlatAdam wraps round them: which gradient tensor the launch reads (the library's buffer, a
mirror arena, the gathered copy), the parameters without a gradient it restores, the parked tail, weight decay and the gradient scale
through step(), hyper-parameters written between steps, and every way a checkpoint comes in or goes out.

The stand-in module (StandIn) has no forward and no images: parameters of 1, 3, 5, 16, 257 and 64 x 33 floats, every slice 16-byte
aligned (so there is padding between them), in the two shapes `flat_layout()` comes in - `(total, offs)` without and
`(total, offs, active)` with a "dead" parameter that never has a gradient, parked at `active`.

The reference (adam_ref64): float64, g = scale * grad + wd * p, ONE global step count, and a parameter without a gradient is left as it
is - no moment decay, no weight decay, no move - while the count still advances for it.  That last point is the documented difference
from torch.optim.Adam, which counts per parameter (mlhot/optim.py, FlatAdam._flat_grad): after a skipped step the bias correction of
that parameter runs one step ahead of torch's.  It is pinned here as FlatAdam's behaviour.  Where no step is skipped adam_ref64 is
itself checked against torch.optim.Adam on float64 copies (inside e32(), to 1e-12).

The metric is the MOVEMENT: per step, for dp = p_after - p_before, exp_avg and exp_avg_sq, max |got - ref64| / max |ref64 quantity|
over all live parameters.  (On the parameter itself, of order 1, an update of order lr that is wrong by percents passes 1e-5.)

The bound is measured, not chosen: fp32 torch.optim.Adam (CPU, foreach=False - an fp32 Adam nobody here wrote) runs the same
gradients and hyper-parameters with every gradient present, its error against adam_ref64 is `e32` per quantity, and FlatAdam may reach
MARGIN = 4 x e32.  The 4 is a margin for multiplying by a reciprocal where torch divides and for fused multiply-adds; it is not
derived.  Rows that withhold a gradient use the e32 of the same row with nothing withheld (torch's per-parameter count makes its own
skipped trajectory a different function).  profiles/INDEX_flat_adam.md holds e32 and what FlatAdam measured."""
import functools
import io
import math
import types

import pytest
import torch

from mlhot.arena import GradArena
from mlhot.optim import FlatAdam

SHAPES = (("s1", (1,)), ("s3", (3,)), ("s5", (5,)), ("s16", (16,)), ("s257", (257,)), ("w", (64, 33)))
DEAD = ("dead", (7,))
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
STEPS, MARGIN = 5, 4.0
QUANTITIES = ("dp", "exp_avg", "exp_avg_sq")
OTHER = dict(lr=0.37, betas=(0.3, 0.4), eps=0.25, weight_decay=0.125)      # constructor values a loaded checkpoint must replace


class StandIn(torch.nn.Module):
    """form "two": flat_layout() -> (total, offs); "three": -> (total, offs, active) with `dead` parked at `active`.  lead: unused
    floats in front of the first slice (a layout need not start at 0)."""

    def __init__(self, form="three", lead=0, seed=11):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for k, s in SHAPES + ((DEAD,) if form == "three" else ()):
            setattr(self, k, torch.nn.Parameter(torch.rand(*s, generator=g) * 2 - 1))          # U[-1, 1]
        self.form, self.lead = form, lead

    def flat_layout(self, *_):
        offs, at = {}, self.lead
        for k, p in self.named_parameters():
            if k != "dead":
                offs[k], at = at, at + (p.numel() + 3) // 4 * 4
        if self.form == "two":
            return at, offs
        offs["dead"] = at
        return at + 8, offs, at


def row(name, form="three", mode="mirrored", lead=0, wd=0.0, scale=1.0, eps=EPS, betas=BETAS, lr=LR, skip=None, writes=None):
    """One line of the table.  mode: where step() finds the gradients (see _place).  skip: (parameter, steps on which its .grad is
    None).  writes: {step: {key: value}} written to param_groups[0] before that step."""
    return types.SimpleNamespace(name=name, form=form, mode=mode, lead=lead, wd=wd, scale=scale, eps=eps, betas=betas, lr=lr,
                                 skip=skip or (None, ()), writes=writes or {})


SKIP = ("s257", (2, 4))
PLAIN = [row(f"plain-{form}-wd{wd}-scale{scale}", form=form, mode=mode, wd=wd, scale=scale)
         for form, mode in (("two", "flat"), ("three", "mirrored")) for wd in (0.0, 0.01) for scale in (1.0, 0.5)] + \
        [row("plain-eps1e-3", eps=1e-3), row("plain-betas0.5-0.9", betas=(0.5, 0.9), wd=0.01)]
# (without a mirror a parked parameter's missing gradient alone sends step() to the gathered copy: the rows that are about ONE reason
# for the fallback, or about the fast path next to it, use the two-tuple layout, which has no parked parameter)
SKIPS = [row(f"skip_{mode}-wd{wd}", form=form, mode=m, wd=wd, skip=SKIP)
         for mode, m, form in (("separate", "separate", "three"), ("mirrored", "mirrored", "three"), ("flat_unmirrored", "flat", "two"))
         for wd in (0.0, 0.01)]
GATHER = [row("other_layout", form="two", mode="other_layout", wd=0.01), row("non_contiguous", form="two", mode="non_contiguous", wd=0.01, scale=0.5),
          row("short_storage", mode="short_storage", wd=0.01), row("negative_base", form="two", mode="negative_base", lead=4, scale=0.5),
          row("separate", form="two", mode="separate"), row("separate_parked", mode="separate", wd=0.01)]
LR_WRITTEN = row("lr_written", wd=0.01, writes={3: {"lr": 3e-3}, 4: {"betas": (0.8, 0.99)}})
PARKED = row("parked", wd=0.01)
BASE = row("base", wd=0.01, scale=0.5)          # what the resume / refusal cases run on


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gradients(total, steps=STEPS, seed=5):
    """`steps` flat fp32 gradient vectors: |g| log-uniform in [1e-3, 1], random sign, and every 7th entry exactly 0 on EVERY step
    (so its moments stay exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        mag = torch.exp(torch.rand(total, generator=g, dtype=torch.float64) * math.log(1e-3)).float()
        v = mag * (torch.randint(0, 2, (total,), generator=g) * 2 - 1).float()
        v[::7] = 0.0
        out.append(v)
    return out


def hypers(r, steps=STEPS):
    """The hyper-parameters in force on each step of row `r`."""
    cur, out = dict(lr=r.lr, betas=r.betas, eps=r.eps, wd=r.wd, scale=r.scale), []
    for t in range(1, steps + 1):
        cur = {**cur, **r.writes.get(t, {})}
        out.append(cur)
    return out


def spans_of(model):
    total, offs, *rest = model.flat_layout()
    named = dict(model.named_parameters())
    return total, {k: (offs[k], named[k].numel()) for k in offs}, (rest[0] if rest else total)


def live_index(spans):
    return torch.cat([torch.arange(a, a + n) for k, (a, n) in spans.items() if k != "dead"])


def present(r, spans, t):
    return [k for k in spans if k != "dead" and not (k == r.skip[0] and t in r.skip[1])]


# ---- references ----------------------------------------------------------------------------------------------------------------
def adam_ref64(p, spans, grads, names, hyp, m=None, v=None, t0=0):
    """Plain float64 Adam over flat vectors.  grads[i]: flat gradient of step i+1, names[i]: the parameters that have one, hyp[i]: its
    hyper-parameters.  A parameter without a gradient is untouched; a step on which nobody has one does not count.  The bias
    corrections use the ONE global count (see the module docstring).  Returns [(p, m, v)] after every step and the count."""
    p = p.double().clone()
    m = torch.zeros_like(p) if m is None else m.double().clone()
    v = torch.zeros_like(p) if v is None else v.double().clone()
    t, out = t0, []
    for g, ks, h in zip(grads, names, hyp):
        if ks:
            t += 1
            b1, b2 = h["betas"]
            for k in ks:
                sl = slice(spans[k][0], spans[k][0] + spans[k][1])
                gi = h["scale"] * g[sl].double() + h["wd"] * p[sl]
                m[sl] = b1 * m[sl] + (1 - b1) * gi
                v[sl] = b2 * v[sl] + (1 - b2) * gi * gi
                p[sl] = p[sl] - (h["lr"] / (1 - b1 ** t)) * m[sl] / (v[sl].sqrt() / math.sqrt(1 - b2 ** t) + h["eps"])
        out.append((p.clone(), m.clone(), v.clone()))
    return out, t


def torch_adam(p, spans, grads, hyp, dtype):
    """torch.optim.Adam (CPU, foreach=False, one tensor per parameter, every gradient present) in `dtype`; [(p, m, v)] as flat float64
    vectors after every step."""
    ps = {k: torch.nn.Parameter(p[a:a + n].to(dtype).clone()) for k, (a, n) in spans.items() if k != "dead"}
    opt = torch.optim.Adam(ps.values(), lr=hyp[0]["lr"], betas=hyp[0]["betas"], eps=hyp[0]["eps"], weight_decay=hyp[0]["wd"], foreach=False)
    out = []
    for g, h in zip(grads, hyp):
        opt.param_groups[0].update(lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["wd"])
        for k, q in ps.items():
            a, n = spans[k]
            q.grad = (g[a:a + n].to(dtype) * h["scale"]).view_as(q)
        opt.step()
        flat = [p.double().clone(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)]
        for k, q in ps.items():
            a, n = spans[k]
            flat[0][a:a + n], flat[1][a:a + n], flat[2][a:a + n] = q.detach().double(), opt.state[q]["exp_avg"].double(), opt.state[q]["exp_avg_sq"].double()
        out.append(tuple(flat))
    return out


def errors(got, ref, p0, idx, first=0):
    """{quantity: max over steps >= first of max |got - ref| / max |ref|} on the live entries `idx`; dp is each step's movement."""
    err = dict.fromkeys(QUANTITIES, 0.0)
    for i in range(first, len(ref)):
        gb, rb = (got[i - 1][0] if i else p0.double()), (ref[i - 1][0] if i else p0.double())
        pairs = {"dp": ((got[i][0] - gb)[idx], (ref[i][0] - rb)[idx]), "exp_avg": (got[i][1][idx], ref[i][1][idx]),
                 "exp_avg_sq": (got[i][2][idx], ref[i][2][idx])}
        for q, (a, b) in pairs.items():
            err[q] = max(err[q], ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item())
    return err


def _key(r):
    return (r.form, r.lead, r.lr, r.betas, r.eps, r.wd, r.scale, tuple(sorted((t, tuple(sorted(w.items()))) for t, w in r.writes.items())))


_E32 = {}


def e32(r):
    """fp32 torch.optim.Adam against adam_ref64 on row r's gradients and hyper-parameters, every gradient present: {quantity: error}.
    Also holds the reference honest: float64 torch.optim.Adam must agree with adam_ref64 to rounding on the same run."""
    k = _key(r)
    if k not in _E32:
        model = StandIn(r.form, r.lead)
        total, spans, _ = spans_of(model)
        p0 = flat_of(model, spans, total)
        gs, hyp, idx = gradients(total), hypers(r), live_index(spans)
        ref, _ = adam_ref64(p0, spans, gs, [[n for n in spans if n != "dead"]] * STEPS, hyp)
        honest = errors(torch_adam(p0, spans, gs, hyp, torch.float64), ref, p0, idx)
        assert max(honest.values()) <= 1e-12, ("adam_ref64 and float64 torch.optim.Adam disagree", honest)
        _E32[k] = errors(torch_adam(p0, spans, gs, hyp, torch.float32), ref, p0, idx)
    return _E32[k]


def flat_of(model, spans, total):
    p = torch.zeros(total, dtype=torch.float64)
    for k, q in model.named_parameters():
        p[spans[k][0]:spans[k][0] + spans[k][1]] = q.detach().double().cpu().reshape(-1)
    return p


def within_bound(r, err, what, measured=None):
    """Print e32 and the measured errors (one line, profiles/INDEX_flat_adam.md is filled from these), then assert err <= 4 x e32."""
    ref = e32(r)
    print(f"[flat_adam] {what}: " + "  ".join(f"{q} e32 {ref[q]:.3e} got {err[q]:.3e} ({err[q] / max(ref[q], 1e-300):.2f}x)" for q in QUANTITIES))
    if measured is not None:
        measured.append((what, ref, err))
    for q in QUANTITIES:
        assert err[q] <= MARGIN * ref[q], (what, q, err[q], ref[q])


# ---- running FlatAdam ------------------------------------------------------------------------------------------------------------
def snap(opt):
    return tuple(t.detach().double().cpu().clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq))


def bits(opt):
    return tuple(t.detach().cpu().clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq))


def count(opt):
    return int(opt.step_dev.item()) if opt.capturable else opt.t


def build(r, capturable, device, weights=None, **ctor):
    """(model, optimizer, store) of row r.  weights: a state_dict to start from.  ctor: FlatAdam arguments instead of the row's."""
    model = StandIn(r.form, r.lead)
    if weights is not None:
        model.load_state_dict(weights)
    model = model.to(device)
    kw = dict(lr=r.lr, betas=r.betas, eps=r.eps, weight_decay=r.wd)
    kw.update(ctor)
    opt = FlatAdam(model, capturable=capturable, **kw)
    total, spans, active = spans_of(model)
    store = {}
    if r.mode == "mirrored":
        model._arena = GradArena(model.parameters()).refresh()
        assert model._arena.flat.numel() == total
        store["buf"] = model._arena.flat
    elif r.mode == "short_storage":                 # a mirror of the live parameters only: `active` floats, the parked tail lies behind it
        model._arena = GradArena([p for k, p in model.named_parameters() if k != "dead"]).refresh()
        assert model._arena.flat.numel() == active < total
        store["buf"] = model._arena.flat
    elif r.mode == "negative_base":
        store["buf"] = torch.zeros(total - r.lead, device=device)
    elif r.mode == "other_layout":
        store["buf"] = torch.zeros(total + 64, device=device)
    elif r.mode != "separate":
        store["buf"] = torch.zeros(total, device=device)
    return model, opt, store


def place(r, model, store, g, names):
    """Hand step() the gradients of `names` (values from the flat vector g), the way row r's mode lays them out; everyone else's .grad
    is None.  The buffers live for the whole run and are never zeroed: a withheld parameter's slot keeps its last gradient."""
    total, spans, _ = spans_of(model)
    buf = store.get("buf")
    for i, (k, p) in enumerate(model.named_parameters()):
        if k not in names:
            p.grad = None
            continue
        a, n = spans[k]
        val = g[a:a + n].to(p.device)
        if r.mode == "separate":
            slot = torch.empty_like(p)
        elif r.mode == "other_layout":              # one storage, but every parameter shifted by another amount
            slot = buf[a + 4 * (i + 1):a + 4 * (i + 1) + n].view_as(p)
        elif r.mode == "negative_base":             # one storage, one shift - to the left of the layout
            slot = buf[a - r.lead:a - r.lead + n].view_as(p)
        elif r.mode == "non_contiguous" and p.dim() == 2:      # in its place in the buffer, but transposed
            slot = buf[a:a + n].view(p.shape[1], p.shape[0]).t()
        else:
            slot = buf[a:a + n].view_as(p)
        slot.copy_(val.view_as(p))
        p.grad = slot


def run(r, capturable, device, steps=STEPS, first=1, built=None, each=None):
    """Steps first..steps of row r.  Returns (model, opt, [snap after each step], p0 flat).  each(t, model, opt, before_bits): called
    after every step."""
    model, opt, store = built or build(r, capturable, device)
    total, spans, _ = spans_of(model)
    gs, p0, out = gradients(total), snap(opt)[0], []
    for t in range(first, steps + 1):
        if t in r.writes:
            opt.param_groups[0].update(r.writes[t])
        place(r, model, store, gs[t - 1], present(r, spans, t))
        before = bits(opt)
        opt.step(grad_scale=r.scale)
        out.append(snap(opt))
        if each is not None:
            each(t, model, opt, before)
    return model, opt, out, p0


def reference(r, model, p0, steps=STEPS):
    total, spans, _ = spans_of(model)
    return adam_ref64(p0, spans, gradients(total)[:steps], [present(r, spans, t) for t in range(1, steps + 1)], hypers(r)[:steps])[0]


def follows_ref(r, capturable, device, measured=None, each=None):
    model, opt, got, p0 = run(r, capturable, device, each=each)
    total, spans, _ = spans_of(model)
    err = errors(got, reference(r, model, p0), p0, live_index(spans))
    within_bound(r, err, f"{r.name} capturable={capturable}", measured)
    assert count(opt) == STEPS
    return model, opt, got, p0


def same_bits(a, b, spans, k=None):
    sl = slice(None) if k is None else slice(spans[k][0], spans[k][0] + spans[k][1])
    return all(torch.equal(x[sl], y[sl]) for x, y in zip(a, b))


# ---- the cases: each takes (capturable, device, measured) --------------------------------------------------------------------------
def case_plain(r, capturable, device, measured=None):
    model, opt, got, p0 = follows_ref(r, capturable, device, measured)
    assert opt._gather is None                      # the launch read the gradients where they lay
    total, spans, _ = spans_of(model)
    if r.wd == 0:                                   # grad, m and v exactly 0, no decay: the parameter does not move by a bit
        idx = live_index(spans)
        idx = idx[idx % 7 == 0]
        assert torch.equal(got[-1][0][idx], p0[idx]) and not got[-1][1][idx].any() and not got[-1][2][idx].any()


def case_skip(r, capturable, device, measured=None):
    spans = spans_of(StandIn(r.form, r.lead))[1]
    seen = []

    def each(t, model, opt, before):
        if t in r.skip[1]:
            assert same_bits(before, bits(opt), spans, r.skip[0]), t        # p, m, v of the withheld parameter: not a bit changed
            seen.append(t)
        else:
            assert not same_bits(before[:1], bits(opt)[:1], spans, r.skip[0]), t
    model, opt, got, p0 = follows_ref(r, capturable, device, measured, each=each)
    assert seen == list(r.skip[1])
    if r.mode == "mirrored":                        # the slot still held step t-1's gradient on the skipped steps, and the launch read it
        assert opt._gather is None and model._arena.slot(getattr(model, r.skip[0])).abs().max() > 0


def case_gather(r, capturable, device, measured=None):
    model, opt, got, p0 = follows_ref(r, capturable, device, measured)
    assert opt._gather is not None


def case_all_none(capturable, device, measured=None):
    model, opt, store = build(BASE, capturable, device)
    run(BASE, capturable, device, steps=2, built=(model, opt, store))
    before = bits(opt)
    place(BASE, model, store, gradients(spans_of(model)[0])[2], [])
    opt.step(grad_scale=BASE.scale)
    assert same_bits(before, bits(opt), None) and count(opt) == 2 and (opt.t == 0 if capturable else opt.step_dev is None)


def case_parked(capturable, device, measured=None):
    model, opt, store = build(PARKED, capturable, device)
    dead0 = model.dead.detach().cpu().clone()
    model, opt, got, p0 = run(PARKED, capturable, device, built=(model, opt, store))
    total, spans, active = spans_of(model)
    within_bound(PARKED, errors(got, reference(PARKED, model, p0), p0, live_index(spans)), f"parked capturable={capturable}", measured)
    a, n = spans["dead"]
    assert a >= active and torch.equal(model.dead.detach().cpu(), dead0)
    assert not opt.exp_avg[a:a + n].any() and not opt.exp_avg_sq[a:a + n].any()
    names = [k for k, _ in model.named_parameters()]
    sd = opt.state_dict()
    assert names.index("dead") not in sd["state"] and set(sd["state"]) == set(range(len(names))) - {names.index("dead")}


def case_lr_written(capturable, device, measured=None):
    model, opt, got, p0 = follows_ref(LR_WRITTEN, capturable, device, measured)
    assert opt.lr == 3e-3 and opt.betas == (0.8, 0.99)


def case_resume_own(cap_from, cap_to, device, measured=None):
    """3 steps, checkpoint through torch.save / torch.load, a fresh model and a fresh FlatAdam built with OTHER hyper-parameters, 2 more
    steps on both: not a bit apart, and the hyper-parameters are the checkpoint's."""
    model, opt, store = build(BASE, cap_from, device)
    run(BASE, cap_from, device, steps=3, built=(model, opt, store))
    f = io.BytesIO()
    torch.save({"opt": opt.state_dict(), "model": {k: v.cpu() for k, v in model.state_dict().items()}}, f)
    f.seek(0)
    ck = torch.load(f, weights_only=False)
    model2, opt2, store2 = build(BASE, cap_to, device, weights=ck["model"], **OTHER)
    assert opt2.lr == OTHER["lr"]
    opt2.load_state_dict(ck["opt"])
    g = opt2.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (BASE.lr, BASE.betas, BASE.eps, BASE.wd)
    assert count(opt2) == 3 and same_bits(bits(opt), bits(opt2), None)
    run(BASE, cap_from, device, first=4, built=(model, opt, store))
    run(BASE, cap_to, device, first=4, built=(model2, opt2, store2))
    assert count(opt) == count(opt2) == 5
    assert same_bits(bits(opt), bits(opt2), None)
    for (k, a), (_, b) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(a, b), k


def _torch_first3(r, device, foreach=None):
    """A model of row r whose own torch.optim.Adam (fp32, on `device`) has taken 3 steps with every gradient present."""
    model = StandIn(r.form, r.lead).to(device)
    total, spans, _ = spans_of(model)
    p0 = flat_of(model, spans, total)
    topt = torch.optim.Adam(model.parameters(), lr=r.lr, betas=r.betas, eps=r.eps, weight_decay=r.wd, foreach=foreach)
    for t in range(1, 4):
        for k, p in model.named_parameters():
            a, n = spans[k]
            p.grad = None if k == "dead" else (gradients(total)[t - 1][a:a + n].to(device) * r.scale).view_as(p)
        topt.step()
    return model, topt, p0


def case_resume_from_torch(capturable, device, measured=None, promote=False):
    """torch.optim.Adam takes 3 steps, FlatAdam continues for 2 (load_state_dict of its state_dict(); promote: through
    FlatAdam.from_torch_adam): steps 4 and 5 against the float64 Adam that took all 5 (adam_ref64 = float64 torch.optim.Adam where
    nothing is skipped, checked in e32())."""
    r = BASE
    model, topt, p0 = _torch_first3(r, device, foreach=None if promote else False)
    if promote:
        opt = FlatAdam.from_torch_adam(topt, model, capturable=capturable)
        assert opt is not None and opt.capturable == capturable
    else:
        opt = FlatAdam(model, capturable=capturable, **OTHER)
        opt.load_state_dict(topt.state_dict())
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (r.lr, r.betas, r.eps, r.wd) and count(opt) == 3
    total, spans, _ = spans_of(model)
    store = {"buf": torch.zeros(total, device=device)}
    rr = row("resume", form=r.form, mode="separate", wd=r.wd, scale=r.scale)
    at3 = snap(opt)
    model, opt, got, _ = run(rr, capturable, device, first=4, built=(model, opt, store))
    ref = reference(r, model, p0)
    err = errors([None, None, at3] + got, ref, p0, live_index(spans), first=3)
    within_bound(r, err, f"resume_from_torch capturable={capturable}", measured)
    assert count(opt) == 5


def case_resume_into_torch(capturable, device, measured=None):
    """FlatAdam takes 3 steps, torch.optim.Adam loads its state_dict() and takes 2 more: all 5 against adam_ref64."""
    r = BASE
    model, opt, got, p0 = run(r, capturable, device, steps=3)
    total, spans, _ = spans_of(model)
    topt = torch.optim.Adam(model.parameters(), lr=0.37, foreach=False)
    topt.load_state_dict(opt.state_dict())
    g = topt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (r.lr, r.betas, r.eps, r.wd)
    if torch.device(device).type == "cpu":
        g["capturable"] = False                      # torch's own CPU step has no capturable path; the state is what is under test
    for t in (4, 5):
        for k, p in model.named_parameters():
            a, n = spans[k]
            p.grad = None if k == "dead" else (gradients(total)[t - 1][a:a + n].to(device) * r.scale).view_as(p)
        topt.step()
        flat = [opt.flat.detach().double().cpu().clone(), torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)]
        for k, p in model.named_parameters():
            if k != "dead":
                a, n = spans[k]
                st = topt.state[p]
                assert int(st["step"]) == t, (k, t)
                flat[1][a:a + n], flat[2][a:a + n] = st["exp_avg"].double().cpu().reshape(-1), st["exp_avg_sq"].double().cpu().reshape(-1)
        got.append(tuple(flat))
    assert model.dead not in topt.state or not topt.state[model.dead]
    err = errors(got, reference(r, model, p0), p0, live_index(spans))
    within_bound(r, err, f"resume_into_torch capturable={capturable}", measured)


def case_resume_refusals(capturable, device, measured=None):
    r = BASE
    model, opt, got, p0 = run(r, capturable, device, steps=3)
    total, spans, _ = spans_of(model)
    names = [k for k, _ in model.named_parameters()]
    sd = opt.state_dict()
    sd["state"][names.index("s16")]["step"] = torch.tensor(2.0)
    model2, opt2, _ = build(r, capturable, device)
    with pytest.raises(ValueError, match="step counts differ"):
        opt2.load_state_dict(sd)
    sd = opt.state_dict()
    del sd["state"][names.index("s16")]
    model3, opt3, _ = build(r, capturable, device, **OTHER)
    opt3.exp_avg.fill_(3.0); opt3.exp_avg_sq.fill_(3.0)
    opt3.load_state_dict(sd)
    a, n = spans["s16"]
    assert count(opt3) == 3 and not opt3.exp_avg[a:a + n].any() and not opt3.exp_avg_sq[a:a + n].any()
    keep = torch.ones(total, dtype=torch.bool)
    keep[a:a + n] = False
    assert torch.equal(opt3.exp_avg.cpu()[keep], opt.exp_avg.cpu()[keep]) and torch.equal(opt3.exp_avg_sq.cpu()[keep], opt.exp_avg_sq.cpu()[keep])


def case_disowned(capturable, device, measured=None):
    model, opt, store = build(BASE, capturable, device)
    run(BASE, capturable, device, steps=2, built=(model, opt, store))
    total, spans, _ = spans_of(model)
    model.s16.data = model.s16.data.clone()
    place(BASE, model, store, gradients(total)[2], present(BASE, spans, 3))
    before, moved = bits(opt), model.s16.detach().cpu().clone()
    with pytest.raises(RuntimeError, match="no longer lives in the optimizer's flat buffer"):
        opt.step(grad_scale=BASE.scale)
    assert same_bits(before, bits(opt), None) and count(opt) == 2 and torch.equal(model.s16.detach().cpu(), moved)


def table():
    """[(id, callable(capturable, device, measured))] - every row of the table but resume_own, which has its own four pairs."""
    out = [(r.name, functools.partial(case_plain, r)) for r in PLAIN]
    out += [(r.name, functools.partial(case_skip, r)) for r in SKIPS]
    out += [(r.name, functools.partial(case_gather, r)) for r in GATHER]
    out += [("all_none", case_all_none), ("parked", case_parked), ("lr_written", case_lr_written),
            ("resume_from_torch", case_resume_from_torch), ("resume_into_torch", case_resume_into_torch),
            ("resume_refusals", case_resume_refusals), ("disowned", case_disowned)]
    return out
