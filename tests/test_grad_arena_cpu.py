"""The gradient arena's contract (mlhot/arena.py, binding._grad_like) on CPU tensors - both are plain torch.

A stand-in Function does what every binding call does: its backward asks _grad_like for the storage of the weight's gradient, writes
the gradient into it and returns it.  With an arena installed the gradients must be the ones the same run gives without one, in
every calling pattern autograd allows: a `.grad` zeroed in place (zero_grad(set_to_none=False)), two backwards accumulated, one
parameter consumed by two nodes of one backward.  In the shipped pattern (`.grad is None` before the backward, one consumer) the
gradient additionally stays a view of `arena.flat` at the same offset on every step: the flat optimizer, GradBucket and graph replay
depend on fixed gradient addresses."""
import pytest
import torch

from mlhot import binding
from mlhot.arena import GradArena


class _Scale(torch.autograd.Function):
    """y = w * x; d w = g * x is written into _grad_like(w) the way a kernel writes its output."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w.detach())
        return x * w

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        out = binding._grad_like(w)
        out.copy_(g * x)
        return None, out


def _params():
    gen = torch.Generator().manual_seed(3)
    return [torch.randn(5, generator=gen).requires_grad_(), torch.randn(2, 3, generator=gen).requires_grad_()]


def _inputs(k):
    gen = torch.Generator().manual_seed(10 + k)
    return [torch.randn(5, generator=gen), torch.randn(2, 3, generator=gen)], [torch.randn(5, generator=gen), torch.randn(2, 3, generator=gen)]


def _backward(ps, k, consumers=1):
    xs, gs = _inputs(k)
    total = 0.0
    for c in range(consumers):
        for p, x, g in zip(ps, xs, gs):
            total = total + (_Scale.apply(x * (c + 1), p) * g).sum()
    total.backward()


def _zeroed_in_place(ps):
    _backward(ps, 0)
    for p in ps:
        p.grad.zero_()
    _backward(ps, 1)


def _two_backwards(ps):
    _backward(ps, 0)
    _backward(ps, 1)


def _two_consumers(ps):
    _backward(ps, 0, consumers=2)


def _shipped(ps):
    for k in range(3):
        for p in ps:
            p.grad = None
        _backward(ps, k)


SITUATIONS = {"zeroed_in_place": _zeroed_in_place, "two_backwards": _two_backwards, "two_consumers": _two_consumers, "shipped": _shipped}


def _run(situation, with_arena):
    ps = _params()
    arena = GradArena(ps).refresh() if with_arena else None
    binding.set_grad_arena(arena)
    try:
        SITUATIONS[situation](ps)
    finally:
        binding.set_grad_arena(None)
    return ps, arena


@pytest.mark.parametrize("situation", list(SITUATIONS))
def test_gradients_with_an_arena_equal_gradients_without(situation):
    plain, _ = _run(situation, False)
    ps, arena = _run(situation, True)
    for i, (p, q) in enumerate(zip(ps, plain)):
        assert torch.equal(p.grad, q.grad), f"{situation}: parameter {i}: with the arena {p.grad.tolist()}, without {q.grad.tolist()}"
    assert binding.get_grad_arena() is None


def test_shipped_pattern_keeps_every_gradient_at_its_slot():
    ps = _params()
    arena = GradArena(ps).refresh()
    binding.set_grad_arena(arena)
    try:
        where = []
        for k in range(3):
            for p in ps:
                p.grad = None
            _backward(ps, k)
            for p in ps:
                assert p.grad.untyped_storage().data_ptr() == arena.flat.untyped_storage().data_ptr()
                assert p.grad.data_ptr() == arena.slot(p).data_ptr() and p.grad.shape == p.shape
            where.append([p.grad.storage_offset() for p in ps])
        assert where[0] == where[1] == where[2]
    finally:
        binding.set_grad_arena(None)


def test_accumulating_into_a_live_gradient_keeps_its_address():
    """zero_grad(set_to_none=False) and micro-batch accumulation: the kernel's output goes elsewhere, autograd adds it INTO the slot."""
    ps = _params()
    arena = GradArena(ps).refresh()
    binding.set_grad_arena(arena)
    try:
        _backward(ps, 0)
        at = [p.grad.data_ptr() for p in ps]
        _backward(ps, 1)
        assert [p.grad.data_ptr() for p in ps] == at == [arena.slot(p).data_ptr() for p in ps]
    finally:
        binding.set_grad_arena(None)


def test_a_tensor_over_several_parameters_is_refused_while_one_of_them_has_a_live_gradient():
    """The stacked per-head weights: the parameters are views of one buffer whose gradient the kernels write as a whole."""
    stack = torch.zeros(4, 3)
    heads = [stack[i].requires_grad_() for i in range(4)]
    arena = GradArena(heads).refresh()
    whole = arena.take(stack)
    assert whole is not None and whole.shape == stack.shape and whole.data_ptr() == arena.flat.data_ptr()
    heads[2].grad = arena.slot(heads[2].detach())
    assert arena.take(stack) is None and arena.take(heads[2].detach()) is None
    assert arena.take(heads[1].detach()) is not None
    heads[2].grad = None
    assert arena.take(stack) is not None
