"""Completeness guard of tests/autograd_cases.py: every torch.autograd.Function defined in mlhot.ops has a case, every case names one.
A Function added later fails here until it gets a case, and with it every variant of tests/test_autograd_seam_gpu.py."""
import inspect

import torch

from mlhot import ops
from tests import autograd_cases as AC


def _functions():
    return sorted(n for n, c in vars(ops).items() if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == ops.__name__)


def test_every_function_of_ops_has_a_case_and_every_case_names_a_function():
    have = _functions()
    assert len(have) >= 21
    missing = [n for n in have if n not in AC.FUNCTIONS]
    unknown = [n for n in AC.FUNCTIONS if n not in have]
    assert not missing, f"mlhot.ops Functions without a case in tests/autograd_cases.py: {missing}"
    assert not unknown, f"cases that name no Function of mlhot.ops: {unknown}"


def test_cases_are_well_formed_and_their_references_run():
    names = set()
    for i, c in enumerate(AC.cases()):
        assert c.name not in names, c.name
        names.add(c.name)
        ins = [n for n, _, _ in c.tensors]
        assert len(set(ins)) == len(ins) and all(t.dtype == torch.float32 and t.is_contiguous() for _, t, _ in c.tensors), c.name
        for group in (c.fixed, c.mutable, c.flags, c.job_flags):
            assert set(group) <= set(ins), (c.name, group)
        assert all(d for n, _, d in c.tensors if n in c.flags + c.job_flags), c.name
        ref = AC.reference(i)
        assert (ref is None) == (c.ref is None)
        if ref is None:
            continue
        outs, grads = ref
        assert all(o.dtype == torch.float64 and bool(torch.isfinite(o).all()) for o in outs), c.name
        for n, t, d in c.tensors:
            if d:
                assert grads[n] is not None and grads[n].shape == t.shape and bool(torch.isfinite(grads[n]).all()), (c.name, n)
        for q in c.judge:
            assert q in [f"out{k}" for k in range(len(outs))] + ["d" + n for n in grads], (c.name, q)
