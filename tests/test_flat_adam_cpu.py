"""mlhot.optim.FlatAdam's host logic on CPU tensors: tests/flat_adam_cases.py's table through the host build of the two Adam entries
(tests/hostsim/, the fixture of tests/conftest.py put in the place of mlhot.lib() for mlhot.optim only).  Nothing here needs a GPU."""
import types

import pytest
import torch

from tests import flat_adam_cases as C

TABLE = C.table()


@pytest.fixture
def host(hostsim, monkeypatch):
    monkeypatch.setattr("mlhot.optim.lib", lambda: hostsim)
    return hostsim


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("name", [n for n, _ in TABLE])
def test_flat_adam_case(host, name, capturable):
    dict(TABLE)[name](capturable, "cpu")


@pytest.mark.parametrize("cap_to", [False, True])
@pytest.mark.parametrize("cap_from", [False, True])
def test_flat_adam_resume_own(host, cap_from, cap_to):
    C.case_resume_own(cap_from, cap_to, "cpu")


def test_stand_in_layout():
    """What the table relies on: 16-byte aligned slices with padding between them, the dead parameter parked at `active`, both return
    shapes, fewer than 3000 floats; gradients with exact zeros and 1e-3 <= |g| <= 1 elsewhere."""
    for form in ("two", "three"):
        total, spans, active = C.spans_of(C.StandIn(form))
        assert total < 3000 and all(a % 4 == 0 for a, _ in spans.values())
        ends = sorted((a, a + n) for a, n in spans.values())
        assert all(e <= b for (_, e), (b, _) in zip(ends, ends[1:])) and any(e < b for (_, e), (b, _) in zip(ends, ends[1:]))
        assert (active == total and "dead" not in spans) if form == "two" else (spans["dead"][0] == active < total)
        g = C.gradients(total)
        assert len(g) == C.STEPS and all((v[::7] == 0).all() for v in g)
        nz = torch.cat([v[v != 0].abs() for v in g])
        assert nz.min() >= 1e-3 * (1 - 1e-6) and nz.max() <= 1 and nz.numel() > 4 * total
    p = torch.cat([q.detach().reshape(-1) for q in C.StandIn().parameters()])
    assert p.min() >= -1 and p.max() <= 1 and p.min() < -0.9 and p.max() > 0.9


def test_a_torch_scheduler_is_refused_and_the_trainer_says_what_to_write():
    """A torch.optim.lr_scheduler takes a torch.optim.Optimizer only: FlatAdam is refused by it (TypeError), so the trainer's advice is
    to WRITE trainer.optimizer.param_groups[0]["lr"] - and it warns about a scheduler built on the replaced optimizer exactly when it
    can tell that there is one (the scheduler's constructor leaves `initial_lr` in the optimizer's groups)."""
    from mlhot.optim import FlatAdam
    from trainer.model_trainer import ModelTrainer
    with pytest.raises(TypeError, match="is not an Optimizer"):
        torch.optim.lr_scheduler.StepLR(FlatAdam(C.StandIn(), lr=1e-2), step_size=1)
    said = {}
    for scheduled in (False, True):
        old = torch.optim.Adam(C.StandIn().parameters(), lr=1e-2)
        if scheduled:
            torch.optim.lr_scheduler.StepLR(old, step_size=1)
        lines = []
        me = types.SimpleNamespace(replaced_optimizer=old, _graph_default=False, _host_prefetch=None, _resident=False, _log=lines.append)
        ModelTrainer._announce(me)
        said[scheduled] = " ".join(lines)
    for text in said.values():
        assert 'trainer.optimizer.param_groups[0]["lr"]' in text and "schedule `trainer.optimizer`" not in text
    assert "has no effect" in said[True] and "has no effect" not in said[False]
