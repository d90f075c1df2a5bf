"""mlhot.optim.FlatAdam on the device: tests/flat_adam_cases.py's table through mlhot.lib() (single launches over fewer than 3000
floats), the promotion of a torch.optim.Adam that has already stepped, one captured step replayed, and the trainer re-capturing its
graphs when a hyper-parameter is written between iterations."""
import os
import types

import pytest
import torch

from tests import flat_adam_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE = C.table()


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("name", [n for n, _ in TABLE])
def test_flat_adam_case(gpulib, name, capturable):
    if name == "resume_from_torch":                 # CUDA parameters: through the promotion the trainer uses
        return C.case_resume_from_torch(capturable, DEV, promote=True)
    dict(TABLE)[name](capturable, DEV)


@pytest.mark.parametrize("cap_to", [False, True])
@pytest.mark.parametrize("cap_from", [False, True])
def test_flat_adam_resume_own(gpulib, cap_from, cap_to):
    C.case_resume_own(cap_from, cap_to, DEV)


@pytest.mark.parametrize("capturable", [False, True])
def test_promoting_an_adam_that_never_stepped_starts_at_zero(gpulib, capturable):
    from mlhot.optim import FlatAdam
    model = C.StandIn().to(DEV)
    opt = FlatAdam.from_torch_adam(torch.optim.Adam(model.parameters(), lr=3e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.02), model, capturable=capturable)
    g = opt.param_groups[0]
    assert C.count(opt) == 0 and opt.t == 0 and (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (3e-3, (0.8, 0.9), 1e-6, 0.02)
    assert not opt.exp_avg.any() and not opt.exp_avg_sq.any() and opt.state_dict()["state"] == {}


def test_captured_step_replays(gpulib):
    """One FlatAdam(capturable=True).step() captured on a side stream (mlhot.graphs.capture, the trainer's helper) over static gradient
    tensors - the mirror arena's, one parameter without a gradient whose slot holds a stale one - after one eager step, replayed 3 times
    with the gradients rewritten in place in between: not a bit from 4 eager steps, and the device count is 4."""
    from mlhot.graphs import capture
    r = C.row("captured", wd=0.01, scale=0.5, skip=("s257", (1, 2, 3, 4)))
    total, spans, _ = C.spans_of(C.StandIn())
    gs, names = C.gradients(total), C.present(r, spans, 1)
    ends = []
    for replayed in (False, True):
        model, opt, store = C.build(r, True, DEV)
        store["buf"].normal_(generator=torch.Generator(DEV).manual_seed(3))          # the withheld parameter's slot: never zero, never read
        stale = model._arena.slot(model.s257).clone()
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            C.place(r, model, store, gs[0], names)
            opt.step(grad_scale=r.scale)
            if replayed:
                graph = torch.cuda.CUDAGraph()
                with capture(graph, side):
                    opt.step(grad_scale=r.scale)
        torch.cuda.current_stream().wait_stream(side)
        assert C.count(opt) == 1                    # a capture executes nothing
        for t in (2, 3, 4):
            C.place(r, model, store, gs[t - 1], names)        # same tensors, new values
            if replayed:
                graph.replay()
            else:
                opt.step(grad_scale=r.scale)
        torch.cuda.synchronize()
        assert int(opt.step_dev.item()) == 4 and opt._gather is None and torch.equal(model._arena.slot(model.s257), stale)
        ends.append(C.bits(opt))
    assert C.same_bits(ends[0], ends[1], None)
    a, n = spans["s257"]
    assert not ends[1][1][a:a + n].any() and not ends[1][2][a:a + n].any()            # never stepped: no moments
    assert not torch.equal(ends[1][0][:a], C.flat_of(C.StandIn(), spans, total).float()[:a])       # ... and the others did move


def test_trainer_recaptures_on_lr_change(gpulib, tmp_path, monkeypatch):
    """A hyper-parameter written between two replayed iterations: ModelTrainer._graph_train_iter drops its graphs, counts the
    re-capture, runs that iteration eagerly and captures again - and the 8 iterations (weight decay 0.01, lr 1e-3 -> 5e-4 behind
    iteration 4) land on the weights and losses of the eager loop bit for bit.  The harness of
    test_graph_replayed_training_equals_eager_training (tests/test_gpu_parity.py) with the context size pinned, so that one shape
    repeats, and the loss read right behind the step (lagged_loss_log=False): the write goes through a wrapped `_report`, which the
    late log would call one iteration later in the replayed loop than in the eager one."""
    from mlhot.optim import FlatAdam
    from mlhot.synth import SyntheticData, get_batch, get_batch_u8
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer

    class Pinned(SyntheticData):
        def _seed(self, source):
            rng = {"train": self.rng, "validation": self.val_rng, "test": self.test_rng}[source]
            self._step += 1
            return int(rng.randint(0, 2 ** 31 - 1))

        def get_batch(self, source, tasks_per_batch, shot):
            return get_batch(self.task, tasks_per_batch, 4 if source == "train" else shot, shot, seed=self._seed(source))

        def get_batch_u8(self, source, tasks_per_batch, shot):
            return get_batch_u8(self.task, tasks_per_batch, 4 if source == "train" else shot, shot, seed=self._seed(source))

    monkeypatch.chdir(tmp_path)
    finals, losses = [], []
    for graph in (False, True):
        cfg = types.SimpleNamespace(device=torch.device(DEV), seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3,
                                    output_dim=2, agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64,
                                    dim_z=64, task="shapenet_1d", iterations=8, val_freq=1000, val_iters=1, bg_gen_freq=1000, gen_bg=False,
                                    max_ctx_num=5, beta=0, contrastive=False, graph_steps=graph, log_every=1, lagged_loss_log=False,
                                    save_path=str(tmp_path / f"g{int(graph)}"), logger=None)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        opt = FlatAdam(model, lr=1e-3, weight_decay=0.01, ctx_num=5, test_num=5, capturable=True)
        tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=opt, config=cfg, data=Pinned())
        seen, orig = [], tr._report

        def report(it, v, _o=orig, _s=seen, _tr=tr):
            _s.append(v)
            if it == 4:
                _tr.optimizer.param_groups[0]["lr"] = 5e-4
            return _o(it, v)
        tr._report = report
        tr.train()
        assert len(seen) == 8 and tr.optimizer is opt and opt.lr == 5e-4
        assert tr.recaptures == (1 if graph else 0)
        if graph:
            assert [isinstance(v, tuple) for v in tr._graphs.values()] == [True]       # one shape, captured again behind the change
        assert int(opt.step_dev.item()) == 8
        assert os.path.exists(tmp_path / f"g{int(graph)}" / "models" / "model_end_8.pt")
        losses.append(seen)
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
    assert losses[0] == losses[1] and len(set(losses[0])) == 8
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
