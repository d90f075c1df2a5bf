"""Device data augmentation: the three numbers of DESIGN.md "Device augmentation".

    python scripts/augment_probe.py sampler      host: mlhot.augment.Sampler.batch per meta-batch (no GPU needed)
    python scripts/augment_probe.py kernel       device: the fused kernel on the ShapeNet1D (T=10, Nc=15, Nq=15) and Pascal1D shapes,
                                                 repeated; time it with `rocprofv3 --kernel-trace --stats -- python ... kernel`
    python scripts/augment_probe.py iter         device: iterations of the shipped ANP_ShapeNet1D (cfg/train/shipped_ANP_ShapeNet1D.yaml)
                                                 through trainer.ModelTrainer, device_augment off / on alternating, three runs each

Prints one JSON line per measurement.  The reference's host imgaug path is NOT measured (imgaug is not installed)."""
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))

from mlhot import augment as A          # noqa: E402

SHAPES = {"shapenet_1d": (10, 15, 15), "pascal_1d": (10, 15, 15)}      # T, Nc (the largest drawn), Nq


def sampler(reps=400):
    for task, (T, Nc, Nq) in SHAPES.items():
        s = A.Sampler(task, seed=2578)
        for _ in range(20):
            s.batch(T * Nc, T * Nq, 128, 128)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s.batch(T * Nc, T * Nq, 128, 128)
            t.append(time.perf_counter() - t0)
        t = np.array(t) * 1e6
        print(json.dumps({"probe": "sampler", "task": task, "images": T * (Nc + Nq), "median_us": round(float(np.median(t)), 1),
                          "p90_us": round(float(np.percentile(t, 90)), 1), "reps": reps}), flush=True)


def kernel(reps=200):
    import torch
    import mlhot
    from mlhot.synth import shape_images
    lib = mlhot.lib()
    for task, (T, Nc, Nq) in SHAPES.items():
        n = T * (Nc + Nq)
        table = A.Sampler(task, seed=1).batch(T * Nc, T * Nq, 128, 128)
        src = torch.from_numpy(shape_images(n, seed=3)[..., None]).cuda()
        rec = torch.from_numpy(table.records).cuda()
        luts = torch.from_numpy(table.luts).cuda() if len(table.luts) else None
        out = torch.empty(n, 1, 128, 128, device="cuda")
        plain = torch.empty_like(out)
        for _ in range(10):
            lib.augment_ingest_u8(src, rec, luts, out=out)
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for _ in range(reps):
            lib.augment_ingest_u8(src, rec, luts, out=out)
        e1.record()
        for _ in range(reps):
            lib.ingest_u8_nhwc(src, out=plain)
        e2.record()
        torch.cuda.synchronize()
        print(json.dumps({"probe": "kernel_events", "task": task, "images": n, "augment_us": round(e0.elapsed_time(e1) * 1e3 / reps, 2),
                          "plain_ingest_us": round(e1.elapsed_time(e2) * 1e3 / reps, 2), "reps": reps,
                          "note": "back-to-back launches, event timing; rocprofv3 --stats gives the per-kernel durations"}), flush=True)
        names = ["crop_pad", "gamma", "blur", "affine", "dropout", "coarse_dropout"]
        for op, name in enumerate(names):              # where the time goes: every image with only this step on (where its list has it)
            r1 = table.records.copy()
            has = (r1[:, A.F_OP:A.F_OP + 7] == op) & (np.arange(7)[None, :] < r1[:, A.F_N_STEPS:A.F_N_STEPS + 1])
            if not has.any():
                continue
            r1[:, A.F_ON] = np.where(has.any(axis=1), 1 << op, 0)
            if op == A.GAMMA:
                r1[:, A.F_LUT] = 0
            rd = torch.from_numpy(r1).cuda()
            lut0 = torch.from_numpy(A.gamma_luts([0.7])).cuda()
            for _ in range(5):
                lib.augment_ingest_u8(src, rd, lut0, out=out)
            e0.record()
            for _ in range(reps):
                lib.augment_ingest_u8(src, rd, lut0, out=out)
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"probe": "kernel_events_one_op", "task": task, "op": name, "images_with_it_on": int(has.any(axis=1).sum()),
                              "us": round(e0.elapsed_time(e1) * 1e3 / reps, 2)}), flush=True)


def iteration(iters=600, runs=3):
    import torch
    from mlhot.synth import SyntheticShapes
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    import yaml
    with open(os.path.join(ROOT, "what-matters-for-meta-learning_amd", "cfg", "train", "shipped_ANP_ShapeNet1D.yaml")) as f:
        y = yaml.safe_load(f)
    class Data(SyntheticShapes):
        """One drawn batch per context size, handed out again (the loader's own gather of 300 images, ~1.3 ms, would hide the step)."""
        def get_batch_u8(self, source, tasks_per_batch, shot):
            n_ctx = int(self.rng.randint(3, shot + 1)) if source == "train" else shot
            cache = self.__dict__.setdefault("_cache", {})
            if n_ctx not in cache:
                while True:
                    b = SyntheticShapes.get_batch_u8(self, source, tasks_per_batch, shot)
                    if b[0].shape[1] == n_ctx:
                        cache[n_ctx] = b
                        break
            return cache[n_ctx]

    results = {False: [], True: []}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(runs):
            for on in (False, True):
                cfg = types.SimpleNamespace(**y)
                cfg.device = torch.device("cuda:0")
                cfg.img_size, cfg.input_dim, cfg.output_dim, cfg.beta, cfg.contrastive = [128, 128, 1], 3, 2, 0, False
                cfg.iterations, cfg.val_freq, cfg.gen_bg, cfg.logger, cfg.save_path = iters, 10 ** 9, False, None, tmp
                cfg.aug_list = ["data_aug"]
                cfg.device_augment = on
                torch.manual_seed(0)
                model = ANPShapeNet1D(cfg).to(cfg.device)
                tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"),
                                  optimizer=torch.optim.Adam(model.parameters(), lr=cfg.lr), config=cfg, data=Data(seed=r))
                tr.iterations = iters // 6                                  # warm-up: every context size captured
                tr.train()
                tr.iterations, tr.start_iter = iters, iters // 6 + 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / (iters - iters // 6)
                results[on].append(ms)
                print(json.dumps({"probe": "iteration", "run": r, "device_augment": on, "ms_per_iter": round(ms, 4)}), flush=True)
    off, on = np.median(results[False]), np.median(results[True])
    print(json.dumps({"probe": "iteration_summary", "median_ms_off": round(float(off), 4), "median_ms_on": round(float(on), 4),
                      "ratio": round(float(on / off), 4), "runs": runs, "iters_timed": iters - iters // 6}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "sampler"
    {"sampler": sampler, "kernel": kernel, "iter": iteration}[what]()
