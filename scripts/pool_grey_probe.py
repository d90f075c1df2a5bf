"""Numbers of the resident grey pool.  Kernel leg: on one headline batch (480 images of 128 x 128 x 1) each
mlhot_pool1_* entry against its byte twin on the same bytes packed on the device - alternating runs in one process, HIP events,
medians, five warm-up rounds (the protocol of profiles/INDEX_pool_ingest.md); the pool entries once on a pool the size of the batch's
working set and once on a 256 MiB pool.  Trainer leg: ANPShapeNet1D, 16 tasks, 15 + 15 shots through ModelTrainer on
mlhot.synth.SyntheticGreyPool, the byte route against config.resident_pool, alternating runs in one process: ms per iteration, H2D bytes
per batch and host staging time per batch.  Writes pool_grey.json and INDEX_pool_grey.md into --out.
    python scripts/pool_grey_probe.py [--reps 200] [--iters 400] [--out profiles]"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "what-matters-for-meta-learning_amd"), ROOT]


def kernel_leg(reps):
    import mlhot
    from mlhot import augment as A
    L, dev, n, H = mlhot.lib(), "cuda:0", 480, 128
    g = torch.Generator(device=dev).manual_seed(0)
    big = torch.randint(0, 256, (16384, H, H, 1), dtype=torch.uint8, device=dev, generator=g)       # 256 MiB
    small = big[:512].clone()                                                                       # 8 MiB: the size of one batch
    ids_small = torch.from_numpy(np.random.default_rng(0).integers(0, 512, n).astype(np.int32)).to(dev)
    ids_big = torch.from_numpy(np.random.default_rng(1).integers(0, 16384, n).astype(np.int32)).to(dev)
    packed = small[ids_small.long()].contiguous()
    t1 = A.Sampler("shapenet_1d", seed=1).batch(n // 2, n // 2, H, H)
    ti = A.ImageSampler("distractor", seed=1).batch(n // 2, n // 2, H, H)
    r1, l1 = torch.from_numpy(t1.records).to(dev), torch.from_numpy(t1.luts).to(dev)
    ri, ct = torch.from_numpy(ti.records).to(dev), A.colour_tables(dev)
    kw = dict(pre_op=ti.pre_op, div=ti.div, div2=ti.div2)
    out = torch.empty(n, 1, H, H, device=dev)
    legs = {
        "plain ingest (packed bytes)": lambda: L.ingest_u8_nhwc(packed, out=out),
        "grey pool, 8 MiB pool": lambda: L.pool1_ingest_u8(small, ids_small, out=out),
        "grey pool, 256 MiB pool": lambda: L.pool1_ingest_u8(big, ids_big, out=out),
        "1D augmenting ingest (packed bytes)": lambda: L.augment_ingest_u8(packed, r1, l1, out=out),
        "1D augmenting, grey pool": lambda: L.pool1_augment_ingest_u8(small, ids_small, r1, l1, out=out),
        "Distractor augmenting ingest (packed bytes)": lambda: L.augment_ingest_u8_img(packed, ri, None, ct, out=out, **kw),
        "Distractor augmenting, grey pool": lambda: L.pool1_augment_ingest_u8_img(small, ids_small, ri, None, ct, out=out, **kw),
    }
    runs = {k: [] for k in legs}
    for i in range(reps + 5):                               # alternating legs; the first five rounds are warm-up
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if i >= 5:
                runs[k].append((a, b))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) * 1e3 for k, v in runs.items()}


def trainer_run(resident, iters, warm):
    from mlhot import binding
    from mlhot.synth import SyntheticGreyPool
    from networks.ANPShapeNet1D import ANPShapeNet1D
    from trainer.losses import LossFunc
    from trainer.model_trainer import ModelTrainer
    with tempfile.TemporaryDirectory() as tmp:
        cfg = types.SimpleNamespace(device=torch.device("cuda:0"), seed=2578, img_size=[128, 128, 1], tasks_per_batch=16, input_dim=3, output_dim=2,
                                    agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d",
                                    iterations=warm + iters, val_freq=10 ** 9, val_iters=1, bg_gen_freq=10 ** 9, gen_bg=False, max_ctx_num=15, beta=0,
                                    contrastive=False, save_path=tmp, logger=None, resident_pool=resident)
        torch.manual_seed(0)
        model = ANPShapeNet1D(cfg).to(cfg.device)
        data = SyntheticGreyPool("shapenet_1d", seed=3, pool=2048)             # 32 MiB of images
        try:
            tr = ModelTrainer(model=model, loss=LossFunc("mse", "shapenet_1d"), optimizer=torch.optim.Adam(model.parameters(), lr=1e-3), config=cfg,
                              data=data)
            stamps, report = [], tr._report
            tr._report = lambda it, v: (stamps.append(time.perf_counter()), report(it, v))[1]
            tr.train()
            torch.cuda.synchronize()
            ms = 1e3 * (stamps[-1] - stamps[warm]) / (len(stamps) - 1 - warm)
            # what one batch costs the host to put on its way, and what it carries across PCIe (the slot's copy length)
            stage, nbytes = [], []
            for _ in range(60):
                t0 = time.perf_counter()
                ticket = tr._feed._stage("train")
                stage.append(time.perf_counter() - t0)
                nbytes.append(ticket.n_bytes)
                tr._feed.ingest.take(ticket)
            torch.cuda.synchronize()
        finally:
            binding.set_grad_arena(None)
    return ms, 1e3 * float(np.median(stage[10:])), float(np.mean(nbytes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warm", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_grey_probe: needs the MI355X (a CPU timing says nothing about it)")
    us = kernel_leg(args.reps)
    base = us["plain ingest (packed bytes)"]
    legs = {"byte route": [], "resident_pool": []}
    for _ in range(3):                                      # alternating trainer legs in one process
        for name, resident in (("byte route", False), ("resident_pool", True)):
            legs[name].append(trainer_run(resident, args.iters, args.warm))
    trainer = {k: {"ms_per_iteration_runs": [r[0] for r in v], "ms_per_iteration": float(np.median([r[0] for r in v])),
                   "host_staging_ms_per_batch": float(np.median([r[1] for r in v])), "h2d_bytes_per_batch_mean": float(np.mean([r[2] for r in v]))}
               for k, v in legs.items()}
    result = {"images": 480, "H": 128, "W": 128, "reps": args.reps, "median_us": us, "ratio_to_plain_ingest": {k: v / base for k, v in us.items()},
              "GBps": {k: 480 * 80 * 1024 / (us[k] * 1e-6) / 1e9 for k in list(us)[:3]},
              "ratio_1d_augmenting_pool_to_packed": us["1D augmenting, grey pool"] / us["1D augmenting ingest (packed bytes)"],
              "ratio_distractor_augmenting_pool_to_packed": us["Distractor augmenting, grey pool"] / us["Distractor augmenting ingest (packed bytes)"],
              "trainer": trainer, "trainer_iterations": args.iters, "trainer_warm_up": args.warm, "multi_rank": "not measured"}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "pool_grey.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = ["# Resident grey pool: kernel and trainer legs (scripts/pool_grey_probe.py)", "",
             f"480 images of 128 x 128 x 1, {args.reps} alternating runs per leg in one process after 5 warm-up rounds, HIP events, medians.  Every leg "
             "reads 16 KB and writes 64 KB per image.", "",
             "| leg | median us | x plain ingest | algorithmic GB/s |", "|---|---|---|---|"]
    for k, v in us.items():
        gbps = f"{result['GBps'][k]:.0f}" if k in result["GBps"] else "-"
        lines.append(f"| {k} | {v:.1f} | {v / base:.2f} | {gbps} |")
    b, r = trainer["byte route"], trainer["resident_pool"]
    lines += ["", f"1D augmenting entry, grey pool against packed bytes: {result['ratio_1d_augmenting_pool_to_packed']:.3f} x; Distractor augmenting entry: "
              f"{result['ratio_distractor_augmenting_pool_to_packed']:.3f} x.", "",
              f"Trainer leg: ANPShapeNet1D, 16 tasks, 15 + 15 shots (context size drawn per iteration), ModelTrainer.train() on "
              f"mlhot.synth.SyntheticGreyPool (2048 images), {args.iters} timed iterations behind {args.warm} warm-up iterations, three alternating runs per leg "
              "in one process, wall clock between the loss reports.", "",
              "| leg | ms / iteration (median of runs) | runs | H2D bytes / batch (mean) | host staging ms / batch |", "|---|---|---|---|---|"]
    for k, v in trainer.items():
        lines.append(f"| {k} | {v['ms_per_iteration']:.3f} | {', '.join(f'{x:.3f}' for x in v['ms_per_iteration_runs'])} | {v['h2d_bytes_per_batch_mean']:.0f} | "
                     f"{v['host_staging_ms_per_batch']:.3f} |")
    lines += ["", f"resident_pool against the byte route: {r['ms_per_iteration'] / b['ms_per_iteration']:.3f} x per iteration, "
              f"{b['h2d_bytes_per_batch_mean'] / r['h2d_bytes_per_batch_mean']:.0f} x fewer bytes across PCIe, "
              f"{b['host_staging_ms_per_batch'] / r['host_staging_ms_per_batch']:.1f} x less host staging time (draw + gather + fill + copy issue).",
              "The byte route's staging runs under the previous step on one GPU; what eight ranks sharing one host gain is not measured."]
    with open(os.path.join(args.out, "INDEX_pool_grey.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
