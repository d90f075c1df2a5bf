"""Numbers of the image tasks' device augmentation: the fused kernel against plain mlhot_ingest_u8_nhwc on the same
bytes (alternating runs, HIP events, median), one op at a time, and the host sampler per batch.
    python scripts/augment_img_probe.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "what-matters-for-meta-learning_amd"), ROOT]


def main():
    import mlhot
    from mlhot import augment as A
    from mlhot.synth import colour_images, shape_images
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    reps = ap.parse_args().reps
    L, dev = mlhot.lib(), "cuda:0"
    ct = A.colour_tables(dev)

    def timed(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        return ev, fn

    def median_us(pairs):
        return float(np.median([a.elapsed_time(b) for a, b in pairs])) * 1e3

    # one shipped ShapeNet3D batch: 20 tasks x 30 views of 64 x 64 x 3; one Distractor batch: 20 x 30 of 128 x 128 x 1
    for task, H, C in (("shapenet_3d", 64, 3), ("distractor", 128, 1)):
        n = 600
        imgs = colour_images(n, H, H, seed=1) if C == 3 else shape_images(n, H, H, seed=1)[..., None]
        src = torch.from_numpy(imgs).to(dev)
        sampler = A.ImageSampler(task, seed=1)
        t0 = time.perf_counter()
        for _ in range(20):
            t = sampler.batch(n // 2, n // 2, H, H)
        sampler_us = (time.perf_counter() - t0) / 20 * 1e6
        rec, luts = torch.from_numpy(t.records).to(dev), (torch.from_numpy(t.luts).to(dev) if len(t.luts) else None)
        out = torch.empty(n, C, H, H, device=dev)
        variants = {"all steps": rec}
        steps = sorted({int(o) for o in t.records[:, A.F_OP:A.F_OP + len(sampler.spec.steps)].ravel()})
        for op in steps:                                    # one op at a time: only that op's `on` bit survives
            r = t.records.copy()
            r[:, A.F_ON] &= 1 << op
            variants[f"op {op} alone"] = torch.from_numpy(r).to(dev)
        runs = {k: [] for k in list(variants) + ["plain ingest"]}
        for i in range(reps + 5):                           # alternating runs; the first five are warm-up
            for k in runs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if k == "plain ingest":
                    L.ingest_u8_nhwc(src, out=out)
                else:
                    L.augment_ingest_u8_img(src, variants[k], luts, ct, out=out, pre_op=t.pre_op, div=t.div, div2=t.div2)
                b.record()
                if i >= 5:
                    runs[k].append((a, b))
        torch.cuda.synchronize()
        print(f"{task}: {n} images {H} x {H} x {C}; sampler {sampler_us:.0f} us per batch")
        for k, pairs in runs.items():
            print(f"  {k:14s} {median_us(pairs):8.1f} us")


if __name__ == "__main__":
    main()
