"""Numbers of the resident image pool, kernel leg: on one shipped ShapeNet3D batch (600 images of 64 x 64) the plain
mlhot_ingest_u8_nhwc on RGB bytes (the byte route's kernel), the pool entry without and with composition, and the augmenting pool
entry - alternating runs in one process, HIP events, medians, five warm-up rounds of each - and, on the host, what one regeneration
of the backgrounds costs a reference-style loader per 1000 objects (the work the route removes).  Writes pool_ingest.json and
INDEX_pool_ingest.md into --out.
    python scripts/pool_probe.py [--reps 200] [--out profiles]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "what-matters-for-meta-learning_amd"), ROOT]


def host_regeneration_ms(pool, bank, views, objects):
    """One regeneration as the reference's loader walks it (dataset/shapenet_3d.py:231-254): per object one np.where over every image
    index, a fancy-index copy of its RGBA views as k / 255 floats, the masked blend, the write back.  -> ms per 1000 objects."""
    images = pool.astype(np.float32) / np.float32(255.0)
    f_bank = bank.astype(np.float32) / np.float32(255.0)
    item_indices = np.repeat(np.arange(images.shape[0] // views), views)
    rng = np.random.RandomState(0)
    t0 = time.perf_counter()
    for obj in range(objects):
        where = np.where(item_indices == obj)[0]
        item = images[where]
        bg = f_bank[rng.choice(f_bank.shape[0], item.shape[0])]
        mask = (item[..., 3] < 1.0)[..., None]
        item[..., :3] = item[..., :3] * mask + bg * (1 - mask)
        images[where] = item
    return 1e3 * (time.perf_counter() - t0) / objects * 1000


def main():
    import mlhot
    from mlhot import augment as A
    from mlhot.synth import SyntheticViewsRGBA
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_probe: needs the MI355X (a CPU timing says nothing about it)")
    L, dev, n, H = mlhot.lib(), "cuda:0", 600, 64
    data = SyntheticViewsRGBA(seed=1, objects=40, views=30)
    pool_np, bank_np = data.rgba_pool("train")
    pool, bank = torch.from_numpy(pool_np).to(dev), torch.from_numpy(bank_np).to(dev)
    ids_np = np.random.default_rng(0).integers(0, pool_np.shape[0], n).astype(np.int32)
    bg_np = A.BackgroundSampler(bank_np.shape[0], seed=1).batch(ids_np, 3)
    ids, bg, none = torch.from_numpy(ids_np).to(dev), torch.from_numpy(bg_np).to(dev), torch.full((n,), -1, dtype=torch.int32, device=dev)
    rgb = torch.from_numpy(np.ascontiguousarray(pool_np[ids_np][..., :3])).to(dev)
    t = A.ImageSampler("shapenet_3d", seed=1).batch(n // 2, n // 2, H, H)
    rec, luts, ct = torch.from_numpy(t.records).to(dev), torch.from_numpy(t.luts).to(dev), A.colour_tables(dev)
    out = torch.empty(n, 3, H, H, device=dev)
    legs = {
        "plain ingest (RGB bytes)": lambda: L.ingest_u8_nhwc(rgb, out=out),
        "pool, bg = -1": lambda: L.pool_ingest_u8(pool, ids, bank, none, out=out),
        "pool, composed": lambda: L.pool_ingest_u8(pool, ids, bank, bg, out=out),
        "augmenting ingest (RGB bytes)": lambda: L.augment_ingest_u8_img(rgb, rec, luts, ct, out=out),
        "pool, composed + augmented": lambda: L.pool_augment_ingest_u8_img(pool, ids, rec, bank, bg, luts, ct, out=out),
    }
    runs = {k: [] for k in legs}
    for i in range(args.reps + 5):                          # alternating legs; the first five rounds are warm-up
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if i >= 5:
                runs[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: float(np.median([a.elapsed_time(b) for a, b in v])) * 1e3 for k, v in runs.items()}
    base = us["plain ingest (RGB bytes)"]
    alpha255 = float((pool_np[ids_np][..., 3] == 255).mean())
    # algorithmic bytes per image: RGB 12 KB or RGBA 16 KB read (+ 12 KB of bank where composed), 48 KB of floats written
    moved = {"plain ingest (RGB bytes)": 60, "pool, bg = -1": 64, "pool, composed": 76}
    result = {"images": n, "H": H, "W": H, "reps": args.reps, "median_us": us, "ratio_to_plain_ingest": {k: v / base for k, v in us.items()},
              "GBps": {k: n * kb * 1024 / (us[k] * 1e-6) / 1e9 for k, kb in moved.items()}, "share_of_pixels_with_alpha_255": alpha255,
              "ratio_pool_augmented_to_augmenting_ingest": us["pool, composed + augmented"] / us["augmenting ingest (RGB bytes)"],
              "host_regeneration_ms_per_1000_objects": host_regeneration_ms(pool_np, bank_np, 30, 40),
              "trainer_leg": "not measured"}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "pool_ingest.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = ["# Resident image pool: kernel leg (scripts/pool_probe.py)", "",
             f"{n} images of {H} x {H}, {args.reps} alternating runs per leg in one process after 5 warm-up rounds, HIP events, medians.", "",
             "| leg | median us | x plain ingest | algorithmic GB/s |", "|---|---|---|---|"]
    for k, v in us.items():
        gbps = f"{result['GBps'][k]:.0f}" if k in moved else "-"
        lines.append(f"| {k} | {v:.1f} | {v / base:.2f} | {gbps} |")
    lines += ["", f"Share of gathered pixels with alpha 255 (their bank dwords are read): {alpha255:.2f}.",
              f"Pool, composed + augmented against the augmenting ingest on RGB bytes: {result['ratio_pool_augmented_to_augmenting_ingest']:.2f} x.",
              f"Host regeneration, reference-style walk (one thread, numpy): {result['host_regeneration_ms_per_1000_objects']:.0f} ms per 1000 objects "
              "of 30 views (a host timing on the GPU machine's CPU).",
              "The expectation from bytes moved was 76 KB against 60 KB per image = 1.27 x for the composing leg.",
              "Trainer leg (shipped_ANPMR_ShapeNet3D through ModelTrainer, byte route against resident route): not measured."]
    with open(os.path.join(args.out, "INDEX_pool_ingest.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
