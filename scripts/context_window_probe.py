"""Sliding-window cached contexts, measured.  One process, the legs alternating, the median of 5 per leg:
  * one sliding step (mlhot.cached.slide by one shot) against a fresh condition on the window, windows 32 ("keys"), 256 ("long")
    and 1024 ("paged"), at the ANP shape (T 20, 64 x 64 x 3) and the vanilla shape (T 10, 128 x 128 x 1): wall and device time,
    next to the image-count ratio;
  * updating a summary - retract one shot and absorb one - against absorbing the whole window again, 64 and 256 shots;
  * mlhot_rows_compact alone at [T 20][cap 4096][W 2048]: bytes moved per second.
Writes profiles/context_window.json (or --out).  Usage: python scripts/context_window_probe.py [--out FILE] [--quick]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "what-matters-for-meta-learning_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"
SHAPES = {
    "anp": ("ANP", 20, (3, 64, 64), 4, dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4,
                                             img_agg="reshape", agg_mode="attention")),
    "vanilla": ("ANPShapeNet1D", 10, (1, 128, 128), 3, dict(seed=2578, img_size=[128, 128, 1], input_dim=3, output_dim=2, agg_mode="attention",
                                                            img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d")),
}
WINDOWS = ((32, "keys"), (256, "long"), (1024, "paged"))


def timed(fn):
    """(wall ms, device ms) of one call, the device idle before and after."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    host = (time.perf_counter() - t0) * 1e3          # until the host is free again
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b), host


def legs(named, reps=5):
    """named: {leg: fn}; the legs alternate, one warm-up round first -> {leg: {wall_ms, device_ms, host_ms}} (medians)."""
    for fn in named.values():
        fn()
    got = {k: [] for k in named}
    for _ in range(reps):
        for k, fn in named.items():
            got[k].append(timed(fn))
    return {k: dict(zip(("wall_ms", "device_ms", "host_ms"), (round(statistics.median(x), 4) for x in zip(*v)))) for k, v in got.items()}


def model_for(name):
    method, T, img, L, cfg = SHAPES[name]
    c = types.SimpleNamespace(device=torch.device(DEV), tasks_per_batch=T, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).to(DEV).eval(), T, img, L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_window.json"))
    ap.add_argument("--quick", action="store_true", help="the 32-slot window and the 64-shot summary only")
    args = ap.parse_args()
    import mlhot
    from mlhot import cached
    res = {"device": torch.cuda.get_device_name(0), "slide": [], "summary": [], "rows_compact": {}}
    g = torch.Generator().manual_seed(3)
    for name in SHAPES:
        model, T, img, L = model_for(name)
        for win, form in WINDOWS[:1] if args.quick else WINDOWS:
            cx, cy = torch.rand(T, win, *img, generator=g).to(DEV), torch.rand(T, win, L, generator=g).to(DEV)
            nx, ny = torch.rand(T, 1, *img, generator=g).to(DEV), torch.rand(T, 1, L, generator=g).to(DEV)
            state = cached.condition(model, cx, cy, form=form)
            r = legs({"slide": lambda: cached.slide(model, state, nx, ny), "condition": lambda: cached.condition(model, cx, cy, form=form)})
            res["slide"].append(dict(shape=name, T=T, window=win, form=form, images_ratio=win, **{f"{k}_{m}": v for k, d in r.items() for m, v in d.items()}))
            print(res["slide"][-1], flush=True)
            del state
        for shots in (64,) if args.quick else (64, 256):
            cx, cy = torch.rand(T, shots, *img, generator=g).to(DEV), torch.rand(T, shots, L, generator=g).to(DEV)
            nx, ny = torch.rand(T, 1, *img, generator=g).to(DEV), torch.rand(T, 1, L, generator=g).to(DEV)
            state = cached.condition(model, cx, cy, form="summary")
            ox, oy = cx[:, :1].contiguous(), cy[:, :1].contiguous()
            r = legs({"update": lambda: cached.extend(model, cached.retract(model, state, ox, oy), nx, ny),
                      "reabsorb": lambda: cached.condition(model, cx, cy, form="summary")})
            res["summary"].append(dict(shape=name, T=T, shots=shots, images_ratio=shots / 2, **{f"{k}_{m}": v for k, d in r.items() for m, v in d.items()}))
            print(res["summary"][-1], flush=True)
            del state
        del model
    T, cap, W = 20, 4096, 2048
    src = torch.randn(T, cap, W, device=DEV)
    plan = torch.arange(1, cap + 1, dtype=torch.int32).repeat(T, 1)
    plan[:, -1] = -1
    plan = plan.to(DEV)
    r = legs({"rows_compact": lambda: mlhot.lib().rows_compact([src], plan)})["rows_compact"]
    copy = legs({"clone": lambda: src.clone()})["clone"]
    moved = 2 * src.numel() * 4
    res["rows_compact"] = dict(T=T, cap=cap, W=W, bytes_moved=moved, device_ms=r["device_ms"], GBps=round(moved / r["device_ms"] / 1e6, 1),
                               clone_device_ms=copy["device_ms"], clone_GBps=round(moved / copy["device_ms"] / 1e6, 1),
                               note="device_ms includes the output's allocation; clone is torch's copy of the same bytes, measured alike")
    print(res["rows_compact"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
