"""Evaluator sweep of one source, plain against config.prefix_sweep, on the GPU.

    python scripts/prefix_sweep_probe.py [--out profiles] [--val-iters 3] [--reps 3]
    python scripts/prefix_sweep_probe.py --fold [--out profiles]      # prefix sweep against prefix sweep + config.prefix_sweep_fold

ANP and CondNeuralProcess (max) at the shape of the reference's cfg/evaluation/ANP_ShapeNet3D.yaml - 20 tasks, max_ctx_num 25, 30
views per object, 64 x 64 x 3 - on mlhot.synth.SyntheticViews through the u8 ingest, `val_iters` cut to 3.  Both sweeps run in this
process on the same evaluator: the plain one is `_validate_iter` per context size (the code path without the config key), the
prefix one `_validate_prefixes`.  One warm-up sweep of each, then `reps` timed sweeps alternating, each between device
synchronisations (both end in their own fetch as well); the median is reported.  One further sweep of each runs under the
library's launch profiler for the per-label times and the launch counts.  Writes <out>/prefix_sweep.json and the paragraph of
<out>/INDEX_prefix_sweep.md.

`--fold` is the third leg under the same protocol: the prefix sweep (the baseline: the code path without config.prefix_sweep_fold)
against the prefix sweep with the fold on, same process, same evaluator, alternating; plus the row-invariant Linear kernel alone
against mlhot_linear_fwd at 15000 x 2048 -> 256 and 15000 x 512 -> 256, timed by the launch profiler.  Writes
<out>/prefix_sweep_fold.json and <out>/INDEX_prefix_sweep_fold.md."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))

T, K, VIEWS = 20, 25, 30
CFG = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
MODELS = {"ANP": "attention", "CondNeuralProcess": "max"}


def group(label):
    if label.startswith("trunk."):
        return "trunks"
    if label.startswith("favor") or label.startswith("agg"):
        return "attention / aggregation"
    if label.startswith("loss"):
        return "loss"
    if label.startswith("ingest"):
        return "ingest"
    return "linears and the rest"


def measure(method, agg, val_iters, reps):
    import torch
    import mlhot
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot.synth import SyntheticViews
    from trainer.losses import LossFunc
    lib = mlhot.lib()
    cfg = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, iterations=0, val_iters=val_iters, max_ctx_num=K,
                                contrastive=False, logger=None, save_path=tempfile.mkdtemp(prefix="prefix_probe_"), agg_mode=agg, **CFG)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(cfg.device)
    ev = ModelEvaluator(model=model, loss=LossFunc("mse", "shapenet_3d"), config=cfg, data=SyntheticViews("shapenet_3d", objects=40, views=VIEWS))
    assert ev.ingest is not None and ev._prefix_property("validation")

    def plain():
        return [ev._validate_iter("validation", k) for k in range(1, K + 1)]

    def prefix():
        return ev._validate_prefixes("validation")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    (_, a), (_, b) = timed(plain), timed(prefix)              # warm-up: kernels loaded, allocator and ingest buffers sized
    worst = max(abs(x[0] - y) for x, y in zip(a, b[0]))
    ms = {"plain": [], "prefix": []}
    for _ in range(reps):
        ms["plain"].append(timed(plain)[0])
        ms["prefix"].append(timed(prefix)[0])
    labels = {}
    for name, fn in (("plain", plain), ("prefix", prefix)):
        lib.prof_begin(1 << 16)
        fn()
        torch.cuda.synchronize()
        rec = lib.prof_end()
        by = {}
        for label, t in rec:
            g = by.setdefault(group(label), [0, 0.0])
            g[0] += 1
            g[1] += t
        labels[name] = {"launches": len(rec), "launches_per_sweep_point": round(len(rec) / K, 1),
                        "by_group_ms": {g: {"launches": n, "ms": round(t, 3)} for g, (n, t) in sorted(by.items())}}
    enc_passes = 2 if agg == "attention" else 1                      # the encoder sees context + targets (ANP) or the context only
    distinct = {"plain": sum(k + VIEWS for k in range(1, K + 1)), "prefix": K + VIEWS}
    passes = {"plain": sum(k + enc_passes * VIEWS for k in range(1, K + 1)), "prefix": K + enc_passes * VIEWS}
    p, q = statistics.median(ms["plain"]), statistics.median(ms["prefix"])
    return {"model": method, "agg_mode": agg, "tasks": T, "max_ctx_num": K, "views": VIEWS, "val_iters": val_iters, "reps": reps,
            "plain_ms": round(p, 2), "prefix_ms": round(q, 2), "plain_ms_all": [round(x, 2) for x in ms["plain"]],
            "prefix_ms_all": [round(x, 2) for x in ms["prefix"]], "ratio": round(p / q, 2),
            "images_per_task_and_iteration": distinct, "image_count_ratio": round(distinct["plain"] / distinct["prefix"], 2),
            "trunk_pass_images_per_task_and_iteration": passes, "trunk_pass_ratio": round(passes["plain"] / passes["prefix"], 2),
            "largest_loss_difference": worst, "profile": labels}


def _profile(lib, fn, torch, points):
    lib.prof_begin(1 << 16)
    fn()
    torch.cuda.synchronize()
    rec = lib.prof_end()
    by, lab = {}, {}
    for label, t in rec:
        g = by.setdefault(group(label), [0, 0.0])
        g[0] += 1
        g[1] += t
        l = lab.setdefault(label, [0, 0.0])
        l[0] += 1
        l[1] += t
    return {"launches": len(rec), "launches_per_sweep_point": round(len(rec) / points, 1), "device_ms": round(sum(t for _, t in rec), 3),
            "by_group_ms": {g: {"launches": n, "ms": round(t, 3)} for g, (n, t) in sorted(by.items())},
            "by_label_ms": {l: {"launches": n, "ms": round(t, 3)} for l, (n, t) in sorted(lab.items())}}


def measure_fold(method, agg, val_iters, reps):
    """Prefix sweep with config.prefix_sweep_fold off (the baseline) and on: wall time, device time per label, launches."""
    import torch
    import mlhot
    from evaluator.model_evaluator import ModelEvaluator
    from mlhot.synth import SyntheticViews
    from trainer.losses import LossFunc
    lib = mlhot.lib()
    cfg = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, iterations=0, val_iters=val_iters, max_ctx_num=K,
                                contrastive=False, logger=None, save_path=tempfile.mkdtemp(prefix="prefix_probe_"), agg_mode=agg,
                                prefix_sweep=True, **CFG)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(cfg.device)
    ev = ModelEvaluator(model=model, loss=LossFunc("mse", "shapenet_3d"), config=cfg, data=SyntheticViews("shapenet_3d", objects=40, views=VIEWS))
    assert ev.ingest is not None and ev._prefix_property("validation")

    def leg(fold):
        def run():
            cfg.prefix_sweep_fold = fold
            return ev._validate_prefixes("validation")
        return run

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    legs = {"prefix": leg(False), "fold": leg(True)}
    (_, a), (_, b) = timed(legs["prefix"]), timed(legs["fold"])          # warm-up of each
    worst = max(abs(x - y) for x, y in zip(a[0], b[0]))
    ms = {"prefix": [], "fold": []}
    for _ in range(reps):
        for name in ("prefix", "fold"):
            ms[name].append(timed(legs[name])[0])
    prof = {name: _profile(lib, legs[name], torch, K) for name in ("prefix", "fold")}
    p, q = statistics.median(ms["prefix"]), statistics.median(ms["fold"])
    return {"model": method, "agg_mode": agg, "tasks": T, "max_ctx_num": K, "views": VIEWS, "val_iters": val_iters, "reps": reps,
            "prefix_ms": round(p, 2), "fold_ms": round(q, 2), "prefix_ms_all": [round(x, 2) for x in ms["prefix"]],
            "fold_ms_all": [round(x, 2) for x in ms["fold"]], "ratio": round(p / q, 2), "largest_loss_difference": worst, "profile": prof}


def measure_kernel(reps=20):
    """mlhot_linear_rows_fwd against mlhot_linear_fwd (the 64-row-tile route at this M) on the same inputs, per-launch device time."""
    import torch
    import mlhot
    lib = mlhot.lib()
    out = []
    for M, Kin, N in ((15000, 2048, 256), (15000, 512, 256)):
        g = torch.Generator().manual_seed(1)
        x = torch.randn(M, Kin, generator=g).cuda()
        w = (torch.randn(N, Kin, generator=g) / Kin ** 0.5).cuda()
        b = torch.randn(N, generator=g).cuda()
        for _ in range(3):
            lib.linear_rows_fwd([(x, 1, 0)], w, b, "relu")
            lib.linear_fwd(x, w, b, "relu")
        torch.cuda.synchronize()
        lib.prof_begin(4 * reps + 16)
        for _ in range(reps):
            lib.linear_rows_fwd([(x, 1, 0)], w, b, "relu")
            lib.linear_fwd(x, w, b, "relu")
        torch.cuda.synchronize()
        by = {}
        for label, t in lib.prof_end():
            by.setdefault(label, []).append(t * 1e3)
        gflop = 2.0 * M * Kin * N / 1e9
        row = {"M": M, "K": Kin, "N": N, "reps": reps}
        for label, ts in by.items():
            med = statistics.median(ts)
            row[label] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2), "tflops_at_median": round(gflop / med * 1e3, 2)}
        out.append(row)
    return out


def main_fold(a):
    res = [measure_fold(m, agg, a.val_iters, a.reps) for m, agg in MODELS.items()]
    kern = measure_kernel()
    with open(os.path.join(a.out, "prefix_sweep_fold.json"), "w") as f:
        json.dump({"probe": "scripts/prefix_sweep_probe.py --fold", "results": res, "kernel": kern}, f, indent=1)
    lines = ["# Folded prefix sweep (DESIGN.md \"prefix sweep\", folded) - config.prefix_sweep against config.prefix_sweep + prefix_sweep_fold", "",
             f"`python scripts/prefix_sweep_probe.py --fold`: {T} tasks, max_ctx_num {K}, {VIEWS} views of 64 x 64 x 3, val_iters {a.val_iters}, "
             f"median of {a.reps} sweeps each, alternating in one process, between device synchronisations, after one warm-up sweep of each; "
             "device time and launches from the library's launch profiler on one further sweep of each; numbers in `prefix_sweep_fold.json`.", ""]
    for r in res:
        pr = r["profile"]
        def parts(name):
            return ", ".join(f"{g} {v['ms']:.2f} ms in {v['launches']} launches" for g, v in pr[name]["by_group_ms"].items())
        lines += [f"- **{r['model']} ({r['agg_mode']})**: prefix sweep {r['prefix_ms']} ms, folded {r['fold_ms']} ms: {r['ratio']} x.  Device time "
                  f"{pr['prefix']['device_ms']} -> {pr['fold']['device_ms']} ms, launches per sweep point {pr['prefix']['launches_per_sweep_point']} -> "
                  f"{pr['fold']['launches_per_sweep_point']}.  By label, prefix: {parts('prefix')}; folded: {parts('fold')}.  Largest difference of "
                  f"the loss means: {r['largest_loss_difference']:.1e}.", ""]
    for k in kern:
        labels = ", ".join(f"{l} {v['median_us']} us ({v['tflops_at_median']} TFLOP/s)" for l, v in k.items() if isinstance(v, dict))
        lines += [f"- **kernel alone, {k['M']} x {k['K']} -> {k['N']}** (median of {k['reps']} launches, alternating): {labels}.", ""]
    with open(os.path.join(a.out, "INDEX_prefix_sweep_fold.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "prefix_sweep_fold", "results": [{k: r[k] for k in ("model", "prefix_ms", "fold_ms", "ratio")} for r in res], "kernel": kern}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold", action="store_true", help="third leg: prefix sweep against prefix sweep + fold, and the kernel alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--val-iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.fold:
        return main_fold(a)
    res = [measure(m, agg, a.val_iters, a.reps) for m, agg in MODELS.items()]
    with open(os.path.join(a.out, "prefix_sweep.json"), "w") as f:
        json.dump({"probe": "scripts/prefix_sweep_probe.py", "results": res}, f, indent=1)
    lines = ["# Prefix sweep (DESIGN.md \"prefix sweep\") - the evaluator's sweep of one source, plain against config.prefix_sweep", "",
             f"`python scripts/prefix_sweep_probe.py`: {T} tasks, max_ctx_num {K}, {VIEWS} views of 64 x 64 x 3, val_iters {a.val_iters}, "
             f"median of {a.reps} sweeps each, alternating, between device synchronisations, after one warm-up sweep of each; numbers in "
             "`prefix_sweep.json`.", ""]
    for r in res:
        pr = r["profile"]
        def parts(name):
            return ", ".join(f"{g} {v['ms']:.2f} ms in {v['launches']} launches" for g, v in pr[name]["by_group_ms"].items())
        lines += [f"- **{r['model']} ({r['agg_mode']})**: plain {r['plain_ms']} ms, prefix {r['prefix_ms']} ms: {r['ratio']} x, against an image-count "
                  f"ratio of {r['image_count_ratio']} ({r['trunk_pass_ratio']} counting every trunk pass).  Launches per sweep point "
                  f"{pr['plain']['launches_per_sweep_point']} -> {pr['prefix']['launches_per_sweep_point']}.  Device time by label, plain: {parts('plain')}; "
                  f"prefix: {parts('prefix')}.", ""]
    with open(os.path.join(a.out, "INDEX_prefix_sweep.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "prefix_sweep", "results": [{k: r[k] for k in ("model", "plain_ms", "prefix_ms", "ratio", "image_count_ratio")} for r in res]}))


if __name__ == "__main__":
    main()
