"""Evaluator sweep of one source, plain against config.prefix_sweep, on the GPU.

    python scripts/prefix_sweep_probe.py [--out profiles] [--val-iters 3] [--reps 3]

ANP and CondNeuralProcess (max) at the shape of the reference's cfg/evaluation/ANP_ShapeNet3D.yaml - 20 tasks, max_ctx_num 25, 30
views per object, 64 x 64 x 3 - on mlhot.synth.SyntheticViews through the u8 ingest, `val_iters` cut to 3.  Both sweeps run in this
process on the same evaluator: the plain one is `_validate_iter` per context size (the code path without the config key), the
prefix one `_validate_prefixes`.  One warm-up sweep of each, then `reps` timed sweeps alternating, each between device
synchronisations (both end in their own fetch as well); the median is reported.  One further sweep of each runs under the
library's launch profiler for the per-label times and the launch counts.  Writes <out>/prefix_sweep.json and the paragraph of
<out>/INDEX_prefix_sweep.md."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--val-iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
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
