"""Prefix sweep of the vanilla family against the plain K-forward loop, on the GPU.

    python scripts/prefix_vanilla_probe.py [--out profiles] [--reps 5]

ANPShapeNet1D and CNPShapeNet1D (mean) at the shipped evaluation shape (cfg/train/shipped_ANP_ShapeNet1D.yaml: 10 tasks,
max_ctx_num = 15, so 15 context shots and 15 targets, 128 x 128 x 1), random images on the device.  One batch's FULL sweep - the
predictions at every context size 1..15 - three ways, the legs alternating in this process, each between device synchronisations,
after one warm-up of each; the median of `reps` is reported:
  a   the plain loop: `forward(ctx[:, :k], labels[:, :k], targets, test=True)` for k = 1..15 - the evaluator's path without the sweep;
  b   `mlhot.cached.sweep(route="composed")`: one encoder pass, then per k a masked state and the composed tail;
  c   `mlhot.cached.sweep(route="fused")`: one encoder pass, the key side or the prefix aggregate, ONE np.prefix launch.
The yardstick for a / c is the image-count ratio: sum_k (k + 15) = 345 images through the encoder in a, 30 in b and c.  One further run
of each leg goes under the library's launch profiler for the launch list and the per-label device times.
Writes <out>/prefix_vanilla.json and <out>/INDEX_prefix_vanilla.md (whose "error lines" section is kept if the file exists)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

T, NC, NQ = 10, 15, 15
CFG = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
           task="shapenet_1d", input_dim=3, output_dim=2)
MODELS = {"ANPShapeNet1D": ("attention", 64), "CNPShapeNet1D": ("mean", 100)}
ERRORS_HEAD = "## Error lines"


def _profile(lib, fn, torch):
    lib.prof_begin(1 << 14)
    fn()
    torch.cuda.synchronize()
    rec = lib.prof_end()
    lab = {}
    for label, t in rec:
        e = lab.setdefault(label, [0, 0.0])
        e[0] += 1
        e[1] += t
    return {"launches": len(rec), "device_ms": round(sum(t for _, t in rec), 4), "labels": [label for label, _ in rec],
            "by_label_ms": {l: {"launches": n, "ms": round(t, 4)} for l, (n, t) in sorted(lab.items())}}


def measure(method, agg, dim_r, reps):
    import torch
    import mlhot
    from mlhot import cached
    lib = mlhot.lib()
    cfg = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, agg_mode=agg, dim_r=dim_r, **CFG)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(cfg.device).eval()
    g = torch.Generator().manual_seed(3)
    cx, cy = torch.rand(T, NC, 1, 128, 128, generator=g).cuda(), torch.rand(T, NC, 3, generator=g).cuda()
    qx = torch.rand(T, NQ, 1, 128, 128, generator=g).cuda()
    ctx = [(cx[:, :k].contiguous(), cy[:, :k].contiguous()) for k in range(1, NC + 1)]

    def leg_a():
        with torch.no_grad():
            return torch.stack([model(x, y, qx, test=True)[0] for x, y in ctx])

    legs = {"a": leg_a, "b": lambda: cached.sweep(model, cx, cy, qx, route="composed"), "c": lambda: cached.sweep(model, cx, cy, qx, route="fused")}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    warm = {k: timed(f)[1] for k, f in legs.items()}
    scale = warm["a"].abs().max().item()
    diff = {k: (warm[k] - warm["a"]).abs().max().item() / scale for k in ("b", "c")}
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    prof = {k: _profile(lib, legs[k], torch) for k in legs}
    return {"model": method, "agg_mode": agg, "tasks": T, "Nc": NC, "Nq": NQ, "reps": reps,
            **{k + "_ms": round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "a_over_b": round(med["a"] / med["b"], 2), "a_over_c": round(med["a"] / med["c"], 2), "b_over_c": round(med["b"] / med["c"], 2),
            "image_count_ratio": round(sum(k + NQ for k in range(1, NC + 1)) / (NC + NQ), 2),
            "largest_difference_to_a_of_mu_scale": diff, "np_prefix_kernel_ms": prof["c"]["by_label_ms"].get("np.prefix", {}).get("ms"),
            "profile": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(m, agg, dim_r, a.reps) for m, (agg, dim_r) in MODELS.items()]
    with open(os.path.join(a.out, "prefix_vanilla.json"), "w") as f:
        json.dump({"probe": "scripts/prefix_vanilla_probe.py", "results": res}, f, indent=1)
    index = os.path.join(a.out, "INDEX_prefix_vanilla.md")
    kept = ""
    if os.path.exists(index):
        old = open(index).read()
        kept = old[old.index(ERRORS_HEAD):] if ERRORS_HEAD in old else ""
    lines = ["# Prefix sweep of the vanilla family (DESIGN.md 6b-2) - one batch's predictions at every context size", "",
             f"`python scripts/prefix_vanilla_probe.py`: {T} tasks, {NC} context shots, {NQ} targets, 128 x 128 x 1, context sizes 1..{NC}; median of {a.reps} "
             "runs per leg, the legs alternating in one process between device synchronisations after one warm-up of each.  Leg a = the plain loop of "
             f"{NC} `forward(test=True)` calls, b = `mlhot.cached.sweep(route=\"composed\")`, c = `sweep(route=\"fused\")`.  Yardstick for a / c: the "
             "image-count ratio 345 / 30.  Launch list and device time by label from the library's launch profiler on one further run; numbers in "
             "`prefix_vanilla.json`.", "",
             "| model | a ms (plain loop) | b ms (composed) | c ms (fused) | a / b | a / c | b / c | image-count ratio | np.prefix kernel ms |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['model']} | {r['a_ms']} | {r['b_ms']} | {r['c_ms']} | {r['a_over_b']} | {r['a_over_c']} | {r['b_over_c']} | {r['image_count_ratio']} | {r['np_prefix_kernel_ms']} |")
    lines.append("")
    for r in res:
        def labels(name):
            return ", ".join(f"{l} {v['ms'] * 1e3:.1f} us x{v['launches']}" for l, v in r["profile"][name]["by_label_ms"].items())
        lines += [f"- **{r['model']}** launches of c in order: {' '.join(r['profile']['c']['labels'])}.  Device time by label: a {r['profile']['a']['device_ms']} ms in "
                  f"{r['profile']['a']['launches']} launches ({labels('a')}); b {r['profile']['b']['device_ms']} ms in {r['profile']['b']['launches']} ({labels('b')}); "
                  f"c {r['profile']['c']['device_ms']} ms in {r['profile']['c']['launches']} ({labels('c')}).  Largest difference to a: b "
                  f"{r['largest_difference_to_a_of_mu_scale']['b']:.1e}, c {r['largest_difference_to_a_of_mu_scale']['c']:.1e} of mu's scale.", ""]
    with open(index, "w") as f:
        f.write("\n".join(lines) + ("\n" + kept if kept else ""))
    print(json.dumps({"probe": "prefix_vanilla", "results": [{k: r[k] for k in ("model", "a_ms", "b_ms", "c_ms", "a_over_b", "a_over_c", "b_over_c", "np_prefix_kernel_ms")} for r in res]}))


if __name__ == "__main__":
    main()
