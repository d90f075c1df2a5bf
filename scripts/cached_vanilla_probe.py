"""Cached-context inference of the vanilla family against the plain forward, on the GPU.

    python scripts/cached_vanilla_probe.py [--out profiles] [--reps 5]

ANPShapeNet1D and CNPShapeNet1D (mean) at the shipped shape - 10 tasks, 15 context shots, 128 x 128 x 1 - for Nq = 1, 15 and 150
targets per task, random images on the device.  Legs, alternating in this process, each between device synchronisations, after one
warm-up of each; the median of `reps` is reported:
  a   the plain `forward(ctx, labels, targets, test=True)`.  Nq = 1 and 15: one call.  Nq = 150: a Python LOOP of ten calls of 15
      targets (the fused training-shape tails serve 16 targets; nothing is padded);
  b   `mlhot.cached.condition` once plus `predict`;
  c   `predict` alone on a state made before (the fused route);
  c2  `predict(route="composed")` on the same state: the same mathematics from linear_rows / favor_query.
The yardstick for a / c is the image-count ratio (Nc + Nq) / Nq: the vanilla encoder runs once per image in both families.  One further
run of a, c and c2 goes under the library's launch profiler for the per-label device times.
Writes <out>/cached_vanilla.json and <out>/INDEX_cached_vanilla.md."""
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

T, NC, NQS, LOOP = 10, 15, (1, 15, 150), 15
CFG = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
           task="shapenet_1d", input_dim=3, output_dim=2)
MODELS = {"ANPShapeNet1D": ("attention", 64), "CNPShapeNet1D": ("mean", 100)}


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
    return {"launches": len(rec), "device_ms": round(sum(t for _, t in rec), 4),
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
    out = []
    for Nq in NQS:
        qx = torch.rand(T, Nq, 1, 128, 128, generator=g).cuda()
        parts = [qx[:, i:i + LOOP].contiguous() for i in range(0, Nq, LOOP)]
        state = cached.condition(model, cx, cy)

        def leg_a():
            with torch.no_grad():
                return torch.cat([model(cx, cy, p, test=True)[0] for p in parts], dim=1)

        legs = {"a": leg_a, "b": lambda: cached.predict(model, cached.condition(model, cx, cy), qx),
                "c": lambda: cached.predict(model, state, qx, route="fused"), "c2": lambda: cached.predict(model, state, qx, route="composed")}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        warm = {k: timed(f)[1] for k, f in legs.items()}
        scale = warm["a"].abs().max().item()
        diff = max((warm[k] - warm["a"]).abs().max().item() / scale for k in ("b", "c", "c2"))
        ms = {k: [] for k in legs}
        for _ in range(reps):
            for k, f in legs.items():
                ms[k].append(timed(f)[0])
        med = {k: statistics.median(v) for k, v in ms.items()}
        out.append({"model": method, "agg_mode": agg, "tasks": T, "Nc": NC, "Nq": Nq, "reps": reps, "leg_a_calls": len(parts),
                    **{k + "_ms": round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                    "a_over_b": round(med["a"] / med["b"], 2), "a_over_c": round(med["a"] / med["c"], 2), "c2_over_c": round(med["c2"] / med["c"], 2),
                    "image_count_ratio": round((NC + Nq) / Nq, 2), "largest_difference_to_a_of_mu_scale": diff,
                    "profile": {k: _profile(lib, legs[k], torch) for k in ("a", "c", "c2")}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [r for m, (agg, dim_r) in MODELS.items() for r in measure(m, agg, dim_r, a.reps)]
    with open(os.path.join(a.out, "cached_vanilla.json"), "w") as f:
        json.dump({"probe": "scripts/cached_vanilla_probe.py", "results": res}, f, indent=1)
    lines = ["# Cached context of the vanilla family (DESIGN.md 6c-2) - condition once, predict for any targets, against the plain forward", "",
             f"`python scripts/cached_vanilla_probe.py`: {T} tasks, {NC} context shots, 128 x 128 x 1, median of {a.reps} runs per leg, the legs alternating in "
             "one process between device synchronisations after one warm-up of each.  Leg a = plain `forward(test=True)` (one call at Nq 1 and 15; at "
             "Nq 150 a Python loop of ten calls of 15 targets), b = `condition` + `predict`, c = `predict` alone (fused route), c2 = `predict` on the "
             "composed route.  Yardstick for a / c: the image-count ratio (Nc + Nq) / Nq.  Device time by label from the library's launch profiler on "
             "one further run; numbers in `cached_vanilla.json`.", "",
             "| model, Nq | a ms | b ms | c ms | c2 ms | a / c | image-count ratio | c2 / c |", "|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['model']}, {r['Nq']} | {r['a_ms']} | {r['b_ms']} | {r['c_ms']} | {r['c2_ms']} | {r['a_over_c']} | {r['image_count_ratio']} | {r['c2_over_c']} |")
    lines.append("")
    for r in res:
        def labels(name):
            return ", ".join(f"{l} {v['ms'] * 1e3:.1f} us x{v['launches']}" for l, v in r["profile"][name]["by_label_ms"].items())
        lines += [f"- **{r['model']}, Nq {r['Nq']}** device time by label: a {r['profile']['a']['device_ms']} ms in {r['profile']['a']['launches']} launches ({labels('a')}); "
                  f"c {r['profile']['c']['device_ms']} ms in {r['profile']['c']['launches']} ({labels('c')}); c2 {r['profile']['c2']['device_ms']} ms in "
                  f"{r['profile']['c2']['launches']} ({labels('c2')}).  Largest difference of b, c, c2 to a: {r['largest_difference_to_a_of_mu_scale']:.1e} of mu's scale.", ""]
    with open(os.path.join(a.out, "INDEX_cached_vanilla.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "cached_vanilla", "results": [{k: r[k] for k in ("model", "Nq", "a_ms", "b_ms", "c_ms", "c2_ms", "a_over_c", "image_count_ratio")} for r in res]}))


if __name__ == "__main__":
    main()
