"""Per-task context sizes and growing states: what the mask costs and what extend saves, on the GPU.

    python scripts/ragged_context_probe.py [--out profiles] [--reps 5]

6c's shape - ANP and CondNeuralProcess (max), 20 tasks, 25 context shots, 64 x 64 x 3 - and 6c-2's - ANPShapeNet1D and CNPShapeNet1D
(mean), 10 tasks, 15 shots, 128 x 128 x 1 - random images on the device.  Legs, alternating in this process, each between device
synchronisations, after one warm-up of each; the median of `reps` is reported:
  a   `condition(ctx_x, ctx_y)` at Nc shots: the unmasked call;
  b   `condition(..., ctx_len=[Nc] * T)`: the same context through the masked path (b / a: the cost of the mask and of the packed list);
  c   `condition(..., ctx_len=mixed)`, lengths spread evenly over 1 .. Nc - 1, mean Nc / 2;
  d   `extend` by one shot per task of a state that holds Nc - 1 shots in Nc slots;
  e   a fresh `condition` on the grown context of Nc shots (e / d: what extend saves; the yardstick is the image-count ratio Nc).
One further run of a, b, c and d goes under the library's launch profiler: the device time by label, and the key launches masked
(favor.keys1r / favor.keys2r) against unmasked (favor.keys1 / favor.keys2).  Reads nothing outside the repository.
Writes <out>/ragged_context.json and <out>/INDEX_ragged_context.md."""
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

CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
             task="shapenet_1d", input_dim=3, output_dim=2)
# name -> (class, configuration, tasks, context shots, image shape, label width)
MODELS = {
    "ANP": ("ANP", dict(CFG3D, agg_mode="attention"), 20, 25, (3, 64, 64), 4),
    "CondNeuralProcess (max)": ("CondNeuralProcess", dict(CFG3D, agg_mode="max"), 20, 25, (3, 64, 64), 4),
    "ANPShapeNet1D": ("ANPShapeNet1D", dict(CFG1D, agg_mode="attention", dim_r=64), 10, 15, (1, 128, 128), 3),
    "CNPShapeNet1D (mean)": ("CNPShapeNet1D", dict(CFG1D, agg_mode="mean", dim_r=100), 10, 15, (1, 128, 128), 3),
}
KEY_LABELS = ("favor.keys1", "favor.keys2", "favor.keys1r", "favor.keys2r")


def _profile(lib, fn, torch):
    lib.prof_begin(1 << 12)
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


def measure(name, reps):
    import torch
    import mlhot
    from mlhot import cached
    method, cfg, T, NC, img, L = MODELS[name]
    lib = mlhot.lib()
    c = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, **cfg)
    model = getattr(importlib.import_module("networks." + method), method)(c).to(c.device).eval()
    g = torch.Generator().manual_seed(3)
    cx, cy = torch.rand(T, NC, *img, generator=g).cuda(), torch.rand(T, NC, L, generator=g).cuda()
    qx = torch.rand(T, 4, *img, generator=g).cuda()
    mixed = [1 + (t * (NC - 2)) // (T - 1) for t in range(T)]
    head_x, head_y = cx[:, :NC - 1].contiguous(), cy[:, :NC - 1].contiguous()
    last_x, last_y = cx[:, NC - 1:].contiguous(), cy[:, NC - 1:].contiguous()
    short = cached.condition(model, head_x, head_y, capacity=NC)
    legs = {"a": lambda: cached.condition(model, cx, cy),
            "b": lambda: cached.condition(model, cx, cy, ctx_len=[NC] * T),
            "c": lambda: cached.condition(model, cx, cy, ctx_len=mixed),
            "d": lambda: cached.extend(model, short, last_x, last_y),
            "e": lambda: cached.condition(model, cx, cy)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    warm = {k: timed(f)[1] for k, f in legs.items()}
    mu = {k: cached.predict(model, warm[k], qx) for k in ("a", "b", "d")}
    scale = mu["a"].abs().max().item()
    diff = {k: (mu[k] - mu["a"]).abs().max().item() / scale for k in ("b", "d")}
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    prof = {k: _profile(lib, legs[k], torch) for k in ("a", "b", "c", "d")}
    keys = {k: {l: prof[k]["by_label_ms"][l]["ms"] for l in KEY_LABELS if l in prof[k]["by_label_ms"]} for k in prof}
    return {"model": name, "tasks": T, "Nc": NC, "mixed_ctx_len": mixed, "mean_mixed": round(sum(mixed) / T, 2), "reps": reps,
            **{k + "_ms": round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "b_over_a": round(med["b"] / med["a"], 2), "c_over_a": round(med["c"] / med["a"], 2), "e_over_d": round(med["e"] / med["d"], 2),
            "image_count_ratio": NC, "images": {"a": T * NC, "b": T * NC, "c": sum(mixed), "d": T, "e": T * NC},
            "difference_to_a_of_mu_scale": diff, "key_launches_ms": keys, "profile": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(name, a.reps) for name in MODELS]
    with open(os.path.join(a.out, "ragged_context.json"), "w") as f:
        json.dump({"probe": "scripts/ragged_context_probe.py", "results": res}, f, indent=1)
    lines = ["# Per-task context sizes and growing states (DESIGN.md 6c-3) - the cost of the mask, what extend saves", "",
             f"`python scripts/ragged_context_probe.py`: median of {a.reps} runs per leg, the legs alternating in one process between device "
             "synchronisations after one warm-up of each.  a = `condition` at Nc shots, b = the same with `ctx_len = [Nc] * T` (masked path), c = "
             "mixed lengths of mean Nc / 2, d = `extend` by one shot per task of a state of Nc - 1 shots, e = a fresh `condition` on the grown "
             "context.  Yardstick for e / d: the image-count ratio Nc.  Device time by label from the library's launch profiler on one further "
             "run; numbers in `ragged_context.json`.", "",
             "| model (T, Nc) | a ms | b ms | c ms | d ms | e ms | b / a | c / a | e / d | image-count ratio |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['model']} ({r['tasks']}, {r['Nc']}) | {r['a_ms']} | {r['b_ms']} | {r['c_ms']} | {r['d_ms']} | {r['e_ms']} | {r['b_over_a']} | "
                     f"{r['c_over_a']} | {r['e_over_d']} | {r['image_count_ratio']} |")
    lines.append("")
    for r in res:
        def labels(leg):
            return ", ".join(f"{l} {v['ms'] * 1e3:.1f} us x{v['launches']}" for l, v in r["profile"][leg]["by_label_ms"].items())
        lines += [f"- **{r['model']}** device time by label: " + "; ".join(f"{leg} {r['profile'][leg]['device_ms']} ms in {r['profile'][leg]['launches']} "
                  f"launches ({labels(leg)})" for leg in ("a", "b", "c", "d")) + f".  Key launches (ms): {json.dumps(r['key_launches_ms'])}.  predict on b's / d's "
                  f"state against a's: {r['difference_to_a_of_mu_scale']['b']:.1e} / {r['difference_to_a_of_mu_scale']['d']:.1e} of mu's scale.", ""]
    with open(os.path.join(a.out, "INDEX_ragged_context.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "ragged_context", "results": [{k: r[k] for k in ("model", "a_ms", "b_ms", "c_ms", "d_ms", "e_ms", "b_over_a", "e_over_d", "key_launches_ms")} for r in res]}))


if __name__ == "__main__":
    main()
