"""Per-target context masks in predict against the only other route to the same numbers, on the GPU.

    python scripts/context_mask_probe.py [--out profiles] [--reps 5] [--test-log LOG]

Models: ANP (ResNet family; T 20, H 8, d 256, m 1419) and ANPShapeNet1D (vanilla family; T 10, H 8, d 64, m 266), the shapes of the
other cached-context probes; Nc = 32 (form "keys") and 128 (form "long") context shots, Nq = 30 targets, G in {1, 8, Nc} masks, group
g dropping context slot g (leave-one-out over the first G slots).  Legs, alternating in this process, each between device
synchronisations, after one warm-up of each; the median of `reps` wall times is reported:
  masked      predict(context_mask=[T, G, Nq, Nc]) on the conditioned state: one encoder pass over the targets, one masked query launch;
  recondition G times condition() on the context without slot g (gathered inside the leg) plus predict() - what the same numbers cost
              without the mask;
  floor       predict() without a mask on the same state.
`--test-log`: the output of `pytest tests/test_context_mask_gpu.py -s`; its error lines against float64 are summarised per mask
pattern.  Writes <out>/context_mask.json and <out>/INDEX_context_mask.md."""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

NCS, NQ = (32, 128), 30
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
CFG1D = dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d",
             input_dim=3, output_dim=2, dim_r=64)
MODELS = {"ANP": (20, CFG3D, (3, 64, 64), 4, dict(H=8, d=256, m=1419)), "ANPShapeNet1D": (10, CFG1D, (1, 128, 128), 3, dict(H=8, d=64, m=266))}


def measure(method, reps):
    import torch
    from mlhot import cached
    T, cfg, img, L, shape = MODELS[method]
    c = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, agg_mode="attention", **cfg)
    model = getattr(importlib.import_module("networks." + method), method)(c).to(c.device).eval()
    g = torch.Generator().manual_seed(3)
    qx = torch.rand(T, NQ, *img, generator=g).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    rows = []
    for Nc in NCS:
        form = "keys" if Nc <= 32 else "long"
        cx, cy = torch.rand(T, Nc, *img, generator=g).cuda(), torch.rand(T, Nc, L, generator=g).cuda()
        state = cached.condition(model, cx, cy, form=form)
        for G in (1, 8, Nc):
            mask = torch.ones(T, G, NQ, Nc, dtype=torch.bool, device="cuda")
            keeps = []
            for k in range(G):
                mask[:, k, :, k] = False
                keeps.append([n for n in range(Nc) if n != k])

            def recondition():             # the sub-context is gathered inside the leg: G copies of the images would not fit beside each other
                return torch.stack([cached.predict(model, cached.condition(model, cx[:, keep].contiguous(), cy[:, keep].contiguous(),
                                                                           form="keys" if Nc - 1 <= 32 else "long"), qx) for keep in keeps], dim=1)
            legs = {"masked": lambda: cached.predict(model, state, qx, context_mask=mask), "recondition": recondition,
                    "floor": lambda: cached.predict(model, state, qx)}
            warm = {name: timed(f)[1] for name, f in legs.items()}
            diff = ((warm["masked"] - warm["recondition"]).abs().max() / warm["recondition"].abs().max()).item()
            ms = {name: [] for name in legs}
            for _ in range(reps):
                for name, f in legs.items():
                    ms[name].append(timed(f)[0])
            med = {n: round(statistics.median(x), 3) for n, x in ms.items()}
            rows.append({"Nc": Nc, "form": form, "G": G, "ms": med, "ms_all": {n: [round(y, 3) for y in x] for n, x in ms.items()},
                         "masked_against_recondition_of_mu_scale": diff})
            del legs, warm
    return dict(shape, model=method, T=T, Nq=NQ, reps=reps, rows=rows)


def test_log_summary(path):
    """Worst error per mask pattern of tests/test_context_mask_gpu.py::test_masked_read_outs_against_float64's printed lines."""
    pat = re.compile(r"favor_query mask (\w+) Nc=\d+ lens=.*? d=\d+ m=\d+ (\w+) G=\d+: out ([0-9.e+-]+), w ([0-9.e+-]+) of their scales, "
                     r"\|sum_n w - 1\| [0-9.e+-]+ \(([0-9.]+) of the bound\)")
    worst = {}
    with open(path) as f:
        text = f.read()
    for route, pattern, eo, ew, share in pat.findall(text):
        w = worst.setdefault(f"{route} {pattern}", {"out": 0.0, "w": 0.0, "rowsum_share_of_bound": 0.0, "lines": 0})
        w["lines"] += 1
        w["out"], w["w"], w["rowsum_share_of_bound"] = max(w["out"], float(eo)), max(w["w"], float(ew)), max(w["rowsum_share_of_bound"], float(share))
    dom = re.findall(r"dominant shot \d+ of \d+, group without slot \d+: out ([0-9.e+-]+), w ([0-9.e+-]+)", text)
    if dom:
        worst["cached dominant-shot leave-one-out"] = {"out": max(float(a) for a, _ in dom), "w": max(float(b) for _, b in dom), "rowsum_share_of_bound": None,
                                                       "lines": len(dom)}
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--test-log", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(m, a.reps) for m in MODELS]
    errs = test_log_summary(a.test_log) if a.test_log else None
    with open(os.path.join(a.out, "context_mask.json"), "w") as f:
        json.dump({"probe": "scripts/context_mask_probe.py", "results": res, "test_errors": errs}, f, indent=1)
    lines = ["# Per-target context masks in predict (DESIGN.md 6c-10) against conditioning again per subset", "",
             f"`python scripts/context_mask_probe.py`: median of {a.reps} wall times per leg in ms, the legs alternating in one process between device "
             f"synchronisations after one warm-up of each; Nq {NQ} targets; group g of the mask drops context slot g.  masked = `predict(context_mask=)` with G "
             "masks on the conditioned state; recondition = G times `condition` on the context without slot g plus `predict`; floor = `predict` without a "
             "mask.  Numbers in `context_mask.json`.", ""]
    for r in res:
        lines += [f"## {r['model']}: T {r['T']}, H {r['H']}, d {r['d']}, m {r['m']}", "",
                  "| Nc | form | G | masked | recondition | floor | recondition / masked | masked / floor | masked - recondition, of mu's scale |", "|---|---|---|---|---|---|---|---|---|"]
        for row in r["rows"]:
            x = row["ms"]
            lines.append(f"| {row['Nc']} | {row['form']} | {row['G']} | {x['masked']:.3f} | {x['recondition']:.3f} | {x['floor']:.3f} | "
                         f"{x['recondition'] / x['masked']:.1f} | {x['masked'] / x['floor']:.2f} | {row['masked_against_recondition_of_mu_scale']:.1e} |")
        lines.append("")
    if errs:
        lines += ["## Errors against float64 in tests/test_context_mask_gpu.py", "",
                  "Worst per kernel and mask pattern over the shapes of tests/context_mask_cases.py, of the tensor's own scale (the bar is 1e-4); the row sum "
                  "of w as a share of its bound Nc 2^-23:", ""]
        for k, w in errs.items():
            share = "" if w["rowsum_share_of_bound"] is None else f", |sum_n w - 1| at most {w['rowsum_share_of_bound']:.2f} of the bound"
            lines.append(f"- {k}: out {w['out']:.2e}, w {w['w']:.2e}{share}")
        lines.append("")
    with open(os.path.join(a.out, "INDEX_context_mask.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "context_mask", "results": [{"model": r["model"], "rows": [{"Nc": row["Nc"], "G": row["G"], **row["ms"]} for row in r["rows"]]} for r in res]}))


if __name__ == "__main__":
    main()
