"""The prefix sweep beyond 32 context shots against the parent's only route, on the GPU.

    python scripts/prefix_long_probe.py [--out profiles] [--reps 5] [--ncs 64 128 256] [--no-models] [--test-log LOG]

Shapes (T 20, H 8, d 256, m 1419) and (T 10, H 8, d 64, m 266); Nq 30; Nc = 64, 128, 256 with ALL prefix sizes 1..Nc; random inputs on
the device.  Legs, alternating in this process, each between device synchronisations, after one warm-up of each; the median of `reps`
wall times is reported:
  op      mlhot.ops.favor_prefixes_long for all Nc sizes (ceil(Nc / 64) calls of three launches);
  loop    per size: favor_absorb of the next shot, then favor_query on the summary state - 3 launches and one pass over A per size;
  sweep   the whole model: mlhot.cached.sweep on an ANPShapeNet1D-shaped model (T 10) / forward_prefixes(fold=True) on an ANP
          (ResNet, 64x64x3)-shaped one (T 20);
  sweep_loop  per size: extend a summary state by the next shot, then predict - the parent's only route for such a context.
Per-launch times of the op come from the library's event profiler in a separate pass.  `--test-log`: the output of
`pytest tests/test_prefix_long_gpu.py -s`; its error lines are summarised.  Writes <out>/prefix_long.json and
<out>/INDEX_prefix_long.md."""
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

SHAPES = [dict(T=20, H=8, d=256, m=1419, model="ANP"), dict(T=10, H=8, d=64, m=266, model="ANPShapeNet1D")]
NQ = 30
CFG = {"ANPShapeNet1D": dict(seed=2578, temperature=0.07, img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64,
                             task="shapenet_1d", input_dim=3, output_dim=2, agg_mode="attention", dim_r=64),
       "ANP": dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07,
                   agg_mode="attention")}


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _median_legs(legs, reps):
    for f in legs.values():
        _timed(f)
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, f in legs.items():
            ms[name].append(_timed(f)[0])
    return {n: round(statistics.median(x), 4) for n, x in ms.items()}, {n: [round(y, 4) for y in x] for n, x in ms.items()}


def measure(shape, ncs, reps, models):
    import torch
    import mlhot
    from mlhot import cached
    from mlhot.ops import favor_absorb, favor_prefixes_long, favor_query
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    T, H, d, m = (shape[k] for k in "THdm")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()
    k_all, v_all = (s * torch.randn(T, max(ncs), H, d, generator=g).cuda() for s in (0.25, 1.0))
    q = (0.25 * torch.randn(T, NQ, H, d, generator=g)).cuda()
    model = None
    if models:
        cfg = CFG[shape["model"]]
        model = getattr(importlib.import_module("networks." + shape["model"]), shape["model"])(
            types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, **cfg)).cuda().eval()
        Hh, Ww, C = cfg["img_size"]
        C = C - 1 if cfg["task"] == "shapenet_3d" else C
        views, ys = torch.rand(T, max(ncs), C, Hh, Ww, generator=g).cuda(), torch.rand(T, max(ncs), cfg["input_dim"], generator=g).cuda()
    rows = []
    for Nc in ncs:
        k, v = k_all[:, :Nc].contiguous(), v_all[:, :Nc].contiguous()

        def loop():
            state, out = None, []
            for n in range(Nc):
                state = favor_absorb(state, k[:, n:n + 1], v[:, n:n + 1], proj)
                out.append(favor_query(q, state, None, proj))
            return torch.stack(out)
        legs = {"op": lambda: favor_prefixes_long(q, k, v, proj), "loop": loop}
        if model is not None:
            cx, cy, qx = views[:, :Nc].contiguous(), ys[:, :Nc].contiguous(), views[:, :NQ].contiguous()
            if shape["model"] == "ANP":
                legs["sweep"] = lambda: model.forward_prefixes(cx, cy, qx, fold=True)
            else:
                legs["sweep"] = lambda: cached.sweep(model, cx, cy, qx)

            def sweep_loop():
                state, out = None, []
                for n in range(Nc):
                    a, b = cx[:, n:n + 1], cy[:, n:n + 1]
                    state = cached.condition(model, a, b, form="summary") if state is None else cached.extend(model, state, a, b)
                    out.append(cached.predict(model, state, qx))
                return torch.stack(out)
            legs["sweep_loop"] = sweep_loop
        diff = ((legs["op"]() - legs["loop"]()).abs().max() / legs["loop"]().abs().max()).item()
        med, every = _median_legs(legs, reps)
        lib.prof_begin(64)
        try:
            favor_prefixes_long(q, k, v, proj)
            torch.cuda.synchronize()
        finally:
            launches = [(label, round(ms, 4)) for label, ms in lib.prof_end()]
        row = {"Nc": Nc, "ms": med, "ms_all": every, "op_launches_ms": launches, "op_against_loop_of_out_scale": diff,
               "loop_over_op": round(med["loop"] / med["op"], 2), "launches": {"op": len(launches), "loop": 3 * Nc},
               "workspace_bytes": lib.favor_prefix_long_workspace_bytes(T, H, NQ, Nc, d, m, 64)}
        if "sweep" in med:
            row["sweep_loop_over_sweep"] = round(med["sweep_loop"] / med["sweep"], 2)
        rows.append(row)
    return dict(shape, Nq=NQ, reps=reps, rows=rows)


def test_log_summary(path):
    """Worst errors per input kind of tests/test_prefix_long_gpu.py's printed lines."""
    pat = re.compile(r"favor_prefixes_long (\w+) d=(\d+) m=(\d+) Nc=(\d+): ([0-9.e+-]+) of out's scale against float64; mlhot_favor_fwd on the sliced "
                     r"context ([0-9.e+-]+); one against the other ([0-9.e+-]+)")
    old = re.compile(r"favor_prefixes_long against favor_prefixes (\w+) d=(\d+) m=(\d+) Nc=(\d+): ([0-9.e+-]+)")
    worst, route = {}, 0.0
    with open(path) as f:
        text = f.read()
    for kind, _, _, _, e, pe, be in pat.findall(text):
        w = worst.setdefault(kind, {"op": 0.0, "mlhot_favor_fwd": 0.0, "op_against_mlhot_favor_fwd": 0.0, "lines": 0})
        w["lines"] += 1
        w["op"], w["mlhot_favor_fwd"] = max(w["op"], float(e)), max(w["mlhot_favor_fwd"], float(pe))
        w["op_against_mlhot_favor_fwd"] = max(w["op_against_mlhot_favor_fwd"], float(be))
    for *_, e in old.findall(text):
        route = max(route, float(e))
    return {"by_kind": worst, "against_favor_prefixes_up_to_32_shots": route}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ncs", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--no-models", action="store_true")
    ap.add_argument("--test-log", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(s, a.ncs, a.reps, not a.no_models) for s in SHAPES]
    errs = test_log_summary(a.test_log) if a.test_log else None
    with open(os.path.join(a.out, "prefix_long.json"), "w") as f:
        json.dump({"probe": "scripts/prefix_long_probe.py", "results": res, "test_errors": errs}, f, indent=1)
    lines = ["# Prefix sweep beyond 32 context shots (DESIGN.md 6b-3) against the per-size loop", "",
             f"`python scripts/prefix_long_probe.py`: median of {a.reps} wall times per leg in ms, the legs alternating in one process between device "
             "synchronisations after one warm-up of each; Nq 30, all prefix sizes 1..Nc.  op = `favor_prefixes_long` (ceil(Nc / 64) calls of three "
             "launches); loop = per size `favor_absorb` of the next shot and `favor_query` on the summary state (3 Nc launches, A streamed Nc times); "
             "sweep = the whole model (`forward_prefixes(fold=True)` of an ANP-shaped ResNet model / `mlhot.cached.sweep` of an ANPShapeNet1D-shaped one); "
             "sweep loop = per size `extend` by the next shot and `predict`.  Per-launch times of the op from the library's event profiler, one "
             "separate pass.  Numbers in `prefix_long.json`.", ""]
    for r in res:
        has = "sweep" in r["rows"][0]["ms"]
        lines += [f"## T {r['T']}, H {r['H']}, d {r['d']}, m {r['m']} ({r['model']})", "",
                  "| Nc | op | loop | loop / op | launches op / loop | " + ("sweep | sweep loop | sweep loop / sweep | " if has else "") + "op's launches (ms) | workspace MB |",
                  "|---|---|---|---|---|" + ("---|---|---|" if has else "") + "---|---|"]
        for row in r["rows"]:
            x = row["ms"]
            by = {}
            for label, ms in row["op_launches_ms"]:
                by[label] = by.get(label, 0.0) + ms
            lines.append(f"| {row['Nc']} | {x['op']:.3f} | {x['loop']:.3f} | {row['loop_over_op']:.1f} | {row['launches']['op']} / {row['launches']['loop']} | "
                         + (f"{x['sweep']:.3f} | {x['sweep_loop']:.3f} | {row['sweep_loop_over_sweep']:.1f} | " if has else "")
                         + ", ".join(f"{k.split('.')[-1]} {v:.3f}" for k, v in by.items()) + f" | {row['workspace_bytes'] / 2 ** 20:.1f} |")
        lines += ["", f"Largest difference of the op to the loop: {max(row['op_against_loop_of_out_scale'] for row in r['rows']):.1e} of out's scale.", ""]
    if errs:
        lines += ["## Errors in tests/test_prefix_long_gpu.py", "",
                  "Worst over the shapes (16, 16), (64, 266), (256, 1419), Nc in {1, 31, 32, 33, 64, 65, 97}, Nq in {1, 16, 17} and the four prefix sets, of "
                  "out's scale: the op against float64; `mlhot_favor_fwd` on the sliced context against float64 on the same inputs (sizes 1, 32, 33, Nc); "
                  "the op against `mlhot_favor_fwd` on the sliced context:", ""]
        lines += [f"- {k}: op {w['op']:.2e}, mlhot_favor_fwd {w['mlhot_favor_fwd']:.2e}, op against mlhot_favor_fwd {w['op_against_mlhot_favor_fwd']:.2e}"
                  for k, w in errs["by_kind"].items()]
        lines += ["", f"Up to 32 shots, the op against the existing prefix route (`favor_prefixes`): worst {errs['against_favor_prefixes_up_to_32_shots']:.2e} "
                  "of out's scale.", ""]
    with open(os.path.join(a.out, "INDEX_prefix_long.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "prefix_long", "results": [{"shape": [r[k] for k in "THdm"], "rows": [{"Nc": row["Nc"], **row["ms"]} for row in r["rows"]]} for r in res]}))


if __name__ == "__main__":
    main()
