"""What shared targets save against the same frame expanded to every task, on the GPU.

    python scripts/shared_query_probe.py [--out profiles] [--reps 5]

One set of Nq query rows asked of T stored contexts, two legs that alternate in this process after one warm-up of each:
    shared      the rows WITHOUT a task axis: favor_query(shared=True) / predict(shared_targets=True)
    expanded    the route there was before: the rows replicated to [T, Nq, ...] (the copy is part of the leg) and the per-task call
Operator alone: `mlhot.ops.favor_query` at the vanilla ANP's shape - H 8, d 64, m 266 - for T in {2, 16}, Nc in {15, 32, 128} (forms
"keys", "keys", "long"), Nq in {1, 15, 300}.  Model: the ResNet ANP (ShapeNet3D, 3 x 64 x 64 images, d 256, m 1419) at T 8, Nc 15,
Nq in {1, 15, 100} through mlhot.cached.predict.  A repetition is CALLS calls between two device synchronisations; the median of
`reps` repetitions is reported per call (wall: Python and launches included).  The library's launch profiler gives the query kernels'
own medians in a run of its own.  No ratio is fixed in advance; out is compared bit for bit (operator) and to the kernels' tolerance
(model).  Writes <out>/shared_query.json and <out>/INDEX_shared_query.md."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

H, D, M = 8, 64, 266
TS, NCS, NQS = (2, 16), (15, 32, 128), (1, 15, 300)
MODEL_T, MODEL_NC, MODEL_NQS = 8, 15, (1, 15, 100)
CALLS = 5


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / CALLS, r


def _alternate(torch, legs, reps):
    """-> ({leg: median us per call}, {leg: every repetition}, {leg: the warm-up's result})"""
    warm = {name: _timed(torch, fn)[1] for name, fn in legs.items()}
    us = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            us[name].append(_timed(torch, fn)[0])
    return {n: statistics.median(x) for n, x in us.items()}, {n: [round(x, 1) for x in xs] for n, xs in us.items()}, warm


def _kernels(torch, lib, fns, reps):
    lib.prof_begin(256 * reps * len(fns) + 64)
    for _ in range(reps):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    by = {}
    for label, t in lib.prof_end():
        by.setdefault(label, []).append(t * 1e3)
    return {label: round(statistics.median(ts), 2) for label, ts in by.items()}


def operator(T, Nc, Nq, reps):
    import torch
    import mlhot
    from mlhot import ops
    from oracle import ref_cpu as O
    g = torch.Generator().manual_seed(1)
    q = (0.25 * torch.randn(Nq, H, D, generator=g)).cuda()
    k, v = (0.25 * torch.randn(T, Nc, H, D, generator=g).cuda() for _ in range(2))
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(M, D).float().cuda()
    form = "keys" if Nc <= 32 else "long"
    state = (ops.favor_keys if form == "keys" else ops.favor_keys_long)(k, proj)
    legs = {"shared": lambda: ops.favor_query(q, state, v, proj, shared=True),
            "expanded": lambda: ops.favor_query(q[None].expand(T, Nq, H, D).contiguous(), state, v, proj)}
    med, all_us, warm = _alternate(torch, legs, reps)
    kern = _kernels(torch, mlhot.lib(), list(legs.values()), reps)
    return {"T": T, "H": H, "d": D, "m": M, "Nc": Nc, "Nq": Nq, "form": form, "reps": reps, "calls_per_rep": CALLS,
            "shared_us": round(med["shared"], 1), "expanded_us": round(med["expanded"], 1), "shared_over_expanded": round(med["shared"] / med["expanded"], 3),
            "us_all": all_us, "kernel_us": kern, "out_bit_equal": bool(torch.equal(warm["shared"], warm["expanded"]))}


def model(Nq, reps):
    import torch
    import mlhot
    from mlhot import cached
    from networks.ANP import ANP
    cfg = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=MODEL_T, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4,
                                output_dim=4, img_agg="reshape", seed=2578, temperature=0.07, agg_mode="attention")
    net = ANP(cfg).cuda().eval()
    g = torch.Generator().manual_seed(2)
    cx, cy = torch.rand(MODEL_T, MODEL_NC, 3, 64, 64, generator=g).cuda(), torch.rand(MODEL_T, MODEL_NC, 4, generator=g).cuda()
    qx = torch.rand(Nq, 3, 64, 64, generator=g).cuda()
    state = cached.condition(net, cx, cy)
    legs = {"shared": lambda: cached.predict(net, state, qx, shared_targets=True),
            "expanded": lambda: cached.predict(net, state, qx[None].expand(MODEL_T, *qx.shape).contiguous())}
    med, all_us, warm = _alternate(torch, legs, reps)
    kern = {name: _kernels(torch, mlhot.lib(), [fn], reps) for name, fn in legs.items()}
    a, b = warm["shared"].double(), warm["expanded"].double()
    return {"model": "ANP (ShapeNet3D)", "T": MODEL_T, "Nc": MODEL_NC, "Nq": Nq, "reps": reps, "calls_per_rep": CALLS,
            "shared_us": round(med["shared"], 1), "expanded_us": round(med["expanded"], 1), "shared_over_expanded": round(med["shared"] / med["expanded"], 3),
            "us_all": all_us, "kernel_us": kern, "kernel_sum_us": {n: round(sum(x.values()), 1) for n, x in kern.items()},
            "rel_err": float((a - b).abs().max() / b.abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    ops_res = [operator(T, Nc, Nq, a.reps) for T in TS for Nc in NCS for Nq in NQS]
    mod_res = [model(Nq, a.reps) for Nq in MODEL_NQS]
    with open(os.path.join(a.out, "shared_query.json"), "w") as f:
        json.dump({"probe": "scripts/shared_query_probe.py", "operator": ops_res, "model": mod_res}, f, indent=1)
    lines = ["# Shared targets (DESIGN.md 6c-16) - one set of query rows against every stored context", "",
             f"`python scripts/shared_query_probe.py`: the shared call against the same rows expanded to [T, Nq, ...] (the copy is part of that leg), the "
             f"legs alternating in one process after one warm-up of each; a repetition is {CALLS} calls between two device synchronisations, median of "
             f"{a.reps} repetitions, per call (wall: Python and launches included).  kernels = the launch profiler's medians in a run of its own.  No ratio "
             "was fixed in advance.  Numbers in `shared_query.json`.", "",
             f"## The operator: `mlhot.ops.favor_query` at H {H}, d {D}, m {M}", "",
             "| T | Nc | form | Nq | shared us | expanded us | shared / expanded | kernels us | out bit-equal |", "|---|---|---|---|---|---|---|---|---|"]
    for r in ops_res:
        kern = ", ".join(f"{k} {v}" for k, v in sorted(r["kernel_us"].items()))
        lines.append(f"| {r['T']} | {r['Nc']} | {r['form']} | {r['Nq']} | {r['shared_us']} | {r['expanded_us']} | {r['shared_over_expanded']} | {kern} | {r['out_bit_equal']} |")
    lines += ["", f"## The model: `mlhot.cached.predict` of the ResNet ANP (ShapeNet3D) at T {MODEL_T}, Nc {MODEL_NC}", "",
              "| Nq | shared us | expanded us | shared / expanded | kernel sum us, shared | kernel sum us, expanded | rel. difference of mu |", "|---|---|---|---|---|---|---|"]
    for r in mod_res:
        lines.append(f"| {r['Nq']} | {r['shared_us']} | {r['expanded_us']} | {r['shared_over_expanded']} | {r['kernel_sum_us']['shared']} | "
                     f"{r['kernel_sum_us']['expanded']} | {r['rel_err']:.2e} |")
    lines.append("")
    with open(os.path.join(a.out, "INDEX_shared_query.md"), "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
