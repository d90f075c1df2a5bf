"""Cached-context inference against the plain forward, on the GPU.

    python scripts/condition_probe.py [--out profiles] [--reps 5] [--test-log LOG]

ANP and CondNeuralProcess (max) at the shape of the reference's cfg/evaluation/ANP_ShapeNet3D.yaml - 20 tasks, 25 context shots,
64 x 64 x 3 - for Nq = 1, 30 and 300 targets per task, random images on the device.  Three legs, alternating in this process, each
between device synchronisations, after one warm-up of each; the median of `reps` is reported:
  a  the plain `forward(ctx, labels, targets, test=True)`.  Nq = 1 and 30: one call.  Nq = 300: a Python LOOP of ten calls of 30
     targets (what a caller of the plain forward does today to stay inside the two-launch FAVOR+ kernels' 32 shots); nothing is padded;
  b  `condition` once plus `predict`;
  c  `predict` alone on a state made before.
The yardstick for leg c is the image-count ratio of a against c on the same build: (Nc + 2 Nq) / (2 Nq) trunk-pass images for ANP,
(Nc + Nq) / Nq for CondNeuralProcess.  One further run of a and c goes under the library's launch profiler for the per-label
times.  Also: mlhot_favor_query_fwd against mlhot_favor_fwd per launch at Nq = 30 (8 heads, d 256, m 1419), and both against float64.
`--test-log`: the output of `pytest tests/test_condition_gpu.py -s`; its error lines are summarised into the INDEX file.
Writes <out>/condition.json and <out>/INDEX_condition.md."""
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

T, NC, NQS, LOOP = 20, 25, (1, 30, 300), 30
CFG = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape", seed=2578, temperature=0.07)
MODELS = {"ANP": "attention", "CondNeuralProcess": "max"}


def group(label):
    if label.startswith("trunk."):
        return "trunks"
    if label.startswith("favor") or label.startswith("agg"):
        return "attention / aggregation"
    return "linears and the rest"


def _profile(lib, fn, torch):
    lib.prof_begin(1 << 16)
    fn()
    torch.cuda.synchronize()
    rec = lib.prof_end()
    by, lab = {}, {}
    for label, t in rec:
        for key, d in ((group(label), by), (label, lab)):
            e = d.setdefault(key, [0, 0.0])
            e[0] += 1
            e[1] += t
    return {"launches": len(rec), "device_ms": round(sum(t for _, t in rec), 3),
            "by_group_ms": {g: {"launches": n, "ms": round(t, 3)} for g, (n, t) in sorted(by.items())},
            "by_label_ms": {l: {"launches": n, "ms": round(t, 3)} for l, (n, t) in sorted(lab.items())}}


def measure(method, agg, reps):
    import torch
    import mlhot
    lib = mlhot.lib()
    cfg = types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, agg_mode=agg, **CFG)
    model = getattr(importlib.import_module("networks." + method), method)(cfg).to(cfg.device).eval()
    g = torch.Generator().manual_seed(3)
    cx, cy = torch.rand(T, NC, 3, 64, 64, generator=g).cuda(), torch.rand(T, NC, 4, generator=g).cuda()
    out = []
    for Nq in NQS:
        qx = torch.rand(T, Nq, 3, 64, 64, generator=g).cuda()
        parts = [qx[:, i:i + LOOP].contiguous() for i in range(0, Nq, LOOP)]

        def leg_a():
            with torch.no_grad():
                return torch.cat([model(cx, cy, p, test=True)[0] for p in parts], dim=1)

        def leg_b():
            return model.predict(model.condition(cx, cy), qx)

        state = model.condition(cx, cy)

        def leg_c():
            return model.predict(state, qx)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        legs = {"a": leg_a, "b": leg_b, "c": leg_c}
        warm = {k: timed(f)[1] for k, f in legs.items()}
        scale = warm["a"].abs().max().item()
        diff = max((warm[k] - warm["a"]).abs().max().item() / scale for k in ("b", "c"))
        ms = {k: [] for k in legs}
        for _ in range(reps):
            for k, f in legs.items():
                ms[k].append(timed(f)[0])
        med = {k: statistics.median(v) for k, v in ms.items()}
        yard = (NC + 2 * Nq) / (2 * Nq) if agg == "attention" else (NC + Nq) / Nq
        out.append({"model": method, "agg_mode": agg, "tasks": T, "Nc": NC, "Nq": Nq, "reps": reps, "leg_a_calls": len(parts),
                    "a_ms": round(med["a"], 3), "b_ms": round(med["b"], 3), "c_ms": round(med["c"], 3),
                    "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                    "a_over_b": round(med["a"] / med["b"], 2), "a_over_c": round(med["a"] / med["c"], 2), "image_count_ratio": round(yard, 2),
                    "largest_difference_to_a_of_mu_scale": diff,
                    "profile": {"a": _profile(lib, leg_a, torch), "c": _profile(lib, leg_c, torch)}})
    return out


def measure_kernel(reps=20):
    """mlhot_favor_query_fwd against mlhot_favor_fwd on the same inputs at Nq = 30: device time per call, error against float64."""
    import torch
    import mlhot
    from mlhot.ops import favor_keys, favor_query
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    H, d, m, Nq = 8, 256, 1419, 30
    g = torch.Generator().manual_seed(1)
    q, k, v = (0.25 * torch.randn(T, H, n, d, generator=g) for n in (Nq, NC, NC))
    v = 4 * v
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float()
    want = O.favor_attention(q.double(), k.double(), v.double(), proj.double()).permute(0, 2, 3, 1).reshape(T, Nq, d * H)
    qd, kd, vd = (t.permute(0, 2, 1, 3).contiguous().cuda() for t in (q, k, v))
    pd = proj.cuda()
    state = favor_keys(kd, pd)
    err = {}
    for name, got in (("favor_query", favor_query(qd, state, vd, pd)), ("mlhot_favor_fwd", lib.favor_fwd(qd, kd, vd, pd)[0])):
        err[name] = ((got.double().cpu() - want).abs().max() / want.abs().max()).item()
    torch.cuda.synchronize()
    lib.prof_begin(16 * reps + 16)
    for _ in range(reps):
        favor_query(qd, state, vd, pd)
        lib.favor_fwd(qd, kd, vd, pd)
        favor_keys(kd, pd)
    torch.cuda.synchronize()
    by = {}
    for label, t in lib.prof_end():
        by.setdefault(label, []).append(t * 1e3)
    med = {l: round(statistics.median(ts), 2) for l, ts in by.items()}
    return {"T": T, "H": H, "Nq": Nq, "Nc": NC, "d": d, "m": m, "reps": reps, "median_us_by_label": med,
            "favor_query_us": med.get("favor.query"), "favor_fwd_us": round(med.get("favor.f1", 0) + med.get("favor.f2", 0), 2),
            "favor_keys_us": round(med.get("favor.keys1", 0) + med.get("favor.keys2", 0), 2), "error_against_float64": err}


def test_log_summary(path):
    """Worst error per input kind of tests/test_condition_gpu.py::test_query_values_against_float64's printed lines."""
    pat = re.compile(r"favor_query (\w+) d=(\d+) m=(\d+) Nc=(\d+) Nq=(\d+): ([0-9.e+-]+) of out's scale(?:; mlhot_favor_fwd ([0-9.e+-]+))?")
    worst = {}
    with open(path) as f:
        for kind, d, m, nc, nq, e, pe in pat.findall(f.read()):
            w = worst.setdefault(kind, {"favor_query": 0.0, "favor_query_Nq_le_32": 0.0, "mlhot_favor_fwd_Nq_le_32": 0.0, "lines": 0})
            w["lines"] += 1
            w["favor_query"] = max(w["favor_query"], float(e))
            if pe:
                w["favor_query_Nq_le_32"] = max(w["favor_query_Nq_le_32"], float(e))
                w["mlhot_favor_fwd_Nq_le_32"] = max(w["mlhot_favor_fwd_Nq_le_32"], float(pe))
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
    res = [r for m, agg in MODELS.items() for r in measure(m, agg, a.reps)]
    kern = measure_kernel()
    errs = test_log_summary(a.test_log) if a.test_log else None
    with open(os.path.join(a.out, "condition.json"), "w") as f:
        json.dump({"probe": "scripts/condition_probe.py", "results": res, "kernel": kern, "test_errors": errs}, f, indent=1)
    lines = ["# Cached context (DESIGN.md 6c) - condition once, predict for any targets, against the plain forward", "",
             f"`python scripts/condition_probe.py`: {T} tasks, {NC} context shots, 64 x 64 x 3, median of {a.reps} runs per leg, the legs alternating in one "
             "process between device synchronisations after one warm-up of each.  Leg a = plain `forward(test=True)` (one call at Nq 1 and 30; at Nq 300 a "
             "Python loop of ten calls of 30 targets, nothing padded), b = `condition` + `predict`, c = `predict` alone.  Yardstick for a / c: the "
             "image-count ratio (Nc + 2 Nq) / (2 Nq) for ANP, (Nc + Nq) / Nq for CondNeuralProcess.  Device time by label from the library's launch "
             "profiler on one further run; numbers in `condition.json`.", ""]
    for r in res:
        def parts(name):
            return ", ".join(f"{g} {v['ms']:.2f} ms in {v['launches']} launches" for g, v in r["profile"][name]["by_group_ms"].items())
        lines += [f"- **{r['model']} ({r['agg_mode']}), Nq {r['Nq']}**: a {r['a_ms']} ms ({r['leg_a_calls']} call(s)), b {r['b_ms']} ms, c {r['c_ms']} ms: "
                  f"a / b = {r['a_over_b']}, a / c = {r['a_over_c']} against an image-count ratio of {r['image_count_ratio']}.  Device time, a: "
                  f"{r['profile']['a']['device_ms']} ms ({parts('a')}); c: {r['profile']['c']['device_ms']} ms ({parts('c')}).  Largest difference of b, c "
                  f"to a: {r['largest_difference_to_a_of_mu_scale']:.1e} of mu's scale.", ""]
    e = kern["error_against_float64"]
    lines += [f"- **kernel alone, Nq 30** ({T} tasks, 8 heads, Nc {NC}, d 256, m 1419; median of {kern['reps']} calls, alternating): favor_query "
              f"{kern['favor_query_us']} us in one launch, mlhot_favor_fwd {kern['favor_fwd_us']} us in two (F1 + F2), favor_keys {kern['favor_keys_us']} us "
              f"in two.  Error against float64: favor_query {e['favor_query']:.2e}, mlhot_favor_fwd {e['mlhot_favor_fwd']:.2e} of out's scale.", ""]
    if errs:
        lines += ["- **errors against float64 in tests/test_condition_gpu.py** (T 2, H 2, (d, m) in (16, 16), (64, 266), (256, 1419), (256, 1536), Nc in 1, 15, 32, "
                  "Nq in 1, 16, 33, 100; worst over the shapes, of out's own scale): "
                  + "; ".join(f"{k}: favor_query {w['favor_query']:.2e} (Nq <= 32: {w['favor_query_Nq_le_32']:.2e}, mlhot_favor_fwd on the same inputs "
                              f"{w['mlhot_favor_fwd_Nq_le_32']:.2e})" for k, w in errs.items()) + ".", ""]
    with open(os.path.join(a.out, "INDEX_condition.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "condition", "results": [{k: r[k] for k in ("model", "Nq", "a_ms", "b_ms", "c_ms", "a_over_c", "image_count_ratio")} for r in res],
                      "kernel": {k: kern[k] for k in ("favor_query_us", "favor_fwd_us", "favor_keys_us")}}))


if __name__ == "__main__":
    main()
