"""The fixed-size FAVOR+ summary state against the per-shot forms, on the GPU.

    python scripts/favor_summary_probe.py [--out profiles] [--reps 5] [--test-log LOG]

Shapes (T 20, H 8, d 256, m 1419) and (T 10, H 8, d 64, m 266); context sizes Nc = 32, 64, 128, 256; target counts Nq = 30, 300; random
inputs on the device.  Legs, alternating in this process, each between device synchronisations, after one warm-up of each; the median
of `reps` wall times is reported:
  absorb_all      favor_absorb(None, ..) of all Nc shots (a fresh state, ceil(Nc / 32) kernel calls of two launches);
  absorb_one      favor_absorb(state, one more shot): a NEW state, the old one kept (the operator's contract);
  absorb_one_ip   the same kernel call with state_in == state_out (mlhot_favor_summary_absorb in place);
  summary_query   favor_query on the summary state, ONE launch;
  plain           mlhot_favor_fwd on the kept keys and values of all Nc shots - the parent's only route above 32 shots;
  keys, cached    at Nc = 32: favor_keys, and favor_query on its state - the default form.
Also the state's bytes per shape and, per shape and Nq, the smallest measured Nc at which summary_query is not slower than plain.
`--test-log`: the output of `pytest tests/test_favor_summary_gpu.py -s`; its error lines (the summary route and mlhot_favor_fwd against
float64 on the same inputs) are summarised.  Writes <out>/favor_summary.json and <out>/INDEX_favor_summary.md."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

SHAPES = [dict(T=20, H=8, d=256, m=1419), dict(T=10, H=8, d=64, m=266)]
NCS, NQS = (32, 64, 128, 256), (30, 300)


def measure(shape, reps):
    import torch
    import mlhot
    from mlhot.ops import favor_absorb, favor_keys, favor_query
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    T, H, d, m = (shape[k] for k in "THdm")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()
    k_all, v_all = (s * torch.randn(T, max(NCS) + 1, H, d, generator=g).cuda() for s in (0.25, 1.0))
    qs = {Nq: (0.25 * torch.randn(T, Nq, H, d, generator=g)).cuda() for Nq in NQS}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    rows = []
    for Nc in NCS:
        k, v = k_all[:, :Nc].contiguous(), v_all[:, :Nc].contiguous()
        k1, v1 = k_all[:, Nc:Nc + 1].contiguous(), v_all[:, Nc:Nc + 1].contiguous()
        state = favor_absorb(None, k, v, proj)
        scratch = state.buf.clone()
        legs = {"absorb_all": lambda: favor_absorb(None, k, v, proj), "absorb_one": lambda: favor_absorb(state, k1, v1, proj),
                "absorb_one_ip": lambda: lib.favor_summary_absorb(k1, v1, proj, scratch, out=scratch)}
        for Nq, q in qs.items():
            legs[f"summary_query_{Nq}"] = lambda q=q: favor_query(q, state, None, proj)
            legs[f"plain_{Nq}"] = lambda q=q: lib.favor_fwd(q, k, v, proj)[0]
        if Nc == 32:
            cached = favor_keys(k, proj)
            legs["keys"] = lambda: favor_keys(k, proj)
            for Nq, q in qs.items():
                legs[f"cached_{Nq}"] = lambda q=q: favor_query(q, cached, v, proj)
        warm = {name: timed(f)[1] for name, f in legs.items()}
        diff = {Nq: ((warm[f"summary_query_{Nq}"] - warm[f"plain_{Nq}"]).abs().max() / warm[f"plain_{Nq}"].abs().max()).item() for Nq in NQS}
        ms = {name: [] for name in legs}
        for _ in range(reps):
            for name, f in legs.items():
                ms[name].append(timed(f)[0])
        rows.append({"Nc": Nc, "ms": {n: round(statistics.median(x), 4) for n, x in ms.items()}, "ms_all": {n: [round(y, 4) for y in x] for n, x in ms.items()},
                     "summary_against_plain_of_out_scale": diff})
        del state, scratch, legs, warm
    cross = {}
    for Nq in NQS:
        ok = [r["Nc"] for r in rows if r["ms"][f"summary_query_{Nq}"] <= r["ms"][f"plain_{Nq}"]]
        cross[str(Nq)] = min(ok) if ok else None
    return dict(shape, reps=reps, state_bytes=lib.favor_summary_bytes(T, H, d, m), keys_state_bytes_Nc32=lib.favor_keys_bytes(T, H, 32, d, m),
                flop_count_crossover=round(m * d / (m + d), 1), measured_crossover_Nc=cross, rows=rows)


def test_log_summary(path):
    """Worst error per input kind of tests/test_favor_summary_gpu.py::test_query_values_against_float64's printed lines."""
    pat = re.compile(r"summary favor_query (\w+) d=(\d+) m=(\d+) (\w+): ([0-9.e+-]+) of out's scale(?:; mlhot_favor_fwd on the kept keys ([0-9.e+-]+))?")
    worst = {}
    with open(path) as f:
        for kind, d, m, chunking, e, pe in pat.findall(f.read()):
            w = worst.setdefault(kind, {"summary": 0.0, "summary_where_plain_serves": 0.0, "mlhot_favor_fwd": 0.0, "lines": 0})
            w["lines"] += 1
            w["summary"] = max(w["summary"], float(e))
            if pe:
                w["summary_where_plain_serves"] = max(w["summary_where_plain_serves"], float(e))
                w["mlhot_favor_fwd"] = max(w["mlhot_favor_fwd"], float(pe))
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
    res = [measure(s, a.reps) for s in SHAPES]
    errs = test_log_summary(a.test_log) if a.test_log else None
    with open(os.path.join(a.out, "favor_summary.json"), "w") as f:
        json.dump({"probe": "scripts/favor_summary_probe.py", "results": res, "test_errors": errs}, f, indent=1)
    lines = ["# Fixed-size FAVOR+ summary state (DESIGN.md 6c-4) against the per-shot forms", "",
             f"`python scripts/favor_summary_probe.py`: median of {a.reps} wall times per leg in ms, the legs alternating in one process between device "
             "synchronisations after one warm-up of each.  absorb all = `favor_absorb` of all Nc shots into a fresh state; +1 = one more shot into a NEW "
             "state (the old one kept) / in place; query = `favor_query` on the summary state; plain = `mlhot_favor_fwd` on the kept keys of all Nc "
             "shots (the parent's only route above 32); at Nc 32 also `favor_keys` and `favor_query` on its state (the default form).  Numbers in "
             "`favor_summary.json`.", ""]
    for r in res:
        lines += [f"## T {r['T']}, H {r['H']}, d {r['d']}, m {r['m']}", "",
                  f"Summary state: {r['state_bytes']} bytes whatever Nc (the per-shot key state at Nc 32: {r['keys_state_bytes_Nc32']} bytes, plus the kept "
                  f"values).  FLOP-count crossover m d / (m + d) = {r['flop_count_crossover']}; measured: the summary query is not slower than plain from Nc = "
                  + ", ".join(f"{c} at Nq {nq}" if c else f"none of the measured sizes at Nq {nq}" for nq, c in r["measured_crossover_Nc"].items()) + ".", "",
                  "| Nc | absorb all | +1 new state | +1 in place | " + " | ".join(f"query Nq {q} | plain Nq {q}" for q in NQS) + " |",
                  "|---|---|---|---|" + "---|---|" * len(NQS)]
        for row in r["rows"]:
            x = row["ms"]
            lines.append(f"| {row['Nc']} | {x['absorb_all']:.3f} | {x['absorb_one']:.3f} | {x['absorb_one_ip']:.3f} | "
                         + " | ".join(f"{x[f'summary_query_{q}']:.3f} | {x[f'plain_{q}']:.3f}" for q in NQS) + " |")
        x = r["rows"][0]["ms"]
        lines += ["", "At Nc 32, the default form: favor_keys " + f"{x['keys']:.3f} ms, favor_query on its state "
                  + ", ".join(f"{x[f'cached_{q}']:.3f} ms at Nq {q}" for q in NQS) + ".  Largest difference of the summary query to plain: "
                  + f"{max(max(row['summary_against_plain_of_out_scale'].values()) for row in r['rows']):.1e} of out's scale.", ""]
    if errs:
        lines += ["## Errors against float64 in tests/test_favor_summary_gpu.py", "",
                  "Worst over the shapes (16, 16), (64, 266), (256, 1419) and the chunkings [1], [32, 1], [7, 32, 31] and the ragged one, of out's own scale; "
                  "mlhot_favor_fwd serves the chunkings with equal totals per task:", ""]
        lines += [f"- {k}: summary {w['summary']:.2e} (where mlhot_favor_fwd serves: {w['summary_where_plain_serves']:.2e}, mlhot_favor_fwd on the same "
                  f"inputs {w['mlhot_favor_fwd']:.2e})" for k, w in errs.items()] + [""]
    with open(os.path.join(a.out, "INDEX_favor_summary.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "favor_summary", "results": [{"shape": [r[k] for k in "THdm"], "state_bytes": r["state_bytes"], "crossover": r["measured_crossover_Nc"],
                                                             "rows": [{"Nc": row["Nc"], **row["ms"]} for row in r["rows"]]} for r in res]}))


if __name__ == "__main__":
    main()
