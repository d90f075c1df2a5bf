"""The long per-shot key state against the summary state and the plain route, on the GPU.

    python scripts/favor_long_probe.py [--out profiles] [--reps 5] [--test-log LOG]

Shapes (T 20, H 8, d 256, m 1419) and (T 10, H 8, d 64, m 266); context sizes Nc = 32, 33, 64, 128, 256; target counts Nq = 30, 300; random
inputs on the device.  Legs, alternating in this process, each between device synchronisations, after one warm-up of each; the median
of `reps` wall times is reported:
  long_keys        favor_keys_long of all Nc shots (two launches);
  long_query       favor_query on that state, ONE launch;
  long_query_w     the same with weights=True (w [T, H, Nq, Nc] written beside out);
  absorb_all       favor_absorb(None, ..) of all Nc shots - the summary form's conditioning;
  summary_query    favor_query on the summary state;
  plain            mlhot_favor_fwd on the kept keys and values of all Nc shots - the only other per-shot route above 32 shots;
  keys, cached, cached_w   at Nc = 32: favor_keys and favor_query on its state, without and with weights - the default form, whose
                   bits the long kernels reproduce there.
Also the states' bytes and, per shape and Nq, the measured context sizes at which the long query is not slower than the summary
query.  `--test-log`: the output of `pytest tests/test_favor_long_gpu.py -s`; its error lines against float64 are summarised per input
kind.  Writes <out>/favor_long.json and <out>/INDEX_favor_long.md."""
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
NCS, NQS = (32, 33, 64, 128, 256), (30, 300)


def measure(shape, reps):
    import torch
    import mlhot
    from mlhot.ops import favor_absorb, favor_keys, favor_keys_long, favor_query
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    T, H, d, m = (shape[k] for k in "THdm")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()
    k_all, v_all = (s * torch.randn(T, max(NCS), H, d, generator=g).cuda() for s in (0.25, 1.0))
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
        long, summary = favor_keys_long(k, proj), favor_absorb(None, k, v, proj)
        legs = {"long_keys": lambda: favor_keys_long(k, proj), "absorb_all": lambda: favor_absorb(None, k, v, proj)}
        for Nq, q in qs.items():
            legs[f"long_query_{Nq}"] = lambda q=q: favor_query(q, long, v, proj)
            legs[f"long_query_w_{Nq}"] = lambda q=q: favor_query(q, long, v, proj, weights=True)[0]
            legs[f"summary_query_{Nq}"] = lambda q=q: favor_query(q, summary, None, proj)
            legs[f"plain_{Nq}"] = lambda q=q: lib.favor_fwd(q, k, v, proj)[0]
        if Nc == 32:
            cached = favor_keys(k, proj)
            legs["keys"] = lambda: favor_keys(k, proj)
            for Nq, q in qs.items():
                legs[f"cached_{Nq}"] = lambda q=q: favor_query(q, cached, v, proj)
                legs[f"cached_w_{Nq}"] = lambda q=q: favor_query(q, cached, v, proj, weights=True)[0]
        warm = {name: timed(f)[1] for name, f in legs.items()}
        diff = {Nq: ((warm[f"long_query_{Nq}"] - warm[f"summary_query_{Nq}"]).abs().max() / warm[f"summary_query_{Nq}"].abs().max()).item() for Nq in NQS}
        equal32 = all(torch.equal(warm[f"long_query_{Nq}"], warm[f"cached_{Nq}"]) for Nq in NQS) if Nc == 32 else None
        ms = {name: [] for name in legs}
        for _ in range(reps):
            for name, f in legs.items():
                ms[name].append(timed(f)[0])
        rows.append({"Nc": Nc, "ms": {n: round(statistics.median(x), 4) for n, x in ms.items()}, "ms_all": {n: [round(y, 4) for y in x] for n, x in ms.items()},
                     "long_against_summary_of_out_scale": diff, "long_bit_equal_to_cached": equal32,
                     "long_state_bytes": lib.favor_keys_long_bytes(T, H, Nc, d, m)})
        del long, summary, legs, warm
    ahead = {str(Nq): [r["Nc"] for r in rows if r["ms"][f"long_query_{Nq}"] <= r["ms"][f"summary_query_{Nq}"]] for Nq in NQS}
    return dict(shape, reps=reps, summary_state_bytes=lib.favor_summary_bytes(T, H, d, m), flop_count_crossover=round(m * d / (m + d), 1),
                long_query_not_slower_than_summary_at_Nc=ahead, rows=rows)


def test_log_summary(path):
    """Worst error per input kind of tests/test_favor_long_gpu.py::test_out_and_weights_against_float64's printed lines."""
    pat = re.compile(r"favor_query long (\w+) d=\d+ m=\d+ Nc=\d+ Nq=\d+: out ([0-9.e+-]+), w ([0-9.e+-]+) of their scales, \|sum_n w - 1\| [0-9.e+-]+ \(([0-9.]+) of the bound\)")
    fpat = re.compile(r"favor_keys_long (\w+) d=\d+ m=\d+ Nc=\d+: F_k ([0-9.e+-]+) of its scale")
    worst = {}
    with open(path) as f:
        text = f.read()
    for kind, eo, ew, share in pat.findall(text):
        w = worst.setdefault(kind, {"out": 0.0, "w": 0.0, "rowsum_share_of_bound": 0.0, "F_k": 0.0, "lines": 0})
        w["lines"] += 1
        w["out"], w["w"], w["rowsum_share_of_bound"] = max(w["out"], float(eo)), max(w["w"], float(ew)), max(w["rowsum_share_of_bound"], float(share))
    for kind, ef in fpat.findall(text):
        if kind in worst:
            worst[kind]["F_k"] = max(worst[kind]["F_k"], float(ef))
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
    with open(os.path.join(a.out, "favor_long.json"), "w") as f:
        json.dump({"probe": "scripts/favor_long_probe.py", "results": res, "test_errors": errs}, f, indent=1)
    lines = ["# Long per-shot FAVOR+ key state (DESIGN.md 6c-7) against the summary state and the plain route", "",
             f"`python scripts/favor_long_probe.py`: median of {a.reps} wall times per leg in ms, the legs alternating in one process between device "
             "synchronisations after one warm-up of each.  keys = `favor_keys_long` of all Nc shots; query / +w = `favor_query` on its state without / "
             "with `weights=True`; absorb = `favor_absorb` of all Nc shots into a fresh summary state; sum. = `favor_query` on the summary state; plain "
             "= `mlhot_favor_fwd` on the kept keys of all Nc shots.  Numbers in `favor_long.json`.", ""]
    for r in res:
        lines += [f"## T {r['T']}, H {r['H']}, d {r['d']}, m {r['m']}", "",
                  f"Summary state: {r['summary_state_bytes']} bytes whatever Nc; long state: "
                  + ", ".join(f"{row['long_state_bytes']} at Nc {row['Nc']}" for row in r["rows"]) + " bytes (plus the kept keys and values).  "
                  f"FLOP-count crossover m d / (m + d) = {r['flop_count_crossover']}.  The long query is not slower than the summary query at Nc = "
                  + "; ".join(f"{c if c else 'none of the measured sizes'} at Nq {nq}" for nq, c in r["long_query_not_slower_than_summary_at_Nc"].items()) + ".", "",
                  "| Nc | keys | absorb | " + " | ".join(f"query Nq {q} | +w Nq {q} | sum. Nq {q} | plain Nq {q}" for q in NQS) + " |",
                  "|---|---|---|" + "---|---|---|---|" * len(NQS)]
        for row in r["rows"]:
            x = row["ms"]
            lines.append(f"| {row['Nc']} | {x['long_keys']:.3f} | {x['absorb_all']:.3f} | "
                         + " | ".join(f"{x[f'long_query_{q}']:.3f} | {x[f'long_query_w_{q}']:.3f} | {x[f'summary_query_{q}']:.3f} | {x[f'plain_{q}']:.3f}" for q in NQS) + " |")
        x, r0 = r["rows"][0]["ms"], r["rows"][0]
        lines += ["", f"At Nc 32, the default form: favor_keys {x['keys']:.3f} ms (long keys {x['long_keys']:.3f}); favor_query on its state "
                  + ", ".join(f"{x[f'cached_{q}']:.3f} ms at Nq {q} (long {x[f'long_query_{q}']:.3f}), with weights {x[f'cached_w_{q}']:.3f} (long {x[f'long_query_w_{q}']:.3f})"
                              for q in NQS)
                  + f".  The long query's out bit-equal to the cached one's there: {r0['long_bit_equal_to_cached']}.  Largest difference of the long query to the "
                  f"summary query: {max(max(row['long_against_summary_of_out_scale'].values()) for row in r['rows']):.1e} of out's scale.", ""]
    if errs:
        lines += ["## Errors against float64 in tests/test_favor_long_gpu.py", "",
                  "Worst over the shapes (16, 16), (64, 266) at Nc 33, 48, 64, 65, 255, 256 and (256, 1419) at Nc 65, every Nq, of the tensor's own scale; the row "
                  "sum of w as a share of its bound Nc 2^-23:", ""]
        lines += [f"- {k}: F_k {w['F_k']:.2e}, out {w['out']:.2e}, w {w['w']:.2e}, |sum_n w - 1| at most {w['rowsum_share_of_bound']:.2f} of the bound"
                  for k, w in errs.items()] + [""]
    with open(os.path.join(a.out, "INDEX_favor_long.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "favor_long", "results": [{"shape": [r[k] for k in "THdm"], "ahead": r["long_query_not_slower_than_summary_at_Nc"],
                                                          "rows": [{"Nc": row["Nc"], **row["ms"]} for row in r["rows"]]} for r in res]}))


if __name__ == "__main__":
    main()
