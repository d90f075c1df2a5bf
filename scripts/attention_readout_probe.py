"""What the attention read-out costs, on the GPU.

    python scripts/attention_readout_probe.py [--out profiles] [--reps 5] [--test-log LOG]

`mlhot.ops.favor_query` on a cached key state with and without `weights=True` - the same kernel text, the second instantiation
storing w [T, H, Nq, Nc] = S / D beside out - at the two shapes in use: T 20, H 8, d 256, m 1419 (the ResNet family) and T 10, H 8,
d 64, m 266 (the vanilla family), Nc 15 and 32, Nq 30 and 300.  The two legs alternate in this process after one warm-up of each; a
repetition is CALLS calls between two device synchronisations, and the median of `reps` repetitions is reported per call, next to the
kernel's own time from the library's launch profiler (labels favor.query / favor.queryw; a run of its own).  No ratio is fixed in
advance: the yardstick is the leg without the read-out, which is the parent commit's favor_query on the same shape (the plain
instantiation is its kernel).  The store adds T H Nq Nc floats, 6.1 MB at the largest shape here.  The outputs of the two legs are
compared bit for bit.
`--test-log`: the output of `pytest tests/test_attention_readout_gpu.py -s`; its error lines are summarised into the INDEX file.
Writes <out>/attention_readout.json and <out>/INDEX_attention_readout.md."""
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

SHAPES = [(20, 8, 256, 1419), (10, 8, 64, 266)]          # T, H, d, m
NCS, NQS, CALLS = (15, 32), (30, 300), 20


def measure(T, H, d, m, Nc, Nq, reps):
    import torch
    import mlhot
    from mlhot.ops import favor_keys, favor_query
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    g = torch.Generator().manual_seed(1)
    q, k, v = (0.25 * torch.randn(T, n, H, d, generator=g).cuda() for n in (Nq, Nc, Nc))
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()
    state = favor_keys(k, proj)
    assert state.route == "cached"
    legs = {"plain": lambda: favor_query(q, state, v, proj), "read_out": lambda: favor_query(q, state, v, proj, weights=True)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / CALLS, r

    warm = {name: timed(fn)[1] for name, fn in legs.items()}
    out, w = warm["read_out"]
    us = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            us[name].append(timed(fn)[0])
    lib.prof_begin(4 * reps * len(legs) + 16)
    for _ in range(reps):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    by = {}
    for label, t in lib.prof_end():
        by.setdefault(label, []).append(t * 1e3)
    med = {name: statistics.median(x) for name, x in us.items()}
    kern = {label: statistics.median(ts) for label, ts in by.items()}
    return {"T": T, "H": H, "d": d, "m": m, "Nc": Nc, "Nq": Nq, "reps": reps, "calls_per_rep": CALLS, "w_bytes": 4 * w.numel(),
            "plain_us": round(med["plain"], 2), "read_out_us": round(med["read_out"], 2), "read_out_over_plain": round(med["read_out"] / med["plain"], 3),
            "us_all": {name: [round(x, 2) for x in xs] for name, xs in us.items()},
            "kernel_plain_us": round(kern["favor.query"], 2), "kernel_read_out_us": round(kern["favor.queryw"], 2),
            "kernel_read_out_over_plain": round(kern["favor.queryw"] / kern["favor.query"], 3),
            "out_bit_equal": bool(torch.equal(out, warm["plain"])),
            "largest_rowsum_excess": float((w.double().sum(dim=-1) - 1.0).abs().max())}


def test_log_summary(path):
    """Worst figures per input kind of the lines tests/test_attention_readout_gpu.py prints."""
    pat = re.compile(r"favor_query weights (\w+) d=\d+ m=\d+ Nc=\d+ Nq=\d+: w ([0-9.e+-]+) of its scale, \|sum_n w - 1\| [0-9.e+-]+ "
                     r"\(([0-9.]+) of the bound\), sum_n w v against out ([0-9.e+-]+)")
    mpat = re.compile(r"favor_query weights, masked lens=\([0-9, ]+\) d=\d+ m=\d+ Nc=\d+: w ([0-9.e+-]+) of its scale, \|sum_n w - 1\| [0-9.e+-]+ \(([0-9.]+) of the bound\)")
    apat = re.compile(r"predict\(return_attention=True\) (\w+) (?:Nc=\d+|ctx_len=\([0-9, ]+\) of \d+ slots): attn ([0-9.e+-]+) of its scale")
    with open(path) as f:
        text = f.read()
    kinds = {}
    for kind, e, share, through in pat.findall(text):
        k = kinds.setdefault(kind, {"lines": 0, "w": 0.0, "rowsum_share_of_bound": 0.0, "w_v_against_out": 0.0})
        k["lines"] += 1
        k["w"], k["rowsum_share_of_bound"], k["w_v_against_out"] = max(k["w"], float(e)), max(k["rowsum_share_of_bound"], float(share)), max(k["w_v_against_out"], float(through))
    mk = mpat.findall(text)
    models = {}
    for case, e in apat.findall(text):
        models[case] = max(models.get(case, 0.0), float(e))
    return {"kinds": kinds, "models": models,
            "masked": {"lines": len(mk), "w": max((float(e) for e, _ in mk), default=None), "rowsum_share_of_bound": max((float(s) for _, s in mk), default=None)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--test-log", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(*shape, Nc, Nq, a.reps) for shape in SHAPES for Nc in NCS for Nq in NQS]
    errs = test_log_summary(a.test_log) if a.test_log else None
    with open(os.path.join(a.out, "attention_readout.json"), "w") as f:
        json.dump({"probe": "scripts/attention_readout_probe.py", "results": res, "test_errors": errs}, f, indent=1)
    lines = ["# Attention read-out (DESIGN.md 6c-5) - favor_query with and without FAVOR+'s per-shot weights", "",
             f"`python scripts/attention_readout_probe.py`: `mlhot.ops.favor_query` on a cached key state, plain and with `weights=True` (w [T, H, Nq, Nc] = S / D "
             f"stored beside out by the same launch), the legs alternating in one process after one warm-up of each; a repetition is {CALLS} calls between two "
             f"device synchronisations, median of {a.reps} repetitions, per call (wall: Python and launch included).  kernel = the launch profiler's median for "
             "`favor.query` / `favor.queryw` in a run of its own.  The plain leg is the parent commit's favor_query (the same kernel): it is the yardstick; no "
             "ratio was fixed in advance.  Numbers in `attention_readout.json`.", "",
             "| T | H | d | m | Nc | Nq | w bytes | plain us | read-out us | ratio | kernel plain us | kernel read-out us | ratio | out bit-equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['T']} | {r['H']} | {r['d']} | {r['m']} | {r['Nc']} | {r['Nq']} | {r['w_bytes']} | {r['plain_us']} | {r['read_out_us']} | "
                     f"{r['read_out_over_plain']} | {r['kernel_plain_us']} | {r['kernel_read_out_us']} | {r['kernel_read_out_over_plain']} | {r['out_bit_equal']} |")
    lines.append("")
    if errs:
        lines += ["**Errors in tests/test_attention_readout_gpu.py** (T 2, H 2, (d, m) in (16, 16), (64, 266), (256, 1419), (256, 1536), Nc in 1, 15, 16, 17, 32, "
                  "Nq in 1, 17, 100; worst over the shapes; w against float64 of w's own scale, |sum_n w - 1| as a share of the bound Nc 2^-23, sum_n w v against the "
                  "launch's out of out's scale): "
                  + "; ".join(f"{k}: w {e['w']:.2e}, row sum {e['rowsum_share_of_bound']:.2f} of the bound, w v {e['w_v_against_out']:.2e} ({e['lines']} lines)"
                              for k, e in errs["kinds"].items()) + ".", ""]
        if errs["masked"]["lines"]:
            lines += [f"Masked states ({errs['masked']['lines']} lines): w {errs['masked']['w']:.2e}, row sum {errs['masked']['rowsum_share_of_bound']:.2f} of the bound.", ""]
        if errs["models"]:
            lines += ["`predict(return_attention=True)` against float64 on the model's own head projections, of attn's scale: "
                      + "; ".join(f"{c} {e:.2e}" for c, e in errs["models"].items()) + ".", ""]
    with open(os.path.join(a.out, "INDEX_attention_readout.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "attention_readout", "results": [{k: r[k] for k in ("T", "d", "m", "Nc", "Nq", "plain_us", "read_out_us", "kernel_plain_us",
                                                                                    "kernel_read_out_us", "out_bit_equal")} for r in res]}))


if __name__ == "__main__":
    main()
