"""What the top-k attention read-out costs against the plain query and against the read-out followed by torch.topk,
on the GPU.

    python scripts/attention_topk_probe.py [--out profiles] [--reps 3]

`mlhot.ops.favor_query` at the ANP shape - T 16, H 8, d 256, m 1419, Nq 300 targets, k 8 - against per-shot key states of 32, 256,
1024 and 4096 slots (forms "keys", "long", "paged", "paged"), three legs:
    topk        favor_query(topk=8): the k heaviest slots per row selected inside the query launch, the paged form in its one walk
    plain       favor_query(): the query of the form alone - yardstick (a), what the selection rides on
    read_out    favor_query(weights=True) followed by torch.topk(w, 8): yardstick (b), the route there was before - w [T, H, Nq, Nc]
                written to memory and read back by torch's selection
The legs alternate in this process after one warm-up of each; a repetition is CALLS calls between two device synchronisations, and
the median of `reps` repetitions is reported per call.  Peak device memory is torch.cuda.max_memory_allocated over one call of the
leg minus what was allocated before it (operands and state excluded).  The library's launch profiler gives the kernels' own medians
in a run of its own, and there the top-k kernel also at k = 1 and k = 16: the selection's rounds grow with k, its page skip does
not, so the three say which part the time goes to.  No ratio is fixed in advance.  out is compared bit for bit, wk with
torch.topk's values bit for bit.
Writes <out>/attention_topk.json and <out>/INDEX_attention_topk.md."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

T, H, D, M, NQ, K = 16, 8, 256, 1419, 300, 8
SLOTS = [(32, "keys"), (256, "long"), (1024, "paged"), (4096, "paged")]
CALLS = 3


def measure(Nc, form, reps):
    import torch
    import mlhot
    from mlhot import ops
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    g = torch.Generator().manual_seed(1)
    q, k, v = (0.25 * torch.randn(T, n, H, D, generator=g).cuda() for n in (NQ, Nc, Nc))
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(M, D).float().cuda()
    state = {"keys": ops.favor_keys, "long": ops.favor_keys_long, "paged": ops.favor_keys_paged}[form](k, proj)
    kk = min(K, Nc)

    def read_out():
        out, w = ops.favor_query(q, state, v, proj, weights=True)
        top = torch.topk(w, kk, dim=-1)
        return out, top.indices, top.values

    legs = {"topk": lambda: ops.favor_query(q, state, v, proj, topk=K), "plain": lambda: ops.favor_query(q, state, v, proj), "read_out": read_out}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / CALLS, r

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = fn()
        torch.cuda.synchronize()
        del r
        return torch.cuda.max_memory_allocated() - before

    def kernels(fns):
        lib.prof_begin(8 * reps * len(fns) + 16)
        for _ in range(reps):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        by = {}
        for label, t in lib.prof_end():
            by.setdefault(label, []).append(t * 1e3)
        return {label: round(statistics.median(ts), 2) for label, ts in by.items()}

    warm = {name: timed(fn)[1] for name, fn in legs.items()}
    us = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            us[name].append(timed(fn)[0])
    mem = {name: peak(fn) for name, fn in legs.items()}
    kern = kernels(list(legs.values()))
    label = {"keys": "favor.querytopk", "long": "favor.lquerytopk", "paged": "favor.pquerytopk"}[form]
    by_k = {str(kx): kernels([lambda kx=kx: ops.favor_query(q, state, v, proj, topk=kx)])[label] for kx in (1, K, 16)}
    med = {name: statistics.median(x) for name, x in us.items()}
    (out_t, idx, wk), out_p, (out_r, _, vals) = warm["topk"], warm["plain"], warm["read_out"]
    return {"T": T, "H": H, "d": D, "m": M, "Nq": NQ, "Nc": Nc, "k": K, "form": form, "reps": reps, "calls_per_rep": CALLS,
            "w_bytes": 4 * T * H * NQ * Nc, "topk_bytes": 8 * T * H * NQ * K,
            "topk_us": round(med["topk"], 1), "plain_us": round(med["plain"], 1), "read_out_topk_us": round(med["read_out"], 1),
            "topk_over_plain": round(med["topk"] / med["plain"], 3), "topk_over_read_out_topk": round(med["topk"] / med["read_out"], 3),
            "topk_peak_bytes": mem["topk"], "plain_peak_bytes": mem["plain"], "read_out_topk_peak_bytes": mem["read_out"],
            "us_all": {name: [round(x, 1) for x in xs] for name, xs in us.items()}, "kernel_us": kern, "topk_kernel_us_by_k": by_k,
            "out_bit_equal": bool(torch.equal(out_t, out_p) and torch.equal(out_t, out_r)),
            "values_bit_equal_torch_topk": bool(torch.equal(wk[..., :kk], vals)),
            "indices_equal_torch_topk": float((idx[..., :kk].long() == warm["read_out"][1]).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(Nc, form, a.reps) for Nc, form in SLOTS]
    with open(os.path.join(a.out, "attention_topk.json"), "w") as f:
        json.dump({"probe": "scripts/attention_topk_probe.py", "results": res}, f, indent=1)
    mib = lambda b: f"{b / 2 ** 20:.1f}"
    lines = ["# Top-k attention read-out (DESIGN.md 6c-15) - the k heaviest context slots per target inside the query launch", "",
             f"`python scripts/attention_topk_probe.py`: `mlhot.ops.favor_query` at T {T}, H {H}, d {D}, m {M}, Nq {NQ}, k {K}; `topk={K}` against (a) the plain "
             f"query of the form and (b) `weights=True` followed by `torch.topk(w, {K})`, the legs alternating in one process after one warm-up of each; a "
             f"repetition is {CALLS} calls between two device synchronisations, median of {a.reps} repetitions, per call (wall: Python and launches included).  "
             "Peak = torch.cuda.max_memory_allocated over one call minus what was allocated before it.  kernels = the launch profiler's medians in a run of "
             "its own; by k = the top-k kernel alone at k 1 / 8 / 16 (the rounds grow with k, the page skip does not).  No ratio was fixed in advance.  "
             "Numbers in `attention_topk.json`.", "",
             "| Nc | form | w MiB | top-k us | plain us | read-out + topk us | vs plain | vs read-out + topk | top-k peak MiB | plain peak MiB | read-out + topk peak MiB "
             "| kernels us | top-k kernel us at k 1 / 8 / 16 | out bit-equal | values = torch.topk | indices = torch.topk |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        kern = ", ".join(f"{k} {v}" for k, v in sorted(r["kernel_us"].items()))
        by_k = " / ".join(str(r["topk_kernel_us_by_k"][k]) for k in ("1", str(K), "16"))
        lines.append(f"| {r['Nc']} | {r['form']} | {mib(r['w_bytes'])} | {r['topk_us']} | {r['plain_us']} | {r['read_out_topk_us']} | {r['topk_over_plain']} | "
                     f"{r['topk_over_read_out_topk']} | {mib(r['topk_peak_bytes'])} | {mib(r['plain_peak_bytes'])} | {mib(r['read_out_topk_peak_bytes'])} | {kern} | "
                     f"{by_k} | {r['out_bit_equal']} | {r['values_bit_equal_torch_topk']} | {r['indices_equal_torch_topk']:.6f} |")
    lines.append("")
    with open(os.path.join(a.out, "INDEX_attention_topk.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "attention_topk", "results": [{k: r[k] for k in ("Nc", "form", "topk_us", "plain_us", "read_out_topk_us", "topk_over_plain",
                                                                                "topk_over_read_out_topk", "topk_peak_bytes", "read_out_topk_peak_bytes",
                                                                                "topk_kernel_us_by_k", "out_bit_equal", "values_bit_equal_torch_topk")} for r in res]}))


if __name__ == "__main__":
    main()
