"""What the attention mass costs against the read-out summed afterwards, on the GPU.

    python scripts/attention_mass_probe.py [--out profiles] [--reps 5]

`mlhot.ops.favor_query` at the ANP shape - T 16, H 8, d 256, m 1419, Nq 300 targets - against per-shot key states of 32, 256, 1024 and
4096 slots (forms "keys", "long", "paged", "paged"), two legs:
    mass        favor_query(mass=True): the column sums of w = S / D formed inside the query launch, the tile partials folded
    read_out    favor_query(weights=True) followed by w.sum(2): the route there was before - w [T, H, Nq, Nc] written to memory and
                read back by torch's reduction
The legs alternate in this process after one warm-up of each; a repetition is CALLS calls between two device synchronisations, and
the median of `reps` repetitions is reported per call.  Peak device memory is torch.cuda.max_memory_allocated over one call of the
leg minus what was allocated before it (operands and state excluded).  The library's launch profiler gives the kernels' own medians
in a run of its own.  No ratio is fixed in advance.  The two legs' masses are compared (the orders differ: torch's reduction is
not the documented fold) and out bit for bit.
Writes <out>/attention_mass.json and <out>/INDEX_attention_mass.md."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

T, H, D, M, NQ = 16, 8, 256, 1419, 300
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
    legs = {"mass": lambda: ops.favor_query(q, state, v, proj, mass=True),
            "read_out": lambda: (lambda out, w: (out, w.sum(2)))(*ops.favor_query(q, state, v, proj, weights=True))}

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

    warm = {name: timed(fn)[1] for name, fn in legs.items()}
    us = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            us[name].append(timed(fn)[0])
    mem = {name: peak(fn) for name, fn in legs.items()}
    lib.prof_begin(8 * reps * len(legs) + 16)
    for _ in range(reps):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    by = {}
    for label, t in lib.prof_end():
        by.setdefault(label, []).append(t * 1e3)
    med = {name: statistics.median(x) for name, x in us.items()}
    kern = {label: round(statistics.median(ts), 2) for label, ts in by.items()}
    (out_m, mass), (out_r, summed) = warm["mass"], warm["read_out"]
    return {"T": T, "H": H, "d": D, "m": M, "Nq": NQ, "Nc": Nc, "form": form, "reps": reps, "calls_per_rep": CALLS,
            "w_bytes": 4 * T * H * NQ * Nc, "partials_bytes": lib.favor_query_mass_bytes(T, H, NQ, Nc, D, M),
            "mass_us": round(med["mass"], 1), "read_out_sum_us": round(med["read_out"], 1), "mass_over_read_out_sum": round(med["mass"] / med["read_out"], 3),
            "mass_peak_bytes": mem["mass"], "read_out_sum_peak_bytes": mem["read_out"],
            "us_all": {name: [round(x, 1) for x in xs] for name, xs in us.items()}, "kernel_us": kern,
            "out_bit_equal": bool(torch.equal(out_m, out_r)),
            "mass_against_torch_sum": float(((mass.double() - summed.double()).abs() / summed.double().clamp_min(1e-30)).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(Nc, form, a.reps) for Nc, form in SLOTS]
    with open(os.path.join(a.out, "attention_mass.json"), "w") as f:
        json.dump({"probe": "scripts/attention_mass_probe.py", "results": res}, f, indent=1)
    mib = lambda b: f"{b / 2 ** 20:.1f}"
    lines = ["# Attention mass (DESIGN.md 6c-14) - the read-out reduced over the targets inside the query launch", "",
             f"`python scripts/attention_mass_probe.py`: `mlhot.ops.favor_query` at T {T}, H {H}, d {D}, m {M}, Nq {NQ}; `mass=True` against `weights=True` followed "
             f"by `w.sum(2)`, the legs alternating in one process after one warm-up of each; a repetition is {CALLS} calls between two device synchronisations, "
             f"median of {a.reps} repetitions, per call (wall: Python and launches included).  Peak = torch.cuda.max_memory_allocated over one call minus what "
             "was allocated before it.  kernels = the launch profiler's medians in a run of its own.  No ratio was fixed in advance.  Numbers in "
             "`attention_mass.json`.", "",
             "| Nc | form | w MiB | partials MiB | mass us | read-out + sum us | ratio | mass peak MiB | read-out + sum peak MiB | kernels us | out bit-equal | mass vs torch sum |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        kern = ", ".join(f"{k} {v}" for k, v in sorted(r["kernel_us"].items()))
        lines.append(f"| {r['Nc']} | {r['form']} | {mib(r['w_bytes'])} | {mib(r['partials_bytes'])} | {r['mass_us']} | {r['read_out_sum_us']} | "
                     f"{r['mass_over_read_out_sum']} | {mib(r['mass_peak_bytes'])} | {mib(r['read_out_sum_peak_bytes'])} | {kern} | {r['out_bit_equal']} | "
                     f"{r['mass_against_torch_sum']:.1e} |")
    lines.append("")
    with open(os.path.join(a.out, "INDEX_attention_mass.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "attention_mass", "results": [{k: r[k] for k in ("Nc", "form", "mass_us", "read_out_sum_us", "mass_over_read_out_sum",
                                                                                "mass_peak_bytes", "read_out_sum_peak_bytes", "out_bit_equal")} for r in res]}))


if __name__ == "__main__":
    main()
