"""Merging FAVOR+ summary states against its yardsticks, on the GPU.

    python scripts/favor_merge_probe.py [--out profiles] [--reps 5]

Shapes (T 20, H 8, d 256, m 1419) and (T 10, H 8, d 64, m 266) - 6c-4's; random inputs on the device.  Legs, alternating in this process,
each between device synchronisations, after one warm-up of each; the median of `reps` wall times is reported:
  merge_2 / _4 / _8   favor_merge of that many 32-shot states: ONE launch that reads n states and writes one;
  absorb_one          favor_absorb(state, one more shot) into a NEW state - it also rewrites A once (reads one state, writes one): the yardstick;
  chain_256           a 256-shot context as ONE absorb chain (favor_absorb of all 256 shots: eight kernel calls, each rewriting A);
  halves_absorb       the two 128-shot halves, each its own chain (what two sources or two streams do on their own);
  halves_merge        favor_merge of the two finished halves;
  halves_total        both halves and the merge, one after the other on one stream.
Beside every merge and the one-shot absorb: the bytes the launch must move ((n + 1) x the state) and bytes / time, also as a share of
the MI355X's 8 TB/s HBM peak.  The wall times include the launch and the synchronisation, so a small state's figure is a floor on the
kernel's own rate.  Also: the merged 2 x 128 state against the 256-shot chain (A, a of their scales; M equal).
Writes <out>/favor_merge.json and <out>/INDEX_favor_merge.md."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

SHAPES = [dict(T=20, H=8, d=256, m=1419), dict(T=10, H=8, d=64, m=266)]
NS = (2, 4, 8)
HBM_PEAK = 8.0e12          # bytes / s


def measure(shape, reps):
    import torch
    import mlhot
    from mlhot.ops import favor_absorb, favor_merge
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    T, H, d, m = (shape[k] for k in "THdm")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()
    k_all, v_all = (s * torch.randn(T, 257, H, d, generator=g).cuda() for s in (0.25, 1.0))
    k, v = k_all[:, :256].contiguous(), v_all[:, :256].contiguous()
    k1, v1 = k_all[:, 256:].contiguous(), v_all[:, 256:].contiguous()
    halves = [(k[:, :128].contiguous(), v[:, :128].contiguous()), (k[:, 128:].contiguous(), v[:, 128:].contiguous())]
    parts = [favor_absorb(None, k[:, 32 * i:32 * i + 32].contiguous(), v[:, 32 * i:32 * i + 32].contiguous(), proj) for i in range(8)]
    half_states = [favor_absorb(None, hk, hv, proj) for hk, hv in halves]
    whole = favor_absorb(None, k, v, proj)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    legs = {f"merge_{n}": (lambda n=n: favor_merge(parts[:n])) for n in NS}
    legs["absorb_one"] = lambda: favor_absorb(whole, k1, v1, proj)
    legs["chain_256"] = lambda: favor_absorb(None, k, v, proj)
    legs["halves_absorb"] = lambda: [favor_absorb(None, hk, hv, proj) for hk, hv in halves]
    legs["halves_merge"] = lambda: favor_merge(half_states)
    legs["halves_total"] = lambda: favor_merge([favor_absorb(None, hk, hv, proj) for hk, hv in halves])
    warm = {name: timed(f)[1] for name, f in legs.items()}
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, f in legs.items():
            ms[name].append(timed(f)[0])
    med = {n: statistics.median(x) for n, x in ms.items()}
    nb = lib.favor_summary_bytes(T, H, d, m)
    moved = {f"merge_{n}": (n + 1) * nb for n in NS}
    moved.update({"absorb_one": 2 * nb, "halves_merge": 3 * nb})
    rate = {n: moved[n] / (med[n] * 1e-3) for n in moved}
    A, a, vs, cnt, M = warm["halves_total"].summary()
    Aw, aw, vsw, cntw, Mw = whole.summary()
    agree = {"A": ((A - Aw).abs().max() / Aw.abs().max()).item(), "a": ((a - aw).abs().max() / aw.abs().max()).item(),
             "vs": ((vs - vsw).abs().max() / vsw.abs().max()).item(), "M_equal": bool(M.item() == Mw.item()), "cnt_equal": bool(torch.equal(cnt, cntw))}
    return dict(shape, reps=reps, state_bytes=nb, ms={n: round(x, 4) for n, x in med.items()}, ms_all={n: [round(y, 4) for y in x] for n, x in ms.items()},
                bytes_moved=moved, bytes_per_s={n: round(x, 0) for n, x in rate.items()}, share_of_hbm_peak={n: round(x / HBM_PEAK, 4) for n, x in rate.items()},
                merged_halves_against_chain=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(s, a.reps) for s in SHAPES]
    with open(os.path.join(a.out, "favor_merge.json"), "w") as f:
        json.dump({"probe": "scripts/favor_merge_probe.py", "hbm_peak_bytes_per_s": HBM_PEAK, "results": res}, f, indent=1)
    lines = ["# Merging FAVOR+ summary states (DESIGN.md 6c-6)", "",
             f"`python scripts/favor_merge_probe.py`: median of {a.reps} wall times per leg in ms, the legs alternating in one process between device "
             "synchronisations after one warm-up of each.  merge n = `favor_merge` of n 32-shot states, one launch; +1 shot = `favor_absorb` of one more "
             "shot into a NEW state, which also rewrites A once - the yardstick.  Bytes = what the launch must move, (n + 1) x the state (2 x for the "
             "absorb); GB/s = bytes / wall time, launch and synchronisation included, and its share of the 8 TB/s HBM peak.  Numbers in "
             "`favor_merge.json`.", ""]
    for r in res:
        x, mv, bw, sh = r["ms"], r["bytes_moved"], r["bytes_per_s"], r["share_of_hbm_peak"]
        lines += [f"## T {r['T']}, H {r['H']}, d {r['d']}, m {r['m']}", "", f"State: {r['state_bytes']} bytes.", "",
                  "| leg | ms | MB moved | GB/s | of HBM peak |", "|---|---|---|---|---|"]
        for n in [f"merge_{k}" for k in NS] + ["absorb_one"]:
            lines.append(f"| {n.replace('_', ' ').replace('absorb one', '+1 shot (favor_absorb, new state)')} | {x[n]:.3f} | {mv[n] / 1e6:.1f} | {bw[n] / 1e9:.0f} | {100 * sh[n]:.1f} % |")
        ag = r["merged_halves_against_chain"]
        lines += ["", "A 256-shot context:", "", "| route | ms |", "|---|---|",
                  f"| one absorb chain of 256 shots (8 kernel calls) | {x['chain_256']:.3f} |",
                  f"| the two 128-shot halves, each its own chain, one after the other | {x['halves_absorb']:.3f} |",
                  f"| `favor_merge` of the two finished halves ({mv['halves_merge'] / 1e6:.1f} MB, {bw['halves_merge'] / 1e9:.0f} GB/s) | {x['halves_merge']:.3f} |",
                  f"| both halves and the merge on one stream | {x['halves_total']:.3f} |", "",
                  f"The merged halves against the chain: A {ag['A']:.1e}, a {ag['a']:.1e}, vs {ag['vs']:.1e} of their scales; M equal: {ag['M_equal']}; cnt equal: {ag['cnt_equal']}.", ""]
    with open(os.path.join(a.out, "INDEX_favor_merge.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "favor_merge", "results": [{"shape": [r[k] for k in "THdm"], "state_bytes": r["state_bytes"], **r["ms"]} for r in res]}))


if __name__ == "__main__":
    main()
