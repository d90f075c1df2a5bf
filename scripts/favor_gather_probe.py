"""Picking and combining tasks across FAVOR+ summary states against its yardsticks, on the GPU.

    python scripts/favor_gather_probe.py [--out profiles] [--reps 5]

Shapes (T 20, H 8, d 256, m 1419) and (T 10, H 8, d 64, m 266) - 6c-6's; random inputs on the device.  6c-6's protocol: the legs
alternate in this process, each between device synchronisations, after one warm-up of each; the median of `reps` wall times is reported:
  merge_2 / _8         favor_merge of that many 32-shot states: the yardstick, ONE launch that reads n states and writes one;
  gather_id_2 / _8     mlhot_favor_summary_gather with the identity table over the same states, the table already on the device: the
                       same bytes, the same sums, the same bits;
  op_id_2 / _8         mlhot.ops.favor_gather of the same: the host checks, the table's upload and the launch;
  gather_perm          a permutation of ONE state (P = 1): reads one state, writes one;
  gather_2_of_8        two parts per task from 8 states (task t = (t % 8, t) + ((t + 1) % 8, (t + 1) % T)): reads two states' worth;
  recondition          mlhot.cached.condition(form="summary") of the same T tasks from their images, 32 shots each - the cost the
                       feature removes (the ResNet ANP at d 256, ANPShapeNet1D at d 64).
Beside every gather and merge: the bytes the launch must move and bytes / time, also as a share of the MI355X's 8 TB/s HBM peak, and
gather over merge for the identity table.  The wall times include the launch and the synchronisation.
Writes <out>/favor_gather.json and <out>/INDEX_favor_gather.md."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

SHAPES = [dict(T=20, H=8, d=256, m=1419), dict(T=10, H=8, d=64, m=266)]
NS = (2, 8)
HBM_PEAK = 8.0e12          # bytes / s
MODELS = {
    256: ("ANP", dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
                      agg_mode="attention"), (3, 64, 64), 4),
    64: ("ANPShapeNet1D", dict(seed=2578, img_size=[128, 128, 1], input_dim=3, output_dim=2, agg_mode="attention", img_agg="", dim_w=64,
                               n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d"), (1, 128, 128), 3),
}


def measure(shape, reps):
    import torch
    import mlhot
    from mlhot import cached
    from mlhot.ops import favor_absorb, favor_gather, favor_merge
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    T, H, d, m = (shape[k] for k in "THdm")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()
    states = [favor_absorb(None, 0.25 * torch.randn(T, 32, H, d, generator=g).cuda(), torch.randn(T, 32, H, d, generator=g).cuda(), proj) for _ in range(8)]
    table = lambda rows: torch.tensor(rows, dtype=torch.int32).cuda()
    ident = {n: [[(i, t) for i in range(n)] for t in range(T)] for n in NS}
    perm = [[(0, (t + 1) % T)] for t in range(T)]
    two = [[(t % 8, t), ((t + 1) % 8, (t + 1) % T)] for t in range(T)]
    dev = {**{f"id_{n}": table(ident[n]) for n in NS}, "perm": table(perm), "two": table(two)}
    raw = lambda n, tab: lib.favor_summary_gather([s.buf for s in states[:n]], [T] * n, tab, H, d, m)
    method, cfg, img, L = MODELS[d]
    model = getattr(importlib.import_module("networks." + method), method)(
        types.SimpleNamespace(device=torch.device("cuda:0"), tasks_per_batch=T, **cfg)).cuda().eval()
    assert tuple(model.attn.projection_matrix.shape) == (m, d)
    cx, cy = torch.rand(T, 32, *img, generator=g).cuda(), torch.rand(T, 32, L, generator=g).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    legs = {}
    for n in NS:
        legs[f"merge_{n}"] = lambda n=n: favor_merge(states[:n])
        legs[f"gather_id_{n}"] = lambda n=n: raw(n, dev[f"id_{n}"])
        legs[f"op_id_{n}"] = lambda n=n: favor_gather(states[:n], ident[n])
    legs["gather_perm"] = lambda: raw(1, dev["perm"])
    legs["gather_2_of_8"] = lambda: raw(8, dev["two"])
    legs["recondition"] = lambda: cached.condition(model, cx, cy, form="summary")
    warm = {name: timed(f)[1] for name, f in legs.items()}
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, f in legs.items():
            ms[name].append(timed(f)[0])
    med = {n: statistics.median(x) for n, x in ms.items()}
    nb = lib.favor_summary_bytes(T, H, d, m)
    moved = {"gather_perm": 2 * nb, "gather_2_of_8": 3 * nb}
    for n in NS:
        moved.update({f"merge_{n}": (n + 1) * nb, f"gather_id_{n}": (n + 1) * nb, f"op_id_{n}": (n + 1) * nb})
    rate = {n: moved[n] / (med[n] * 1e-3) for n in moved}
    same = {n: bool(torch.equal(warm[f"gather_id_{n}"].view(torch.int32), warm[f"merge_{n}"].buf.view(torch.int32))) for n in NS}
    return dict(shape, reps=reps, state_bytes=nb, ms={n: round(x, 4) for n, x in med.items()}, ms_all={n: [round(y, 4) for y in x] for n, x in ms.items()},
                bytes_moved=moved, bytes_per_s={n: round(x, 0) for n, x in rate.items()}, share_of_hbm_peak={n: round(x / HBM_PEAK, 4) for n, x in rate.items()},
                gather_over_merge={str(n): round(med[f"gather_id_{n}"] / med[f"merge_{n}"], 4) for n in NS},
                identity_bits_equal_merge={str(n): same[n] for n in NS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    os.makedirs(a.out, exist_ok=True)
    res = [measure(s, a.reps) for s in SHAPES]
    with open(os.path.join(a.out, "favor_gather.json"), "w") as f:
        json.dump({"probe": "scripts/favor_gather_probe.py", "hbm_peak_bytes_per_s": HBM_PEAK, "results": res}, f, indent=1)
    lines = ["# Picking and combining tasks across FAVOR+ summary states (DESIGN.md 6c-8)", "",
             f"`python scripts/favor_gather_probe.py`: median of {a.reps} wall times per leg in ms, the legs alternating in one process between device "
             "synchronisations after one warm-up of each (6c-6's protocol).  merge n = `favor_merge` of n 32-shot states; gather id n = "
             "`mlhot_favor_summary_gather` with the identity table over the same states, the table already on the device - the same bytes and the same "
             "bits; op id n = `mlhot.ops.favor_gather` of the same, with the host checks and the table's upload.  Bytes = what the launch must move; "
             "GB/s = bytes / wall time, launch and synchronisation included, and its share of the 8 TB/s HBM peak.  Numbers in `favor_gather.json`.", ""]
    names = {"gather_perm": "gather, a permutation of one state (P = 1)", "gather_2_of_8": "gather, two parts per task from 8 states (P = 2)"}
    for r in res:
        x, mv, bw, sh = r["ms"], r["bytes_moved"], r["bytes_per_s"], r["share_of_hbm_peak"]
        lines += [f"## T {r['T']}, H {r['H']}, d {r['d']}, m {r['m']}", "", f"State: {r['state_bytes']} bytes.", "",
                  "| leg | ms | MB moved | GB/s | of HBM peak |", "|---|---|---|---|---|"]
        for n in [f"{k}_{i}" for i in NS for k in ("merge", "gather_id", "op_id")] + ["gather_perm", "gather_2_of_8"]:
            lines.append(f"| {names.get(n, n.replace('_', ' '))} | {x[n]:.3f} | {mv[n] / 1e6:.1f} | {bw[n] / 1e9:.0f} | {100 * sh[n]:.1f} % |")
        lines += ["", "Gather over merge, identity table: " + ", ".join(f"n = {n}: {r['gather_over_merge'][str(n)]:.3f}" for n in NS)
                  + "; bits equal to merge's: " + ", ".join(f"n = {n}: {r['identity_bits_equal_merge'][str(n)]}" for n in NS) + ".", "",
                  f"Re-conditioning the same {r['T']} tasks from their images (32 shots each, `condition(form=\"summary\")`): {x['recondition']:.3f} ms - "
                  f"{x['recondition'] / x['gather_perm']:.0f} x the permutation, {x['recondition'] / x['gather_2_of_8']:.0f} x the two-part gather.", ""]
    with open(os.path.join(a.out, "INDEX_favor_gather.md"), "w") as f:
        f.write("\n".join(lines))
    print(json.dumps({"probe": "favor_gather", "results": [{"shape": [r[k] for k in "THdm"], "state_bytes": r["state_bytes"], **r["ms"],
                                                            "gather_over_merge": r["gather_over_merge"]} for r in res]}))


if __name__ == "__main__":
    main()
