"""FAVOR+ forward + backward above 32 shots: the linear form (option "favor_linear") against favor.h's chain, on the GPU.

    python scripts/favor_linear_probe.py [--out profiles] [--reps 5] [--step-timeout 300]

Shapes (T 20, H 8, d 256, m 1419) and (T 10, H 8, d 64, m 266); shot counts Nq = Nc in {33, 64, 128, 256} and Nq 30 with Nc in
{64, 256}; random inputs on the device.  One leg = mlhot_favor_fwd then mlhot_favor_bwd on the forward's workspace, with the option off
(the chain: the only route these shapes had before) and on.  Per shape family ONE process runs every size: the two legs alternate,
each between device synchronisations, after one warm-up of each; the median of `reps` wall times is reported, and for one size
(Nq = Nc = 128) the per-label times of mlhot_prof_*.  A third step runs both routes over tests/favor_linear_cases.py and records the
worst U.rel_err per tensor against float64.  This driver never touches the GPU: every step is a child process under its own
`timeout`, and the first step that fails ends the run.  Writes <out>/favor_linear.json and <out>/INDEX_favor_linear.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

SHAPES = [dict(T=20, H=8, d=256, m=1419), dict(T=10, H=8, d=64, m=266)]
SIZES = [(33, 33), (64, 64), (128, 128), (256, 256), (30, 64), (30, 256)]        # (Nq, Nc)
PROF_SIZE = (128, 128)
LEGS = (("chain", 0), ("linear", 1))


def step_time(shape, reps):
    import torch
    import mlhot
    from oracle import ref_cpu as O
    lib = mlhot.lib()
    T, H, d, m = (shape[k] for k in "THdm")
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(77)
    proj = O.gaussian_orthogonal_random_matrix(m, d).float().cuda()

    def leg(option, ops):
        q, k, v, dout = ops
        lib.set_option("favor_linear", option)
        try:
            out, ws = lib.favor_fwd(q, k, v, proj)
            return (out,) + tuple(lib.favor_bwd(q, k, v, proj, out, dout, ws))
        finally:
            lib.set_option("favor_linear", 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    rows = []
    for Nq, Nc in SIZES:
        ops = ((d ** -0.25 * torch.randn(T, Nq, H, d, generator=g)).cuda(), (d ** -0.25 * torch.randn(T, Nc, H, d, generator=g)).cuda(),
               torch.randn(T, Nc, H, d, generator=g).cuda(), torch.randn(T, Nq, d * H, generator=g).cuda())
        warm = {name: timed(lambda o=o: leg(o, ops))[1] for name, o in LEGS}
        diff = {n: ((a - b).abs().max() / b.abs().max()).item() for n, a, b in zip(("out", "dq", "dk", "dv"), warm["linear"], warm["chain"])}
        # dk once more without THE arg-max key row: that row alone takes the batch-wide sum of G_k (the stabiliser's gradient), a sum of
        # T Nc H m terms that cancels almost entirely and that each route rounds in its own way
        top = int(torch.einsum("tnhd,md->tnhm", ops[1], proj).flatten(2).max(dim=2).values.argmax())       # (t, n) of the batch maximum
        keep = torch.ones(T * Nc, dtype=torch.bool, device="cuda")
        keep[top] = False
        a, b = (x.reshape(T * Nc, H * d)[keep] for x in (warm["linear"][2], warm["chain"][2]))
        diff["dk_without_argmax_shot"] = ((a - b).abs().max() / b.abs().max()).item()
        ms = {name: [] for name, _ in LEGS}
        for _ in range(reps):
            for name, o in LEGS:
                ms[name].append(timed(lambda o=o: leg(o, ops))[0])
        row = {"Nq": Nq, "Nc": Nc, "ms": {n: round(statistics.median(x), 4) for n, x in ms.items()}, "ms_all": {n: [round(y, 4) for y in x] for n, x in ms.items()},
               "linear_against_chain_of_own_scale": diff}
        if (Nq, Nc) == PROF_SIZE:
            row["labels_ms"] = {}
            for name, o in LEGS:
                lib.prof_begin(256)
                try:
                    leg(o, ops)
                finally:
                    recs = lib.prof_end()
                row["labels_ms"][name] = [[label, round(t, 4)] for label, t in recs]
        rows.append(row)
        del ops, warm
    return dict(shape, reps=reps, rows=rows)


def step_errors():
    import torch
    import mlhot
    from tests import favor_linear_cases as LC
    from tests import util as U
    lib = mlhot.lib()
    worst = {name: {n: [0.0, None] for n in LC.NAMES} for name, _ in LEGS}
    per_case = []
    for c in LC.CASES:
        qn, kn, vn, dout, proj = (t.cuda() for t in LC.kernel_layout(LC.inputs(c.name)))
        ref = LC.reference(c, torch.float64)
        floor = LC.floors(c, ref)
        rec = {"case": c.name}
        for name, o in LEGS:
            lib.set_option("favor_linear", o)
            try:
                out, ws = lib.favor_fwd(qn, kn, vn, proj)
                dq, dk, dv = lib.favor_bwd(qn, kn, vn, proj, out, dout, ws)
                torch.cuda.synchronize()
            finally:
                lib.set_option("favor_linear", 0)
            got = LC.reference_layout(c, *(t.cpu() for t in (out, dq, dk, dv)))
            rec[name] = {n: U.rel_err(got[n], ref[n], floor[n]) for n in LC.NAMES}
            for n in LC.NAMES:
                if rec[name][n] > worst[name][n][0]:
                    worst[name][n] = [rec[name][n], c.name]
        per_case.append(rec)
    return {"worst": worst, "per_case": per_case}


def run_steps(reps, step_timeout):
    """Every GPU step as a child under `timeout`; the first failure ends the run (nothing more is started on the device)."""
    results = {}
    steps = [f"time{i}" for i in range(len(SHAPES))] + ["errors"]
    with tempfile.TemporaryDirectory() as tmp:
        for step in steps:
            path = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(reps), "--step-out", path]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit(f"favor_linear_probe: step {step} ended with status {rc}; nothing further was started")
            with open(path) as f:
                results[step] = json.load(f)
            print(f"favor_linear_probe: step {step} done", flush=True)
    return results


def label_table(row):
    lines = []
    for name, _ in LEGS:
        total = {}
        for label, t in row["labels_ms"][name]:
            total[label] = total.get(label, 0.0) + t
        lines.append(f"- {name}, Nq {row['Nq']} Nc {row['Nc']} ({sum(total.values()):.3f} ms of device time in {len(row['labels_ms'][name])} launches): "
                     + ", ".join(f"`{k}` {v:.3f}" for k, v in total.items()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", default=None, help="internal: run one GPU step in this process")
    ap.add_argument("--step-out", default=None)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    if a.step:
        res = step_errors() if a.step == "errors" else step_time(SHAPES[int(a.step[4:])], a.reps)
        with open(a.step_out, "w") as f:
            json.dump(res, f)
        return
    os.makedirs(a.out, exist_ok=True)
    r = run_steps(a.reps, a.step_timeout)
    res, errs = [r[f"time{i}"] for i in range(len(SHAPES))], r["errors"]
    with open(os.path.join(a.out, "favor_linear.json"), "w") as f:
        json.dump({"probe": "scripts/favor_linear_probe.py", "results": res, "errors_against_float64": errs}, f, indent=1)
    lines = ["# FAVOR+ forward + backward above 32 shots: linear form (option `favor_linear`, DESIGN.md 6d) against the chain", "",
             f"`python scripts/favor_linear_probe.py`: median of {a.reps} wall times in ms of `mlhot_favor_fwd` + `mlhot_favor_bwd`, the two legs (option off = "
             "`favor.h`'s chain, the route these shapes took before; option on = `favor_linear.h`) alternating in one process per shape family between "
             "device synchronisations, after one warm-up of each.  Every size is listed, also where the linear route loses.  Numbers in `favor_linear.json`.", ""]
    for s in res:
        lines += [f"## T {s['T']}, H {s['H']}, d {s['d']}, m {s['m']}", "", "| Nq | Nc | chain | linear | chain / linear |", "|---|---|---|---|---|"]
        for row in s["rows"]:
            x = row["ms"]
            lines.append(f"| {row['Nq']} | {row['Nc']} | {x['chain']:.3f} | {x['linear']:.3f} | {x['chain'] / x['linear']:.2f} |")
        lines += ["", "Largest difference between the two routes' results, of each tensor's own scale: "
                  + ", ".join(f"{n} {max(row['linear_against_chain_of_own_scale'][n] for row in s['rows']):.1e}" for n in ("out", "dq", "dk", "dv"))
                  + f"; dk without the shot that holds the batch-wide key maximum (it alone takes the stabiliser's gradient, a cancelling sum of T Nc H m terms): "
                  f"{max(row['linear_against_chain_of_own_scale']['dk_without_argmax_shot'] for row in s['rows']):.1e}.", "",
                  "Device time per launch label (`mlhot_prof_*`, one pass each):", ""]
        lines += label_table(next(row for row in s["rows"] if "labels_ms" in row)) + [""]
    lines += ["## Worst error against float64 over tests/favor_linear_cases.py", "",
              "`U.rel_err` per tensor (dead tensors at dv's scale), worst case in brackets:", ""]
    for name, _ in LEGS:
        lines.append(f"- {name}: " + ", ".join(f"{n} {e:.2e} ({c})" for n, (e, c) in errs["worst"][name].items()))
    with open(os.path.join(a.out, "INDEX_favor_linear.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"probe": "favor_linear", "results": [{"shape": [s[k] for k in "THdm"], "rows": [{"Nq": row["Nq"], "Nc": row["Nc"], **row["ms"]} for row in s["rows"]]}
                                                           for s in res], "worst_errors": errs["worst"]}))


if __name__ == "__main__":
    main()
