"""Wall times of the paged per-shot state on one GPU: keys, query without and with w, against the summary query,
mlhot_favor_fwd on kept keys and - at 256 slots - the long query, at 6c-7's two shapes; leave-one-out at 512 shots against
conditioning again per subset.  Median of 5 wall times per leg, the legs alternating in one process.  Prints one JSON object.

    python scripts/favor_paged_probe.py [--out profiles/favor_paged.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "what-matters-for-meta-learning_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [dict(T=20, H=8, d=256, m=1419), dict(T=10, H=8, d=64, m=266)]
NCS, NQS, REPS = [256, 512, 1024, 2048], [30, 300], 5


def timed(legs):
    """{name: fn} -> {name: median ms of REPS wall times}, one warm-up each, the legs alternating"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(REPS):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def kernels():
    from mlhot import lib
    from mlhot.ops import favor_absorb, favor_keys_long, favor_keys_paged, favor_query
    rows = []
    for s in SHAPES:
        T, H, d, m = s["T"], s["H"], s["d"], s["m"]
        g = torch.Generator().manual_seed(1)
        proj = torch.randn(m, d, generator=g).cuda()
        for Nc in NCS:
            k = (0.25 * torch.randn(T, Nc, H, d, generator=g)).cuda()
            v = torch.randn(T, Nc, H, d, generator=g).cuda()
            paged, summary = favor_keys_paged(k, proj), favor_absorb(None, k, v, proj)
            long = favor_keys_long(k, proj) if Nc <= 256 else None
            for Nq in NQS:
                q = (0.25 * torch.randn(T, Nq, H, d, generator=g)).cuda()
                legs = {"keys_paged": lambda: favor_keys_paged(k, proj), "query_paged": lambda: favor_query(q, paged, v, proj),
                        "query_paged_w": lambda: favor_query(q, paged, v, proj, weights=True),
                        "query_summary": lambda: favor_query(q, summary, None, proj)}
                if long is not None:
                    legs["query_long"] = lambda: favor_query(q, long, v, proj)
                    legs["query_long_w"] = lambda: favor_query(q, long, v, proj, weights=True)
                try:
                    lib().favor_fwd(q, k, v, proj)
                    legs["favor_fwd"] = lambda: lib().favor_fwd(q, k, v, proj)
                except Exception as e:                       # outside that kernel's envelope
                    legs_note = str(e)[:80]
                else:
                    legs_note = None
                row = dict(s, Nc=Nc, Nq=Nq, ms=timed(legs))
                if legs_note:
                    row["favor_fwd"] = legs_note
                rows.append(row)
                print(json.dumps(row), flush=True)
            del paged, summary, long, k, v
            torch.cuda.empty_cache()
    return rows


def leave_one_out(shots=512, Nq=30, T=2):
    from mlhot import cached
    from networks.ANPShapeNet1D import ANPShapeNet1D
    cfg = types.SimpleNamespace(device=torch.device("cuda:0"), seed=2578, img_size=[128, 128, 1], tasks_per_batch=T, input_dim=3, output_dim=2,
                                agg_mode="attention", img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_r=64, dim_z=64, task="shapenet_1d",
                                temperature=0.07)
    model = ANPShapeNet1D(cfg).cuda().eval()
    g = torch.Generator().manual_seed(3)
    cx, cy, qx = (torch.rand(T, shots, 1, 128, 128, generator=g).cuda(), torch.rand(T, shots, 3, generator=g).cuda(),
                  torch.rand(T, Nq, 1, 128, 128, generator=g).cuda())
    state = cached.condition(model, cx, cy, form="paged")
    sx, sy = cx[:, 1:].contiguous(), cy[:, 1:].contiguous()
    ms = timed({"leave_one_out": lambda: cached.leave_one_out(model, state, qx),
                "condition_and_predict_one_subset": lambda: cached.predict(model, cached.condition(model, sx, sy, form="paged"), qx),
                "predict_unmasked": lambda: cached.predict(model, state, qx)})
    row = dict(model="ANPShapeNet1D", T=T, shots=shots, Nq=Nq, ms=ms, per_subset_times_shots_ms=round(ms["condition_and_predict_one_subset"] * shots, 1))
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), reps=REPS, kernels=kernels(), leave_one_out=leave_one_out())
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
