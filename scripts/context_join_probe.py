"""Joined cached contexts, measured.  One process, the legs alternating, the median of 5 per leg:
  * leg A: mlhot.cached.concat of two states against conditioning again on all their shots - the only route there was - at 16 + 16
    ("keys"), 128 + 128 ("long") and 512 + 512 ("paged") shots, at the ANP shape (T 20, 64 x 64 x 3) and the vanilla shape (T 10,
    128 x 128 x 1): wall, device and host time;
  * leg B: mlhot_rows_gather alone at [T 20][cap 4096][W 2048] from 8 sources against torch.clone of the same bytes and
    mlhot_rows_compact on the same bytes: bytes moved per second - with ONE row set of W 2048, and with TWO of W 1024 each (the
    kernel every attention concat launches: kh and vh).
Writes profiles/context_join.json (or --out).  Usage: python scripts/context_join_probe.py [--out FILE] [--quick]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "what-matters-for-meta-learning_amd"), ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from context_window_probe import DEV, legs, model_for, SHAPES  # noqa: E402

JOINS = ((16, "keys"), (128, "long"), (512, "paged"))            # shots per state; the result holds twice as many


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_join.json"))
    ap.add_argument("--quick", action="store_true", help="16 + 16 only, and the kernel leg")
    args = ap.parse_args()
    import mlhot
    from mlhot import cached
    res = {"device": torch.cuda.get_device_name(0), "concat": [], "rows_gather": {}, "rows_gather_two_sets": {}}
    g = torch.Generator().manual_seed(3)
    for name in SHAPES:
        model, T, img, L = model_for(name)
        for n, form in JOINS[:1] if args.quick else JOINS:
            cx, cy = torch.rand(T, 2 * n, *img, generator=g).to(DEV), torch.rand(T, 2 * n, L, generator=g).to(DEV)
            a = cached.condition(model, cx[:, :n].contiguous(), cy[:, :n].contiguous(), form=form)
            b = cached.condition(model, cx[:, n:].contiguous(), cy[:, n:].contiguous(), form=form)
            r = legs({"concat": lambda: cached.concat(model, [a, b], form=form), "condition": lambda: cached.condition(model, cx, cy, form=form)})
            res["concat"].append(dict(shape=name, T=T, shots=f"{n} + {n}", form=form, **{f"{k}_{m}": v for k, d in r.items() for m, v in d.items()}))
            print(res["concat"][-1], flush=True)
            del a, b
        del model
    T, cap, nsrc = 20, 4096, 8
    per = cap // nsrc
    s = torch.arange(cap)
    t = torch.arange(T)
    plan = torch.stack([(s // per)[None, :].expand(T, -1), t[:, None] * per + (s % per)[None, :]], dim=-1).to(torch.int32).contiguous().to(DEV)
    keep = torch.arange(cap, dtype=torch.int32).repeat(T, 1).to(DEV)
    for key, widths in (("rows_gather", (2048,)), ("rows_gather_two_sets", (1024, 1024))):
        srcs = [[torch.randn(T, per, W, device=DEV) for W in widths] for _ in range(nsrc)]
        whole = [torch.cat([src[i] for src in srcs], dim=1) for i in range(len(widths))]      # the same bytes in one buffer per set
        got = mlhot.lib().rows_gather(srcs, plan, T, cap)
        assert all(torch.equal(a, b) for a, b in zip(got, whole))
        del got
        r = legs({"rows_gather": lambda: mlhot.lib().rows_gather(srcs, plan, T, cap), "rows_compact": lambda: mlhot.lib().rows_compact(whole, keep),
                  "clone": lambda: [x.clone() for x in whole]})
        moved = 2 * sum(x.numel() for x in whole) * 4
        res[key] = dict(T=T, cap=cap, W=list(widths), nsrc=nsrc, bytes_moved=moved,
                        **{f"{k}_{m}": v for k, d in r.items() for m, v in (("device_ms", d["device_ms"]), ("GBps", round(moved / d["device_ms"] / 1e6, 1)))},
                        gather_of_clone=round(r["clone"]["device_ms"] / r["rows_gather"]["device_ms"], 3),
                        gather_of_compact=round(r["rows_compact"]["device_ms"] / r["rows_gather"]["device_ms"], 3),
                        note="device_ms includes the outputs' allocation; clone is torch's copy of the same bytes, measured alike")
        print(key, res[key], flush=True)
        del srcs, whole
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
