"""Per launch label medians (mlhot_prof_begin / mlhot_prof_end) of every entry built from csrc/favor_tile.h, for the library in
MLHOT_LIB: 30 repetitions after 3 warm-ups per entry.  Run it once per library, alternating, each in a fresh process:

    MLHOT_LIB=<a libmlhot.so> python scripts/favor_tile_time.py OUT.json

profiles/INDEX_favor_tiles.md says how the legs are compared."""
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
REPS = 30


def main():
    import torch
    import mlhot
    from mlhot.ops import favor_absorb, favor_keys, favor_prefixes_long, favor_query
    from oracle import ref_cpu as O
    from tests import test_cached_vanilla_gpu as CV
    from tests import test_prefix_vanilla_gpu as PV
    lib = mlhot.lib()
    out = {}

    def timed(tag, fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per = {}
        for _ in range(REPS):
            lib.prof_begin(4096)
            fn()
            torch.cuda.synchronize()
            acc = {}
            for label, ms in lib.prof_end():
                acc[label] = acc.get(label, 0.0) + ms
            for label, ms in acc.items():
                per.setdefault(label, []).append(ms)
        for label, xs in per.items():
            xs.sort()
            out[f"{tag}:{label}"] = {"median_ms": statistics.median(xs), "p10_ms": xs[len(xs) // 10], "p90_ms": xs[len(xs) * 9 // 10]}

    for T, H, d, m in ((20, 8, 256, 1419), (10, 8, 64, 266)):
        g = torch.Generator().manual_seed(1)
        with torch.random.fork_rng():
            torch.manual_seed(3)
            proj = O.gaussian_orthogonal_random_matrix(m, d).float().to(DEV)
        q = (0.25 * torch.randn(T, 300, H, d, generator=g)).to(DEV)
        k = (0.25 * torch.randn(T, 128, H, d, generator=g)).to(DEV)
        v = torch.randn(T, 128, H, d, generator=g).to(DEV)
        k32, v32 = k[:, :32].contiguous(), v[:, :32].contiguous()
        k64, v64 = k[:, :64].contiguous(), v[:, :64].contiguous()
        tag = f"d{d}m{m}"
        timed(f"{tag} keys Nc32", lambda: favor_keys(k32, proj))
        lens = [32 - (t % 20) for t in range(T)]
        timed(f"{tag} keys_ragged Nc32", lambda: favor_keys(k32, proj, lens=lens))
        st = favor_keys(k32, proj)
        timed(f"{tag} query Nc32 Nq300", lambda: favor_query(q, st, v32, proj))
        timed(f"{tag} absorb Nc64", lambda: favor_absorb(None, k64, v64, proj))
        ss = favor_absorb(None, k64, v64, proj)
        timed(f"{tag} sum_query Nq300", lambda: favor_query(q, ss, None, proj))
        q30 = q[:, :30].contiguous()
        timed(f"{tag} prefix_long Nc128 Nq30 K8", lambda: favor_prefixes_long(q30, k, v, proj, [1, 16, 32, 33, 64, 65, 100, 128]))
        Tl = 4
        ql, kl, vl = q[:Tl, :40].contiguous(), k[:Tl, :70].contiguous(), v[:Tl, :70].contiguous()
        dout = torch.randn(Tl, 40, d * H, generator=g).to(DEV)

        def lin():
            o, ws = lib.favor_fwd(ql, kl, vl, proj)
            lib.favor_bwd(ql, kl, vl, proj, o, dout, ws)
        lib.set_option("favor_linear", 1)
        try:
            timed(f"{tag} favor_linear Nq40 Nc70", lin)
        finally:
            lib.set_option("favor_linear", 0)

    s = CV._Setup(lib, "live", 64, 266, 32, 300, True)
    timed("np_query d64m266 Nc32 Nq300", lambda: s.fused(s.x))
    p = PV._Setup(lib, "live", 64, 266, 32, 300, True)
    timed("np_prefix d64m266 Nc32 Nq300", lambda: p.fused(p.x))
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(len(out), "labels ->", sys.argv[1])


if __name__ == "__main__":
    main()
