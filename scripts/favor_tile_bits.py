"""One sha256 per (entry, case, output tensor) of every entry whose kernels are built from csrc/favor_tile.h, over the case tables
the tests own.  Two builds of the library compute the same thing iff the lists are equal line for line: no tolerance.

    MLHOT_LIB=<a libmlhot.so> python scripts/favor_tile_bits.py --out A.txt      (one fresh process per library)
    python scripts/favor_tile_bits.py --diff A.txt B.txt                         (exit status 1 and the differing lines, if any)

Entries: keys, ragged keys and query (favor_cached.h), summary absorb and query (favor_summary.h), prefix-long
(favor_prefix_long.h), np_query and np_prefix (np_query.h, np_prefix.h), favor forward and backward with favor_linear=1
(favor_linear.h).  Cases: test_condition_gpu's and test_ragged_context_gpu's grids, tests/favor_summary_ref.py,
tests/prefix_long_ref.py, the vanilla tests' DM x NCS grids, tests/favor_linear_cases.py."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "what-matters-for-meta-learning_amd"))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
KINDS = ["live", "big", "peak", "equal"]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def run(emit):
    import torch
    import mlhot
    from mlhot.ops import favor_absorb, favor_keys, favor_prefixes_long, favor_query
    from tests import favor_linear_cases as LC
    from tests import favor_summary_ref as S
    from tests import prefix_long_ref as L
    from tests import test_cached_vanilla_gpu as CV
    from tests import test_condition_gpu as TC
    from tests import test_prefix_vanilla_gpu as PV
    from tests import test_ragged_context_gpu as RC
    lib = mlhot.lib()

    for d, m in TC.DM:
        for Nc in TC.NCS:
            for kind in KINDS:
                q, k, v, proj = TC._inputs(kind, d, m, Nc, 100)
                qd, vd, pd = dev(q), dev(v), proj.to(DEV)
                state = favor_keys(dev(k), pd)
                fk, M = state.features()
                case = f"{kind}-d{d}-m{m}-Nc{Nc}"
                emit("keys", case, "fk", fk)
                emit("keys", case, "M", M)
                for Nq in (1, 17, 100):
                    emit("query", f"{case}-Nq{Nq}", "out", favor_query(qd[:, :Nq].contiguous(), state, vd, pd))

    for d, m, Nc, lens in RC.MASKED_CASES:
        for kind in ("live", "big", "equal"):
            q, k, v, proj = RC._inputs(kind, d, m, Nc, 33)
            pd = proj.to(DEV)
            state = favor_keys(dev(k), pd, lens=list(lens))
            fk, M = state.features()
            case = f"{kind}-d{d}-m{m}-Nc{Nc}-lens{'_'.join(map(str, lens))}"
            emit("keys_ragged", case, "fk", fk)
            emit("keys_ragged", case, "M", M)
            emit("query", case, "out", favor_query(dev(q), state, dev(v), pd))

    for d, m in S.SHAPES:
        for chunking in S.CHUNKINGS:
            for kind in S.KINDS:
                c = S.case(kind, d, m, chunking)
                state, pd = None, c["proj"].to(DEV)
                for kc, vc, lens in c["chunks"]:
                    state = favor_absorb(state, dev(kc), dev(vc), pd, lens=None if all(n == kc.shape[2] for n in lens) else lens)
                case = f"{kind}-d{d}-m{m}-{chunking}"
                for name, t in zip(("A", "a", "vs", "cnt", "M"), state.summary()):
                    emit("summary_absorb", case, name, t)
                emit("summary_query", case, "out", favor_query(dev(c["q"]), state, None, pd))

    for d, m in L.SHAPES:
        for Nc in L.NCS:
            for kind in L.KINDS:
                c = L.case(kind, d, m, Nc)
                kd, vd, pd = dev(c["k"]), dev(c["v"]), c["proj"].to(DEV)
                for Nq in L.NQS:
                    qd = dev(c["q"][:, :, :Nq])
                    for name, ks in L.ks_sets(Nc).items():
                        emit("prefix_long", f"{kind}-d{d}-m{m}-Nc{Nc}-Nq{Nq}-ks{name}", "out", favor_prefixes_long(qd, kd, vd, pd, ks))
            for lens in L.LENS.get(Nc, ()):
                c = L.case("live", d, m, Nc)
                out = favor_prefixes_long(dev(c["q"]), dev(c["k"]), dev(c["v"]), c["proj"].to(DEV), lens=list(lens))
                emit("prefix_long", f"live-d{d}-m{m}-Nc{Nc}-lens{'_'.join(map(str, lens))}", "out", out)

    for d, m in CV.DM:
        for Nc in CV.NCS:
            for kind in KINDS:
                s = CV._Setup(lib, kind, d, m, Nc, 33, True)
                emit("np_query", f"{kind}-d{d}-m{m}-Nc{Nc}", "mu", s.fused(s.x))
    for d, m in PV.DM:
        for Nc in PV.NCS:
            for kind in PV.PR.ATTENTION_KINDS:
                s = PV._Setup(lib, kind, d, m, Nc, 33, True)
                emit("np_prefix", f"{kind}-d{d}-m{m}-Nc{Nc}-all", "mu", s.fused(s.x))
                emit("np_prefix", f"{kind}-d{d}-m{m}-Nc{Nc}-last", "mu", s.fused(s.x, [Nc]))

    lib.set_option("favor_linear", 1)
    try:
        for case in LC.CASES:
            qn, kn, vn, dout, proj = (t.to(DEV) for t in LC.kernel_layout(LC.inputs(case.name)))
            out, ws = lib.favor_fwd(qn, kn, vn, proj)
            dq, dk, dv = lib.favor_bwd(qn, kn, vn, proj, out, dout, ws)
            for name, t in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv)):
                emit("favor_linear", case.name, name, t)
    finally:
        lib.set_option("favor_linear", 0)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the digest list here as well as to stdout")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"), help="compare two digest lists; no GPU needed")
    args = ap.parse_args()
    if args.diff:
        a, b = (open(p).read().splitlines() for p in args.diff)
        bad = [f"{x}\n    != {y}" for x, y in zip(a, b) if x != y]
        if len(a) != len(b):
            bad.append(f"{len(a)} lines against {len(b)}")
        print("\n".join(bad) if bad else f"{len(a)} digests, all equal")
        return 1 if bad else 0
    lines = []

    def emit(entry, case, name, t):
        lines.append(f"{entry} {case} {name} {digest(t)}")
        print(lines[-1], flush=True)

    run(emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
