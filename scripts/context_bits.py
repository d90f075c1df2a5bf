"""Cached-context inference and the prefix sweeps through their public entry points, over the model grids the GPU tests own: per
call one sha256 per output tensor and per state tensor, and the sequence of launch labels (mlhot_prof_begin / _end).  Two trees
of the Python package on one library compute the same thing through the same launches iff the lists are equal line for line: no
tolerance.

    python scripts/context_bits.py --pkg <a package directory> --out A.txt        (one fresh process per tree)
    python scripts/context_bits.py --diff A.txt B.txt                             (exit status 1 and the differing lines, if any)

`--pkg`: the directory that holds mlhot/ and networks/ (default: this tree's); MLHOT_LIB names the library as everywhere.  Models
and shot counts: test_condition_gpu, test_cached_vanilla_gpu, test_ragged_context_gpu, test_cached_summary_gpu, test_sweep_long_gpu,
test_prefix_vanilla_gpu, test_prefix_sweep_gpu, test_prefix_fold_gpu.  Per model: condition dense, with ctx_len / capacity and - an
attention model - form="summary"; extend once on each; predict at one target and chunked; sweep / forward_prefixes with the default
ks, a sparse ks and fold=True where it exists."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STATE_TENSORS = ("vh", "kh", "rs", "lv", "r", "z")


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(emit):
    import torch
    import mlhot
    from mlhot import cached
    from tests import test_cached_summary_gpu as CS
    from tests import test_cached_vanilla_gpu as CV
    from tests import test_condition_gpu as TC
    from tests import test_prefix_fold_gpu as PF
    from tests import test_prefix_sweep_gpu as PS
    from tests import test_prefix_vanilla_gpu as PV
    from tests import test_ragged_context_gpu as RC
    from tests import test_sweep_long_gpu as SL
    lib = mlhot.lib()

    def call(tag, what, fn):
        """fn() between prof_begin / prof_end -> its result; the launch labels and every tensor of the result go to emit."""
        lib.prof_begin(1 << 14)
        try:
            out = fn()
        finally:
            labels = [label for label, _ in lib.prof_end()]
        emit(f"{tag} {what} launches {' '.join(labels)}")
        if torch.is_tensor(out):
            emit(f"{tag} {what} out {tuple(out.shape)} {digest(out)}")
            return out
        emit(f"{tag} {what} state {out.kind} {out.form} Nc={out.Nc} lens={out.lens} capacity={out.capacity}")
        if out.keys is not None:
            views = out.keys.summary() if out.keys.route == "summary" else out.keys.features()
            for i, t in enumerate(views):
                emit(f"{tag} {what} keys.{out.keys.route}.{i} {digest(t)}")
        for name in STATE_TENSORS:
            t = getattr(out, name)
            if t is not None:
                emit(f"{tag} {what} {name} {tuple(t.shape)} {digest(t)}")
        return out

    def predicts(tag, what, model, state, qx):
        call(tag, f"{what}.predict1", lambda: cached.predict(model, state, qx[:, :1].contiguous()))
        call(tag, f"{what}.predict_chunk3", lambda: cached.predict(model, state, qx, chunk=3))

    def lifecycle(tag, model, shots, Nc, Nq=7):
        """shots(n, seed) -> (images [T, n, ...], labels [T, n, L]) on the device."""
        (cx, cy), (nx, ny), qx = shots(Nc, 3), shots(2, 4), shots(Nq, 5)[0]
        T = cx.shape[0]
        predicts(tag, "dense", model, call(tag, "dense", lambda: cached.condition(model, cx, cy)), qx)
        if Nc < 1:
            return
        lens, add = [1 + (2 * t) % Nc for t in range(T)], [(t + 1) % 3 for t in range(T)]
        state = call(tag, "ragged", lambda: cached.condition(model, cx, cy, ctx_len=lens, capacity=Nc + 3))
        predicts(tag, "ragged", model, state, qx)
        predicts(tag, "ragged.extend", model, call(tag, "ragged.extend", lambda: cached.extend(model, state, nx, ny, new_len=add)), qx)
        if model.ATTENTION:
            summary = call(tag, "summary", lambda: cached.condition(model, cx, cy, ctx_len=lens, form="summary"))
            predicts(tag, "summary", model, summary, qx)
            predicts(tag, "summary.extend", model, call(tag, "summary.extend", lambda: cached.extend(model, summary, nx, ny, new_len=add)), qx)

    def split(batch):
        """A tests' _batch(Nc, Nq, seed) -> shots(n, seed)."""
        return lambda n, seed: batch(n, 1, seed)[:2]

    for case, (_, cfg) in TC.MODEL_CASES.items():
        for Nc in (0, 1, 5):
            lifecycle(f"condition/{case}/Nc{Nc}", TC._model(case), split(lambda n, q, s, cfg=cfg: TC._batch(cfg, n, q, seed=s)), Nc)
    for case in CV.MODEL_CASES:
        for Nc in (0, 1, 5):
            lifecycle(f"cached_vanilla/{case}/Nc{Nc}", CV._model(case), split(lambda n, q, s, case=case: CV._batch(case, n, q, seed=s)), Nc)
    for case in RC.MODEL_CASES:
        lifecycle(f"ragged/{case}/Nc5", RC._model(case), lambda n, s, case=case: RC._images(case, n, s), 5, Nq=RC.NQ)
    for case in CS.CASES:
        model, (cx, cy, qx) = CS._model(case), CS._batch(case)
        tag = f"summary/{case}/Nc40"
        first = call(tag, "summary20", lambda: cached.condition(model, cx[:, :20].contiguous(), cy[:, :20].contiguous(), form="summary"))
        grown = call(tag, "summary20.extend", lambda: cached.extend(model, first, cx[:, 20:].contiguous(), cy[:, 20:].contiguous(), new_len=[20, 11]))
        predicts(tag, "summary20.extend", model, grown, qx)
        predicts(tag, "summary40", model, call(tag, "summary40", lambda: cached.condition(model, cx, cy, form="summary")), qx)

    def sweeps(tag, model, cx, cy, qx, sparse, fold=False, **kw):
        call(tag, "sweep", lambda: cached.sweep(model, cx, cy, qx, **kw))
        call(tag, f"sweep.ks{'_'.join(map(str, sparse))}", lambda: cached.sweep(model, cx, cy, qx, ks=sparse, **kw))
        if fold:
            call(tag, "fold", lambda: model.forward_prefixes(cx, cy, qx, fold=True))
            call(tag, f"fold.ks{'_'.join(map(str, sparse))}", lambda: model.forward_prefixes(cx, cy, qx, ks=sparse, fold=True))

    for case in PV.MODEL_CASES:
        sweeps(f"prefix_vanilla/{case}", PV._model(case), *PV._batch(case, 5, 7), [2, 5])
        sweeps(f"prefix_vanilla/{case}/composed", PV._model(case), *PV._batch(case, 5, 7), [2, 5], route="composed")
    for case, (method, cfg, T, Nc, Nq) in PS.MODEL_CASES.items():
        sweeps(f"prefix_sweep/{case}", PS._model(method, cfg, T), *PS._batch(cfg, T, Nc, Nq), [1, Nc], fold=case in PF.CASES)
    for method, cfg in (("ANPShapeNet1D", SL.CFG1D), ("ANP", SL.CFG3D)):
        sweeps(f"sweep_long/{method}", SL._model(method, cfg), *SL._batch(cfg, SL.NC, SL.NQ), SL.KS, fold=method == "ANP")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "what-matters-for-meta-learning_amd"), help="the directory that holds mlhot/ and networks/")
    ap.add_argument("--out", help="write the list here as well as to stdout")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"), help="compare two lists; no GPU needed")
    args = ap.parse_args()
    if args.diff:
        a, b = (open(p).read().splitlines() for p in args.diff)
        bad = [f"{x}\n    != {y}" for x, y in zip(a, b) if x != y]
        if len(a) != len(b):
            bad.append(f"{len(a)} lines against {len(b)}")
        launches = sum(1 for x in a if " launches " in x)
        print("\n".join(bad) if bad else f"{len(a) - launches} digests and {launches} launch sequences, all equal")
        return 1 if bad else 0
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(args.pkg))
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    run(emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
