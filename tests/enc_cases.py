"""Shared by tests/test_enc_cases_cpu.py (host flavour of the library) and tests/test_enc_envelope_gpu.py (MI355X): the vanilla image
encoder (csrc/encoder.h and the kernels it launches: conv_tc.h, conv_split.h, conv3_tc.h, enc_linear.h, the generic chain of igemm.h)
through enc_vanilla_fwd / enc_vanilla_bwd at every image count where one of its kernels changes what it does, against float64.

The geometry is fixed (1 x 128 x 128 images), so a case is (n0, n1, dim_w, options).  The edges the code draws, and the counts on
either side of each:
  el::RCH = 240     enc_linear_bwd_kernel stages 240 rows at a time: one chunk, a second and a third partial chunk (239 .. 241, 479,
                    481), and chunks that straddle the Rows2 boundary of dfeat ((239,2), (240,1), (1,240), (200,57), (256,1))
  16-row tiles      enc_linear_fwd_kernel and its fold: 15, 16, 17; Rows2 out split at a multiple of 16 and one off it
  conv12_grid(n)    n * 8 below 32 images, 256 from there on: 31, 32, 33 (33: 264 units on 256 workgroups, a remainder)
  conv3 forward     two half-image units per image on <= 256 workgroups: 127, 128, 129
  C2_GRID = 256     the merged conv3 backward from n >= 256: 255, 256, 257, and its split conv3_nw = 128 (option 1), 64, 2 and 255
                    (the extreme legal splits), 0 (two launches) at 256 and 257
  the generic chain enc_linw_split at 64, conv3w_split = n / 4, conv2w_split = n / 2 capped at 240, conv1w_split = 2 n capped at 1024
                    (from n = 512): 3, 4, 63, 64, 65, 513 under conv2_tc = 0
  the mixed route   weight-stationary convolutions with the generic Linear: dim_w = 32 at n = 65, dim_w = 128 at n = 17

Inputs: util.enc_params (the shapes and scales of tests/test_enc_route_gpu.py), images torch.rand with image 0 all zero (the bias-only path)
and image 1 all one (the padding ring is the only structure), the LAST image random - the last rows of a partial chunk are where these
kernels can go wrong - and dfeat randn, split at n0.  EVERY case has images and dfeat of its own (the seed takes the case's place in the
table), also where two cases share (n0, n1, dim_w): the binding takes its scratch from the caching allocator, which hands a case the
block the last call of the same size left behind, and with the same inputs that block would hold the RIGHT dp2, dy3 and slab rows - an
output row a kernel never writes would pass.  With inputs of its own a case finds in such a block, at best, another case's numbers.

Reference: oracle.ref_cpu.vanilla_encoder_routed on float64 copies, under the library's OWN routing decisions (enc_routes of the
forward's saved buffer; the generic chain keeps a1 itself and writes no sign-bit words, so its conv1 mask is a1 > 0).  Every decision
that differs from the float64 sign / arg-max must be a util.TIE tie (util.encoder_flips), and at most max(1, FLIP_RATE x decisions) may
differ: a condition on the INPUTS (tests/test_enc_cases_cpu.py checks it in the host flavour), never a measurement to be widened.
One kind of window is not counted: the all-one image has ~12,000 pool windows of mathematically equal entries, and float64's own
288-term sums leave a few of them (last rows) 1e-16 apart; the kernels, whose four fp32 values are bit-equal, take the first.  A
gap of at most F64_TIE = 1e-12 of the map's largest entry is the reference's rounding, not a decision (counted apart and printed).

Compared (util.rel_err): the features, the saved p2 and a3 (so that a failure names its layer) at 1e-5, the saved pool arg-max against
the reference's own choice wherever the window's two largest post-ReLU values are more than a tie apart, all eight gradients at 2e-5:
the tolerances of test_encoder_full_size_gradients_with_pinned_routing.  Worst values on record: profiles/INDEX_enc_envelope.md."""
import collections

import torch

from oracle import ref_cpu as O
from tests import util as U

TOL_FWD = 1e-5            # features, p2, a3
TOL_GRAD = 2e-5           # the eight gradients
F64_TIE = 1e-12           # of the pooled map's largest entry: four orders above float64's rounding of a 288-term sum, seven below util.TIE
REF_CHUNK = 64            # images per float64 pass (the gradients are sums over images)
PARAM_SEED = 3

Case = collections.namedtuple("Case", "name n0 n1 dim_w opts bwd_labels")


def _case(group, n0, n1=0, dim_w=64, opts=None, bwd_labels=None, tag=""):
    name = f"{group}-n{n0}" + (f"+{n1}" if n1 else "") + (f"-{tag}" if tag else "")
    return Case(name, n0, n1, dim_w, dict(opts or {}), bwd_labels)


def _default_labels(n):
    return U.ENC_BWD_WS_MERGED if n >= 256 else U.ENC_BWD_WS


CASES = (
    [_case("default", n, bwd_labels=_default_labels(n)) for n in (15, 16, 17, 31, 32, 33, 127, 128, 129, 239, 240, 241, 255, 256, 257, 479, 481)]
    + [_case("default", a, b, bwd_labels=_default_labels(a + b)) for a, b in ((15, 1), (16, 16), (17, 15), (239, 2), (240, 1), (1, 240), (200, 57), (256, 1))]
    + [_case("merged", n, opts={"conv3_bwd_merged": m}, bwd_labels=U.ENC_BWD_WS if m == 0 else U.ENC_BWD_WS_MERGED, tag=f"m{m}") for n in (256, 257) for m in (0, 1, 64, 2, 255)]
    + [_case("split7", n, opts={"conv2_split": 7}) for n in (33, 241)]
    + [_case("generic", n, opts={"conv2_tc": 0}) for n in (3, 4, 63, 64, 65, 513)]
    + [_case("mixed", 65, dim_w=32, tag="dw32"), _case("mixed", 17, dim_w=128, tag="dw128")]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the host flavour has the generic chain only and ignores the options: every case of <= 65 images, and one of 241
CPU_CASES = [c.name for c in CASES if c.n0 + c.n1 <= 65] + ["default-n241"]
GRAD_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "wl", "bl")


def inputs(case):
    """-> (params dict, images [n,1,128,128], dfeat [n,dim_w]) on the CPU, fp32; images and dfeat differ from case to case."""
    n = case.n0 + case.n1
    assert n >= 3
    g = torch.Generator().manual_seed(100003 * CASES.index(case) + 1000 * case.n0 + case.n1 + 7 * case.dim_w)
    x = torch.rand(n, 1, 128, 128, generator=g)
    x[0], x[1] = 0.0, 1.0                                  # the last image stays random
    df = torch.randn(n, case.dim_w, generator=g)
    return U.enc_params(case.dim_w, PARAM_SEED), x, df


def reference(case, routes):
    """The float64 encoder under `routes` = (m1, arg2, m2, m3), REF_CHUNK images at a time -> dict(feat, p2, a3, am (the reference's own
    pool choice, uint8), decided (where that choice is more than a tie), grads (8, in parameter order), flips, decisions, where (the
    differing decisions as (layer, image, count)))."""
    p, x, df = inputs(case)
    n = x.shape[0]
    pr = {k: v.double().requires_grad_() for k, v in p.items()}
    out = dict(feat=[], p2=[], a3=[], am=[], decided=[], where=[], flips=0, f64_ties=0, decisions=sum(r.numel() for r in routes))
    for lo in range(0, n, REF_CHUNK):
        hi = min(n, lo + REF_CHUNK)
        m1, arg2, m2, m3 = (r[lo:hi] for r in routes)
        feat, pre = O.vanilla_encoder_routed(x[lo:hi].double(), pr, m1.double(), arg2, m2.double(), m3.double())
        feat.backward(df[lo:hi].double())
        out["flips"] += U.encoder_flips((m1, arg2, m2, m3), pre, f"{case.name} images {lo}..{hi - 1}", U.TIE)
        with torch.no_grad():
            win = pre["y2win"]
            chosen = torch.gather(win, 4, arg2.long().unsqueeze(-1)).squeeze(-1)
            # a pool window whose float64 values differ by float64's OWN rounding (the all-one image: mathematically equal entries, 288-term
            # sums that come out 1e-16 apart in the last rows) is an exact tie, not a decision: whichever entry the kernel took, it is no flip
            gap = torch.relu(win).amax(dim=4) - torch.relu(chosen)
            noise = (gap > 0) & (gap <= F64_TIE * torch.relu(win).max())
            out["flips"] -= int(noise.sum())
            out["f64_ties"] += int(noise.sum())
            for layer, bad in (("conv1", (m1 > 0) != (pre["y1"] > 0)), ("pool", (gap > 0) & ~noise),
                               ("conv2", (m2 > 0) != (chosen > 0)), ("conv3", (m3 > 0) != (pre["y3"] > 0))):
                for i in bad.flatten(1).sum(dim=1).nonzero().flatten().tolist():
                    out["where"].append((layer, lo + i, int(bad[i].sum())))
            out["p2"].append(chosen * m2)
            out["a3"].append(pre["y3"] * m3)
            top = torch.relu(win).topk(2, dim=4)
            out["am"].append(top.indices[..., 0].to(torch.uint8))
            out["decided"].append((top.values[..., 0] - top.values[..., 1]) > U.TIE * top.values.max())
            out["feat"].append(feat.detach())
    for k in ("feat", "p2", "a3", "am", "decided"):
        out[k] = torch.cat(out[k])
    out["grads"] = [v.grad for v in pr.values()]
    # `where` repeats util.encoder_flips' arithmetic to name layer and image: the two must count the same decisions
    assert sum(c for _, _, c in out["where"]) == out["flips"], (out["where"], out["flips"], out["f64_ties"])
    return out


def flip_cap(decisions):
    return max(1, U.FLIP_RATE * decisions)


def check_encoder(lib, case, dev):
    """One forward and one backward of the library on `dev` under the case's options, held to the float64 reference as the module's
    docstring states -> {quantity: rel_err}.  On the device a case that names its backward's launches asserts them as well."""
    p, x, df = inputs(case)
    n0, n1, n, dim_w = case.n0, case.n1, case.n0 + case.n1, case.dim_w
    on_gpu = dev != "cpu"
    plist = [t.to(dev) for t in p.values()]
    x0, x1 = x[:n0].to(dev), (x[n0:].to(dev) if n1 else None)
    df0, df1 = df[:n0].contiguous().to(dev), df[n0:].contiguous().to(dev)

    def run():
        f0, f1, saved = lib.enc_vanilla_fwd(x0, x1, plist, dim_w)
        bwd = lambda: lib.enc_vanilla_bwd(x0, x1, plist, dim_w, df0, df1, saved)
        labels, grads = U.launch_labels(lib, bwd) if on_gpu and case.bwd_labels is not None else (None, bwd())
        if on_gpu:
            torch.cuda.synchronize()
        return torch.cat([f0, f1]).cpu(), saved, [g.cpu() for g in grads], labels
    feat, saved, grads, labels = U.with_options(lib, case.opts, run) if on_gpu else run()
    a1, p2, am2, a3 = (t.cpu() for t in lib.enc_saved_views(saved, n))
    # the generic chain (conv2_tc = 0; all the host flavour has) stores a1 and no sign-bit words
    generic = not on_gpu or case.opts.get("conv2_tc", U.ENC_OPTION_DEFAULTS["conv2_tc"]) == 0
    routes = ((a1 > 0).float(), am2, (p2 > 0).float(), (a3 > 0).float()) if generic else lib.enc_routes(saved, n)
    ref = reference(case, routes)
    errs = {"feat": U.rel_err(feat, ref["feat"]), "p2": U.rel_err(p2, ref["p2"]), "a3": U.rel_err(a3, ref["a3"])}
    errs.update({"d" + k: U.rel_err(g, r) for k, g, r in zip(GRAD_NAMES, grads, ref["grads"])})
    decided = ref["decided"]
    am_wrong = int((am2[decided] != ref["am"][decided]).sum())
    worst_f, worst_g = max(errs[k] for k in ("feat", "p2", "a3")), max(errs["d" + k] for k in GRAD_NAMES)
    print(f"[enc envelope] {case.name} on {dev}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f" | worst forward {worst_f:.2e} (bound {TOL_FWD:.0e}) worst gradient {worst_g:.2e} (bound {TOL_GRAD:.0e}); pool arg-max wrong at {am_wrong} of "
          f"{int(decided.sum())} decided windows; {ref['flips']} of {ref['decisions']} decisions on a tie fell the other way (layer, image, count): {ref['where']}; {ref['f64_ties']} pool windows tied to float64's rounding")
    assert ref["flips"] <= flip_cap(ref["decisions"]), f"{case.name}: {ref['flips']} of {ref['decisions']} routing decisions differ (on ties): change the seed"
    if labels is not None:
        assert labels == case.bwd_labels, f"{case.name}: backward launched {labels}"
    for k in ("p2", "a3", "feat"):
        assert errs[k] <= TOL_FWD, f"{case.name}: {k} rel err {errs[k]:.2e} > {TOL_FWD:.0e}"
    assert am_wrong == 0, f"{case.name}: pool arg-max differs from the reference's choice away from a tie at {am_wrong} windows"
    for k in GRAD_NAMES:
        assert errs["d" + k] <= TOL_GRAD, f"{case.name}: d{k} rel err {errs['d' + k]:.2e} > {TOL_GRAD:.0e}"
    return errs
