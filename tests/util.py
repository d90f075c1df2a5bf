"""Shared helpers for the parity tests."""
import glob
import hashlib
import importlib
import json
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star: "outputs match the reference PyTorch CPU path within 1e-4 rel fp32".
# Metric (SURVEY.md §7 hard parts): tensor-scale relative error  max|a-b| / max|b|.
RTOL = 1e-4
# Gradients far below the model's largest gradient entry are fp32 cancellation residue (at
# init the FAVOR+ normaliser cancels the Q/K scale, leaving ~1e-9 gradients next to ~1e-1
# ones); they are compared at a floor of GRAD_FLOOR x (largest |grad| entry of the model).
GRAD_FLOOR = 1e-4


def rel_err(a, b, floor=0.0):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.numel() == b.numel(), (a.shape, b.shape)
    a = a.reshape(b.shape)
    scale = max(b.abs().max().item(), floor, 1e-30)
    return (a - b).abs().max().item() / scale


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def model_case_names(prefix=""):
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, prefix + "*.npz"))
                  if os.path.basename(f)[0] in "cs" and os.path.basename(f)[1] in "123_" and "conv_emb" not in f)


def load_case(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    return fx, json.loads(str(fx["meta"]))


def case_config(meta, device="cpu"):
    return types.SimpleNamespace(device=torch.device(device), **meta["cfg"])


def build_model(meta, device="cpu", fx=None):
    """Identically-seeded module of this repo.  Parameters must regenerate bit-exactly (sha-checked
    against the reference); the FAVOR+ projection buffer comes out of a LAPACK QR whose low bits
    depend on the host CPU, so it is checked to 1e-5 and then loaded from the fixture."""
    cfg = case_config(meta, device)
    mod = importlib.import_module("networks." + meta["method"])
    model = getattr(mod, meta["method"])(cfg)
    for k, v in model.state_dict().items():
        if k == "attn.projection_matrix":
            continue
        assert sha(v) == meta["state_sha"][k], f"{k}: seeded init differs from the reference"
    if fx is not None and "projection_matrix" not in fx.files and meta.get("projection_from"):
        fx = np.load(os.path.join(GOLDEN, meta["projection_from"] + ".npz"))      # the same buffer for every fixture of this model and seed
    if fx is not None and "projection_matrix" in fx.files:
        ref = torch.from_numpy(fx["projection_matrix"])
        assert sha(ref) == meta["state_sha"]["attn.projection_matrix"]
        assert rel_err(model.attn.projection_matrix, ref) <= 1e-3   # QR low bits are host-LAPACK dependent
        with torch.no_grad():
            model.attn.projection_matrix.copy_(ref)
    return model


def case_inputs(meta):
    c = meta["cfg"]
    T, Nc, Nq = c["tasks_per_batch"], meta["Nc"], meta["Nq"]
    H, W, C = c["img_size"]
    g = torch.Generator().manual_seed(meta["input_seed"])
    cx = torch.rand(T, Nc, C, H, W, generator=g)
    qx = torch.rand(T, Nq, C, H, W, generator=g)
    cy = torch.rand(T, Nc, c["input_dim"], generator=g)
    qy = torch.rand(T, Nq, c["input_dim"], generator=g)
    for k, t in (("cx", cx), ("qx", qx), ("cy", cy), ("qy", qy)):
        assert sha(t) == meta["input_sha"][k], f"input {k} does not regenerate from the seed"
    return cx, qx, cy, qy


def resnet_case_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "r_*.npz")))


def fcl_case_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "f_*.npz")))


def mr_case_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "m_*.npz")))


def resnet_case_inputs(meta, fx):
    c = meta["cfg"]
    T, Nc, Nq, C = c["tasks_per_batch"], meta["Nc"], meta["Nq"], meta["C"]
    H, W, _ = c["img_size"]
    g = torch.Generator().manual_seed(meta["input_seed"])
    cx = torch.rand(T, Nc, C, H, W, generator=g)
    qx = torch.rand(T, Nq, C, H, W, generator=g)
    cy = torch.rand(T, Nc, c["input_dim"], generator=g)
    for k, t in (("cx", cx), ("qx", qx), ("cy", cy)):
        assert sha(t) == meta["input_sha"][k], f"input {k} does not regenerate from the seed"
    return cx, qx, cy, torch.from_numpy(fx["qy"])


def c5_full_case_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "c5_*.npz")))


def c5_full_case_inputs(meta):
    """The c5 per-GPU-size fixtures' inputs (tests/golden/make_fixtures.py::run_c5_full_case): ONE generator seeded 1234, images
    U[0, 1), labels = normalised N(0, 1)^4 quaternions ("quat") or SURVEY section 8c's torch.rand labels ("rand")."""
    T, Nc, Nq = meta["cfg"]["tasks_per_batch"], meta["Nc"], meta["Nq"]
    g = torch.Generator().manual_seed(meta["input_seed"])
    cx, qx = torch.rand(T, Nc, 3, 64, 64, generator=g), torch.rand(T, Nq, 3, 64, 64, generator=g)
    if meta["labels"] == "quat":
        cy = torch.nn.functional.normalize(torch.randn(T, Nc, 4, generator=g), dim=-1)
        qy = torch.nn.functional.normalize(torch.randn(T, Nq, 4, generator=g), dim=-1)
    else:
        cy, qy = torch.rand(T, Nc, 4, generator=g), torch.rand(T, Nq, 4, generator=g)
    for k, t in (("cx", cx), ("qx", qx), ("cy", cy), ("qy", qy)):
        assert sha(t) == meta["input_sha"][k], f"input {k} does not regenerate from the seed"
    return cx, qx, cy, qy


def loss_kind(task):
    return {"shapenet_1d": "azimuth", "pascal_1d": "mse", "shapenet_3d": "quaternion", "distractor": "distractor"}[task]


def fixture_gmax(keys, fx):
    gmax = 0.0
    for k in keys:
        if "grad/" + k in fx:
            gmax = max(gmax, float(np.abs(fx["grad/" + k]).max()))
        elif "gradhead/" + k in fx:
            gmax = max(gmax, float(np.abs(fx["gradhead/" + k]).max()))
    return gmax


def check_grads_against_fixture(grads, fx, meta, tol=RTOL, head=4096, stride_cap=None, gmax=None):
    """grads: dict key -> tensor (or None).  Compares with the fixture's full / sampled grads.  gmax: the model's largest gradient
    entry (default: the largest among `grads`' fixture entries); gradients below GRAD_FLOOR x gmax are compared at that floor."""
    gmax = fixture_gmax(grads, fx) if gmax is None else gmax
    floor = GRAD_FLOOR * gmax
    worst = (0.0, None)
    for k, g in grads.items():
        want_norm = meta["grad_norm"][k]
        if want_norm is None:
            assert g is None, f"{k}: reference has grad=None"
            continue
        assert g is not None, f"{k}: missing gradient"
        g = g.detach().cpu()
        if "grad/" + k in fx:
            e = rel_err(g, fx["grad/" + k], floor)
        else:
            flat = g.reshape(-1)
            strided = flat[1::61] if stride_cap is None else flat[1::61][:stride_cap]
            e = max(rel_err(flat[:head], fx["gradhead/" + k], floor), rel_err(strided, fx["gradstride/" + k], floor))
            assert abs(float(flat.double().norm()) - want_norm) <= tol * max(want_norm, floor), f"{k}: grad norm"
        if e > worst[0]:
            worst = (e, k)
        assert e <= tol, f"{k}: gradient rel err {e:.3e} > {tol}"
    return worst


def test_loss_allowance(task, mu, gt, rtol=RTOL):
    """How far LossFunc.calc_loss(..., test=True) may move when mu is off by north_star's `rtol` of its scale - derived, not guessed
    (trainer/losses.py:50-80).  shapenet_1d's test loss is the degree error acos(mu[0]): acos is the one amplifying step,
    |d deg| = (180 / pi) |d mu0| / sqrt(1 - mu0^2), capped at acos's square-root branch point by (180 / pi) sqrt(2 |d mu0|);
    everything behind it (the 360-degree wrap, abs, the minimum of three, the mean over rows) is 1-Lipschitz.  The other tasks'
    test losses are their training losses: mean_square_loss moves by mean(2 |gt - mu| dm + dm^2) (pascal_1d), the distractor's
    Euclidean distance and the quaternion L1 by at most sqrt(k) dm resp. k dm / |q| per row; + 1e-5 relative for the fp32
    reductions themselves."""
    mu, gt = torch.as_tensor(mu).detach().double().cpu(), torch.as_tensor(gt).detach().double().cpu()
    dm = rtol * mu.abs().max().item()
    if task == "shapenet_1d":
        m0 = mu[..., 0].clamp(-1.0, 1.0)
        per_row = torch.minimum(dm / torch.sqrt((1.0 - m0 * m0).clamp_min(1e-30)), torch.full_like(m0, (2.0 * dm) ** 0.5)) * (180.0 / np.pi)
        return per_row.mean().item()
    if task == "pascal_1d":
        return (2.0 * (gt - mu).abs() * dm + dm * dm).mean().item()
    if task == "distractor":
        return mu.shape[-1] ** 0.5 * dm
    norm = mu.pow(2).sum(-1).sqrt().clamp_min(1e-30)            # shapenet_3d: q / |q|, then an L1 distance
    return (2.0 * mu.shape[-1] * dm / norm).mean().item()


test_loss_allowance.__test__ = False       # a helper, not a test (pytest collects names starting with test_)


# What ONE routing decision that sits on a tie and fell the other way does to a gradient: it adds or removes one position's term of the
# sums behind every weight gradient below it, so its share of a tensor's largest entry shrinks with the number of images summed over.
# On record (MI355X box, round 6; kernels vs the REFERENCE's own gradients): 3.6e-2 of a stem gradient's scale for one flip at 5 images
# (r_anp_distractor), 7.9e-3 at 8 (r_cnp_distractor_mean), 1.5e-2 / 3.0e-3 at 10 (f_fclcnp_distractor_*), 3.0e-4 at 360 (c5, T = 8),
# 7e-5 per flip at 480 (c2: three flips, 2.1e-4) - every one of them <= 0.2 / n_images.  The bound against the fixture is therefore
#     tol                                           when no decision differs from the oracle's own (the strong statement), else
#     tol + (flips + 1) x FLIP_SHARE / n_images     flips = decisions that differ between the kernels and the oracle run beside them;
# the "+ 1": the oracle's own run on THIS host may itself decide a tie differently from the reference's recorded run on the build
# container (another CPU, another summation order - seen on the GPU box: the oracle's own-routing gradients were off the fixture's by
# one flip's worth while the kernels' routing equalled the oracle's).  The exact effect of the kernels-vs-oracle flips, measured in
# the oracle (flip_effect), is logged next to the error.
FLIP_SHARE = 0.2
_EFFECT_CACHE = {}


def flip_effect(routed, own, floor=0.0):
    """Per parameter: max |grad under the kernels' routing - grad under the oracle's own routing| / scale of the tensor (both from the
    oracle, same arithmetic): what the differing routing decisions do to that gradient."""
    out = {}
    for k, g in routed.items():
        if g is None or own.get(k) is None:
            continue
        out[k] = rel_err(g, own[k], floor)
    return out


def parity_log(line):
    """Append one line to the parity log the GPU tests keep (flip counts, decisions, worst errors): $MLHOT_PARITY_LOG, else
    gpurun_out/parity_flips.txt next to the repo root (merged back by gpurun; the summary is committed under profiles/)."""
    path = os.environ.get("MLHOT_PARITY_LOG") or os.path.join(os.path.dirname(GOLDEN.rstrip("/")), "..", "gpurun_out", "parity_flips.txt")
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line.rstrip("\n") + "\n")
    except OSError:
        pass


def check_grads_against_fixture_flipped(grads, fx, meta, flips, what="", tol=RTOL, effect=None, n_images=None, **kw):
    """The reference's OWN gradients (the fixture) against the kernels', ALWAYS - at `tol` when no routing decision differs, otherwise
    at tol + (flips + 1) x FLIP_SHARE / n_images (above); each differing decision was proven a <= TIE tie of the oracle's
    pre-activations by the caller.  `effect`: flip_effect(...) or a callable returning it - the differing decisions' exact effect in
    the oracle, logged.  Returns (worst error, its tensor, the bound)."""
    if n_images is None:
        n_images = meta["cfg"]["tasks_per_batch"] * (meta["Nc"] + meta["Nq"])
    bound = tol if flips == 0 else tol + (flips + 1) * FLIP_SHARE / max(1, n_images)
    worst = check_grads_against_fixture(grads, fx, meta, tol=bound, **kw)
    note = ""
    if flips and effect is not None:
        # one extra oracle run (under its OWN routing): once per case and flip count is enough for the log - the tail / split-precision
        # flavours of a case share the encoder's routing
        key = (what.split(" ")[0], flips)
        if key not in _EFFECT_CACHE:
            eff = effect() if callable(effect) else effect
            _EFFECT_CACHE[key] = max(eff.values(), default=0.0)
        note = f"; the differing decisions' effect measured in the oracle: {_EFFECT_CACHE[key]:.2e} of a tensor's scale at most"
    parity_log(f"{what}: {flips} routing decisions on a tie fell the other way ({n_images} images); gradients vs the REFERENCE's own (fixture): "
               f"worst {worst[0]:.2e} ({worst[1]}) <= {bound:.2e}{note}")
    return worst[0], worst[1], bound


# ---- pinned routing: the kernels' own ReLU / pool decisions, fed to the oracle; every disagreement with the
# oracle's own decision must sit on a rounding-level tie of the oracle's pre-activations -----------------------------------
TIE = 1e-5


def relu_flips(mask, pre, what="", tie=None):
    """# of ReLU decisions in `mask` that differ from sign(pre); asserts that each of them is a tie (|pre| <= tie * max|pre|,
    tie = TIE unless given)."""
    tie = TIE if tie is None else tie
    mask, pre = torch.as_tensor(mask).cpu().reshape(pre.shape), pre.detach()
    bad = (mask > 0) != (pre > 0)
    n = int(bad.sum())
    if n:
        worst = float((bad * pre.abs()).max() / pre.abs().max())
        assert worst <= tie, f"{what}: ReLU routing differs away from a tie ({worst:.2e} of the layer's largest pre-activation > {tie:.2e})"
    return n


def encoder_flips(route, pre, what="", tie=None):
    """Vanilla encoder: route = (m1, arg2, m2, m3) against the pre-activations of oracle.vanilla_encoder_routed."""
    m1, arg2, m2, m3 = route
    n = relu_flips(m1, pre["y1"], what + " conv1", tie) + relu_flips(m3, pre["y3"], what + " conv3", tie)
    win = torch.relu(pre["y2win"].detach())               # the pool runs on the post-ReLU map
    chosen = torch.gather(win, 4, arg2.long().unsqueeze(-1)).squeeze(-1)
    gap = win.max(dim=4).values - chosen
    assert not bool((gap > (TIE if tie is None else tie) * win.abs().max()).any()), f"{what}: pool arg-max differs away from a tie"
    n += int((gap > 0).sum())
    n += relu_flips(m2, torch.gather(pre["y2win"].detach(), 4, arg2.long().unsqueeze(-1)).squeeze(-1), what + " conv2", tie)
    return n


def self_routes_vanilla(x, p, prefix="encoder_w0."):
    """The oracle's OWN routing decisions on images x, in the form vanilla_encoder_routed takes them."""
    from oracle import ref_cpu as O
    taps = {}
    with torch.no_grad():
        O.vanilla_encoder(x, p, prefix=prefix, taps=taps)
    a2 = taps["a2"]
    n, c, h, w = a2.shape
    win = a2.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    return (taps["a1"] > 0).float(), win.argmax(dim=4).to(torch.uint8), (taps["p2"] > 0).float(), (taps["a3"] > 0).float()


# ---- vanilla encoder: parameters, options, launch labels (tests/enc_cases.py, tests/test_enc_route_gpu.py, tests/test_gpu_parity.py) ----
FLIP_RATE = 1e-6        # bound on the share of routing decisions that may sit on a tie and fall the other way

ENC_OPTION_DEFAULTS = {"conv2_tc": 1, "conv2_split": 0, "conv3_bwd_merged": 1, "materialize_a1": 0, "tail_spec": 7935}


def enc_params(dim_w, seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [("0.weight", (32, 1, 3, 3), 0.3), ("0.bias", (32,), 0.1), ("2.weight", (48, 32, 3, 3), 0.06), ("2.bias", (48,), 0.1),
              ("5.weight", (64, 48, 3, 3), 0.05), ("5.bias", (64,), 0.1), ("8.weight", (dim_w, 4096), 0.02), ("8.bias", (dim_w,), 0.1)]
    return {"encoder_w0." + k: torch.randn(*s, generator=g) * a for k, s, a in shapes}


def with_options(gpulib, opts, fn):
    """fn() under the options `opts`; every option of ENC_OPTION_DEFAULTS is back at its default afterwards."""
    try:
        for k, v in opts.items():
            gpulib.set_option(k, v)
        return fn()
    finally:
        for k, v in ENC_OPTION_DEFAULTS.items():
            gpulib.set_option(k, v)


def launch_labels(gpulib, fn):
    """-> (the labels of the launches fn() made, counted through mlhot_prof_begin / _end, fn's result)"""
    gpulib.prof_begin(256)
    try:
        out = fn()
    finally:
        labels = [label for label, _ in gpulib.prof_end()]
    return labels, out


# the weight-stationary encoder's launches, recorded by tests/test_enc_route_gpu.py (see its docstring)
ENC_FWD_WS = ["enc.conv12", "enc.conv3", "enc.linear", "slab_reduce"]
ENC_BWD_WS_TAIL = ["enc.bwd.conv12.wgrad", "enc.bwd.conv12.dgrad", "slab_reduce", "slab_reduce"]      # conv1's gradients (tensors of their own), the deferred folds
ENC_BWD_WS = ["enc.bwd.linear", "enc.bwd.conv3.wgrad", "enc.bwd.conv3.dgrad"] + ENC_BWD_WS_TAIL
ENC_BWD_WS_MERGED = ["enc.bwd.linear", "enc.bwd.conv3"] + ENC_BWD_WS_TAIL
