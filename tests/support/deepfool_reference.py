"""CPU restatement of DeepFool ("DeepFool"), written from the definition and independently of the device code
(defensegan_amd/csrc/dg_deepfool.hip, attacks.DeepFool): torch on the CPU, float64 by default, the class gradients from autograd.

    net   = logits_fn(model, params, torch.float64)               # x [B,H,W,C] tensor -> logits [B,n], differentiable
    state = start(net, x, nb_candidate)                           # orig, cand, r_tot = 0, adv = x, active
    state, info = step(net, state, lo, hi)                        # one iteration; info: jstar, pert, pert_gap, logit_gap
    out   = run(model, params, x, nb_candidate, overshoot, max_iter, lo, hi)

The definition, per image, on the LOGITS:  orig = first argmax at x;  cand = the nb_candidate classes of the largest logits at x,
descending, ties to the lower class;  r_tot = 0, adv = x.  Active while the first argmax over all classes at adv is orig.  One
iteration of an active image, f_j = Z[cand_j] - Z[cand_0] and w_j = grad Z[cand_j] - grad Z[cand_0] at adv, 0 < j < nc:
pert_j = (|f_j| + 1e-5) / ||w_j||_2 (+inf where ||w_j|| == 0), j* = the first index of the minimum (+inf and NaN are never the minimum;
without a minimum the image becomes inactive and keeps r_tot), r_tot += pert_j* w_j* / ||w_j*||_2, adv = clip(x + r_tot, lo, hi).  A NaN
among the logits makes the image inactive and takes the step that produced it back.  The result is clip(x + (1 + overshoot) r_tot, lo, hi).

``run`` also returns the DECISION MARGINS of its trajectory, per image and iteration: ``pert_gap`` -- (second smallest - smallest) /
smallest of the pert_j -- and ``logit_gap`` -- the gap between the two largest logits at the new adv --, plus ``cand_gap`` (the smallest
gap between neighbours among the nb_candidate + 1 largest logits at x: the order of the candidates) and ``final_gap`` (the two largest
logits at x_adv: final_class).  With ``shadow=torch.float32`` every iteration is ALSO taken in float32 from the same float64 state, and
the largest float32-vs-float64 difference of each quantity compared is recorded: ``pert_err`` (relative, over the pert_j) and
``logit_err`` (absolute, over the logits at x, at the new adv and at x_adv).  ``decidable(out)`` marks the images all of whose margins
exceed 4 x that difference -- the factor leaves room for the device's different summation order, as generator_reference.draw_rows does."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.support import bpda_reference as R


def logits_fn(model, params, dtype=torch.float64):
    """The model's logits (before Softmax; Dropout is the identity) as a differentiable torch function of x [B,H,W,C]."""
    from defensegan_amd import network_builder as nb
    ps = [(torch.tensor(np.asarray(W), dtype=dtype), torch.tensor(np.asarray(b), dtype=dtype)) for W, b in params]

    def net(x):
        h, flat, k = x.permute(0, 3, 1, 2), False, 0                # NCHW inside
        for l in model.layers:
            if isinstance(l, nb.Conv2D):
                W, b = ps[k]
                k += 1
                (kh, kw), (sh, sw) = l.kernel_shape, l.strides
                if l.padding == "SAME":                             # TF: out = ceil(in / stride), the smaller half of the padding in front
                    ih, iw = int(h.shape[2]), int(h.shape[3])
                    pt, pl = max((-(-ih // sh) - 1) * sh + kh - ih, 0), max((-(-iw // sw) - 1) * sw + kw - iw, 0)
                    h = F.pad(h, (pl // 2, pl - pl // 2, pt // 2, pt - pt // 2))
                h = F.conv2d(h, W.permute(3, 2, 0, 1), b, stride=(sh, sw))
            elif isinstance(l, nb.ReLU):
                h = torch.relu(h)
            elif isinstance(l, nb.Flatten):
                h, flat = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1), True
            elif isinstance(l, nb.Linear):
                if not flat:
                    h, flat = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1), True
                W, b = ps[k]
                k += 1
                h = h @ W + b
            elif isinstance(l, (nb.Softmax, nb.Dropout)):
                pass
            else:
                raise NotImplementedError(l.__class__.__name__)
        return h
    return net


def _first_argmax(z):
    """numpy's argmax: the first maximum."""
    return np.argmax(z, axis=1)


def _top_gap(z):
    s = np.sort(z, axis=1)
    return s[:, -1] - s[:, -2]


def start(net, x, nb_candidate):
    """The state at x: x, r_tot, adv (tensors), orig [B], cand [B, nc] (stable descending order), active [B], logits (NumPy)."""
    with torch.no_grad():
        z = net(x).numpy()
    cand = np.argsort(-z, axis=1, kind="stable")[:, :nb_candidate]
    nan = np.isnan(z).any(axis=1)
    return {"x": x, "r_tot": torch.zeros_like(x), "adv": x.clone(), "orig": _first_argmax(np.where(np.isnan(z), -np.inf, z)), "cand": cand,
            "active": ~nan, "logits": z}


def step(net, state, lo, hi):
    """One iteration from ``state`` (not modified).  Returns (new state, info): jstar [B] (-1: no step), pert [B, nc] (column 0
    unused, +inf), pert_gap [B] and logit_gap [B] (+inf where the image took no step), wnorm [B, nc]."""
    x, cand, orig = state["x"], state["cand"], state["orig"]
    B, nc = cand.shape
    act = state["active"].copy()
    adv = state["adv"].clone().requires_grad_(True)
    z = net(adv)
    ct = torch.as_tensor(cand)
    grads = [torch.autograd.grad(z.gather(1, ct[:, j:j + 1]).sum(), adv, retain_graph=j + 1 < nc)[0] for j in range(nc)]
    zc = z.detach().gather(1, ct)
    f = zc - zc[:, :1]
    w = torch.stack([g - grads[0] for g in grads], dim=1).reshape(B, nc, -1)             # [B, nc, P]
    wn = w.norm(dim=2)
    pert = torch.where(wn > 0, (f.abs() + 1e-5) / wn, torch.full_like(wn, float("inf")))
    pert[:, 0] = float("inf")
    pn = pert.numpy().copy()
    pn[np.isnan(pn)] = np.inf
    jstar = np.where(np.isfinite(pn).any(axis=1) & act, np.argmin(pn, axis=1), -1)
    moved = jstar >= 0
    r_new = state["r_tot"].clone()
    idx = torch.as_tensor(np.maximum(jstar, 0))
    rows = torch.arange(B)
    delta = (pert[rows, idx] / wn[rows, idx]).reshape(B, 1) * w[rows, idx]
    mt = torch.as_tensor(moved)
    r_new[mt] = r_new[mt] + delta[mt].reshape(r_new[mt].shape)
    adv_new = state["adv"].clone()
    adv_new[mt] = torch.clamp(x[mt] + r_new[mt], lo, hi)
    with torch.no_grad():
        z_new = net(adv_new).numpy()
    nan = np.isnan(z_new).any(axis=1) & act
    back = torch.as_tensor(nan & moved)
    r_new[back] = state["r_tot"][back]                              # the NaN rule: the step is taken back
    still = act & moved & ~nan & (_first_argmax(np.where(np.isnan(z_new), -np.inf, z_new)) == orig)
    sp = np.sort(pn, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        pgap = np.where(moved & (nc > 2), (sp[:, 1] - sp[:, 0]) / sp[:, 0], np.inf) if nc > 2 else np.full(B, np.inf)
    pgap = np.where(np.isnan(pgap), np.inf, pgap)
    lgap = np.where(moved & ~nan, _top_gap(z_new), np.inf)
    new = dict(state, r_tot=r_new, adv=adv_new, active=still, logits=z_new)
    return new, {"jstar": jstar.astype(np.int32), "pert": pn, "pert_gap": pgap, "logit_gap": lgap, "wnorm": wn.numpy(), "entered": act}


def finish(net, state, overshoot, lo, hi):
    """(x_adv tensor, r_norm [B], final_class [B], final logits)."""
    x_adv = torch.clamp(state["x"] + (1.0 + overshoot) * state["r_tot"], lo, hi)
    with torch.no_grad():
        z = net(x_adv).numpy()
    r_norm = (x_adv - state["x"]).reshape(x_adv.shape[0], -1).norm(dim=1).numpy()
    return x_adv, r_norm, _first_argmax(np.where(np.isnan(z), -np.inf, z)).astype(np.int32), z


def _cast(state, dtype):
    return dict(state, x=state["x"].to(dtype), r_tot=state["r_tot"].to(dtype), adv=state["adv"].to(dtype))


def run(model, params, x, nb_candidate=10, overshoot=0.02, max_iter=50, lo=0.0, hi=1.0, dtype=torch.float64, shadow=None):
    """The whole loop on x [B,H,W,C] (NumPy).  A dict of NumPy arrays: x_adv, r_tot, r_norm, iters, final_class, orig, cand, choices
    [max_iter, B] (-1: no step), pert_gap, logit_gap [max_iter, B], cand_gap, final_gap [B]; with ``shadow`` pert_err, logit_err (floats)."""
    net = logits_fn(model, params, dtype)
    net_s = logits_fn(model, params, shadow) if shadow is not None else None
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    B = int(xt.shape[0])
    state = start(net, xt, nb_candidate)
    z0 = np.sort(np.where(np.isnan(state["logits"]), -np.inf, state["logits"]), axis=1)[:, ::-1][:, :nb_candidate + 1]
    cand_gap = np.min(z0[:, :-1] - z0[:, 1:], axis=1)
    cand_gap = np.where(np.isnan(cand_gap), 0.0, cand_gap)
    pert_err = logit_err = 0.0
    if net_s is not None:
        with torch.no_grad():
            logit_err = _abs_err(net_s(xt.to(shadow)).numpy(), state["logits"])
    iters = np.zeros(B, np.int32)
    choices = np.full((max_iter, B), -1, np.int32)
    pert_gap, logit_gap = np.full((max_iter, B), np.inf), np.full((max_iter, B), np.inf)
    for k in range(max_iter):
        if not state["active"].any():
            break
        new, info = step(net, state, lo, hi)
        if net_s is not None:
            new_s, info_s = step(net_s, _cast(state, shadow), lo, hi)
            a = info["entered"]
            p64, p32 = info["pert"][a][:, 1:], info_s["pert"][a][:, 1:].astype(np.float64)
            ok = np.isfinite(p64) & np.isfinite(p32)
            if ok.any():
                pert_err = max(pert_err, float(np.max(np.abs(p32[ok] - p64[ok]) / p64[ok])))
            logit_err = max(logit_err, _abs_err(new_s["logits"][a], new["logits"][a]))
        iters += info["entered"].astype(np.int32)
        choices[k], pert_gap[k], logit_gap[k] = info["jstar"], info["pert_gap"], info["logit_gap"]
        state = new
    x_adv, r_norm, final_class, zf = finish(net, state, overshoot, lo, hi)
    if net_s is not None:
        logit_err = max(logit_err, _abs_err(finish(net_s, _cast(state, shadow), overshoot, lo, hi)[3], zf))
    out = {"x_adv": x_adv.numpy(), "r_tot": state["r_tot"].numpy(), "r_norm": r_norm, "iters": iters, "final_class": final_class,
           "orig": state["orig"].astype(np.int32), "cand": state["cand"].astype(np.int32), "choices": choices, "pert_gap": pert_gap,
           "logit_gap": logit_gap, "cand_gap": cand_gap, "final_gap": np.where(np.isnan(zf).any(axis=1), 0.0, _top_gap(zf)),
           "active": state["active"]}
    if net_s is not None:
        out["pert_err"], out["logit_err"] = pert_err, logit_err
    return out


def _abs_err(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def decidable(out):
    """[B] bool: every decision margin of the image's float64 trajectory exceeds 4 x the largest float32-vs-float64 difference of the
    quantity compared (``out`` from ``run(..., shadow=torch.float32)``)."""
    tp, tl = 4.0 * out["pert_err"], 4.0 * out["logit_err"]
    return ((out["pert_gap"] > tp).all(axis=0) & (out["logit_gap"] > tl).all(axis=0) & (out["cand_gap"] > tl) & (out["final_gap"] > tl))


def margin_room(out):
    """[B]: the smallest decision margin of each image over the threshold ``decidable`` holds it to (decidable is room > 1)."""
    tp, tl = 4.0 * out["pert_err"], 4.0 * out["logit_err"]
    return np.minimum.reduce([out["pert_gap"].min(axis=0) / tp, out["logit_gap"].min(axis=0) / tl, out["cand_gap"] / tl, out["final_gap"] / tl])


# ---- the input sets the GPU tests use (tests/test_deepfool_cpu.py asserts that at least 75 % of each are decidable) --------------
def model_of(name, shape=(28, 28, 1)):
    """'F': model F's Conv2D stack, 10 classes; 'lin70': Flatten + Linear(70) + Softmax; 'convlin': Conv + ReLU + Linear(10)."""
    from defensegan_amd import network_builder as nb
    inp = (None,) + tuple(shape)
    if name == "F":
        return nb.model_f(input_shape=inp)
    if name.startswith("lin") and name[3:].isdigit():               # 'lin70', and the edge cases' 'lin5', 'lin300', 'lin2049'
        return nb.MLP([nb.Flatten(), nb.Linear(int(name[3:])), nb.Softmax()], input_shape=inp)
    if name == "convlin":
        return nb.MLP([nb.Conv2D(4, (3, 3), (1, 1), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=inp)
    raise KeyError(name)


def images(B, shape, seed, lo=0.0, hi=1.0):
    """[B, H, W, C] float32 in [lo, hi] ([0, 1] unless given); every third image (0, 3, ...) holds exact lo and hi pixels (about a
    quarter each), so the clip binds."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(lo, hi, (B,) + tuple(shape)).astype(np.float32)
    u = rs.uniform(0.0, 1.0, x.shape)
    sat = np.where(u < 0.25, lo, np.where(u > 0.75, hi, x)).astype(np.float32)
    x[::3] = sat[::3]
    return x


# name -> model, input shape, weight seed, image seed, B, nb_candidate: the whole-run cases (defaults and max_iter = 3 share the inputs)
RUN_CASES = {
    "F28": dict(model="F", shape=(28, 28, 1), clf_seed=70, x_seed=31, B=9, nc=10),
    "lin70": dict(model="lin70", shape=(28, 28, 1), clf_seed=7, x_seed=5, B=65, nc=10),
    "convlin5": dict(model="convlin", shape=(5, 5, 1), clf_seed=5, x_seed=3, B=12, nc=10),
}
# the one-step cases: every B, both vector paths, the lane-strided loops of 70 classes at nb_candidate 2, 10 and 70, model F
STEP_CASES = [("lin70", (28, 28, 1), B, nc) for B in (1, 3, 65) for nc in (2, 10, 70)] + \
             [("lin70", (5, 5, 1), 3, 70), ("convlin", (5, 5, 1), 3, 10), ("F", (28, 28, 1), 3, 10), ("F", (28, 28, 1), 65, 10)]
STEP_SEEDS = dict(clf_seed=17, x_seed=9)


LOGIT_SCALE = 0.05          # on the last layer: small logits keep their float32 error well under the 1e-5 that pert_j adds to |f_j|


def case_inputs(case):
    """(model, params, x) of a RUN_CASES entry (no device touched): bpda_reference.init_params' weights, the last layer scaled by
    LOGIT_SCALE."""
    c = RUN_CASES[case] if isinstance(case, str) else case
    m = model_of(c["model"], c["shape"])
    p = R.init_params(m, c["clf_seed"])
    s = np.float32(c.get("logit_scale", LOGIT_SCALE))
    p[-1] = (p[-1][0] * s, p[-1][1] * s)
    return m, p, clear_images(m, p, c["B"], c["shape"], c["x_seed"], c.get("lo", 0.0), c.get("hi", 1.0), c.get("pool", 4))


MIN_GAP = 0.25              # of the standard deviation of the image's logits


def clear_images(model, params, B, shape, seed, lo=0.0, hi=1.0, pool=4):
    """B of ``images(pool B, ...)`` (pool = 4 unless the case says otherwise), every third still one with exact lo and hi pixels, kept
    in order where the float64 logits at the image have their two largest at least MIN_GAP standard deviations (of that image's logits) apart.  r_tot is proportional to that gap while
    the float32 error of a logit is not, so an image that starts almost on a boundary cannot be held to a relative bound on r_norm in
    float32 at all; tests/test_deepfool_cpu.py asserts that the float32 CPU run meets a quarter of the GPU test's bound on what is kept."""
    n, pool = pool * B, images(pool * B, shape, seed, lo, hi)
    with torch.no_grad():
        z = logits_fn(model, params)(torch.tensor(pool, dtype=torch.float64)).numpy()
    keep = _top_gap(z) >= MIN_GAP * z.std(axis=1)
    sat, free = [i for i in range(0, n, 3) if keep[i]], [i for i in range(n) if i % 3 and keep[i]]
    return np.stack([pool[(sat if i % 3 == 0 else free).pop(0)] for i in range(B)])


_RUNS = {}


def case_run(case, max_iter=50, overshoot=0.02):
    """The float64 run of a RUN_CASES entry with its float32 shadow, computed once and shared (never modified)."""
    key = (case, max_iter, overshoot)
    if key not in _RUNS:
        m, p, x = case_inputs(case)
        _RUNS[key] = run(m, p, x, RUN_CASES[case]["nc"], overshoot, max_iter, 0.0, 1.0, shadow=torch.float32)
    return _RUNS[key]


# ---- the edge cases (tests/test_gpu_deepfool_edges.py; tests/test_deepfool_edges_cpu.py asserts what each choice promises) -----------
# The grid caps of dg_deepfool.hip and the strides that go with them, as text: a test that tiles its images past a cap reaches the
# second loop trip only while the cap stands where it was chosen for (tests/support/strided_cases.CAP_SOURCES' way).
IMAGE_CAP = 65536                    # df_image_grid: one workgroup per image (the step and the final kernel)
WAVE_CAP = 4096 * 4                  # df_wave_grid: 4096 workgroups of 4 images (select, activity, class)
CAP_SOURCES = (("dg_deepfool.hip", "unsigned df_wave_grid(int B) { return (unsigned)((B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096); }"),
               ("dg_deepfool.hip", "unsigned df_image_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }"),
               ("dg_deepfool.hip", "for (long long b = blockIdx.x; b < B; b += gridDim.x) {"),
               ("dg_deepfool.hip", "b += (long long)gridDim.x * 4"),
               ("dg_deepfool.hip", "for (int j = 1 + tid; j < nc; j += 256) {"),
               ("dg_deepfool.hip", "constexpr int DEEPFOOL_MAX_CAND = 2048;"))

TILE_B = IMAGE_CAP + 2               # workgroups 0 and 1 of the image-strided kernels take a second image; the wave-strided make 5 trips
# the base sets that are tiled to TILE_B: 67 images, 65536 % 67 == 10, so workgroup 0 sees base image 0 (a NaN pixel: inactive) and then
# base image 10, workgroup 1 base images 1 and 11; 4 x 4 is the float4 path, 3 x 3 (P = 9) the scalar one
TILE_CASES = {
    "tile4x4": dict(model="lin5", shape=(4, 4, 1), clf_seed=11, x_seed=2, B=67, nc=3, max_iter=4),
    "tile3x3": dict(model="lin5", shape=(3, 3, 1), clf_seed=12, x_seed=3, B=67, nc=3, max_iter=4),
}
# many candidates: pass 2's candidate stride takes its second trip at nc >= 258; DEEPFOOL_MAX_CAND = 2048 is the last nc that runs
MANY_STEP_CASES = [("lin300", (28, 28, 1), 3, 257), ("lin300", (28, 28, 1), 3, 258), ("lin300", (28, 28, 1), 3, 300),
                   ("lin2049", (4, 4, 1), 2, 2048)]
# (with hundreds of classes few images have their two largest logits MIN_GAP apart: a wider pool to keep from.  The seeds were
# searched on the CPU for margins at least twice what ``decidable`` asks: at 2049 classes on 16 pixels the smallest gap between two
# neighbouring logits is of the order of four float32 errors, and a draw that clears the bar by a hair on one CPU misses it on another)
MANY_SEEDS = {"lin300": dict(clf_seed=17, x_seed=1, pool=16), "lin2049": dict(clf_seed=135, x_seed=2468, pool=64)}
MANY_RUN = dict(model="lin300", shape=(28, 28, 1), clf_seed=17, x_seed=1, pool=16, B=3, nc=300, max_iter=50)
# a signed range: images in [-1, 1], every third saturated at exactly -1 and +1, clipped to [-1, 1]
SIGNED_CASE = dict(model="lin10", shape=(4, 4, 1), clf_seed=21, x_seed=6, B=24, nc=10, max_iter=50, lo=-1.0, hi=1.0)


def tile_inputs(name):
    """(model, params, x [67, ...]) of a TILE_CASES entry: case_inputs' draw, then one NaN pixel in image 0."""
    m, p, x = case_inputs(TILE_CASES[name])
    x = x.copy()
    x[0].reshape(-1)[1] = np.nan
    return m, p, x


def edge_run(key, m, p, x, c, overshoot=0.02):
    """The float64 run with its float32 shadow of an edge case ``c`` on ``x``, computed once per ``key`` and shared (never modified)."""
    if key not in _RUNS:
        _RUNS[key] = run(m, p, x, c["nc"], overshoot, c["max_iter"], c.get("lo", 0.0), c.get("hi", 1.0), shadow=torch.float32)
    return _RUNS[key]


# The NaN take-back: a model and an image whose logits are finite at x while the first step lands where float32 overflows.  u and v are
# orthonormal directions of the 16 pixels, t = u . x, q = v . x.  Three Linear layers, no ReLU between them:
#     h1 = (S t, S t, 1e3 q),   h2 = (S h1_0, S h1_1, 1e3 h1_2),   S^2 = 1.5e38:  h2_0 = h2_1 = 1.5e38 t is finite below t = 2.27
#     Z_0 = 4.5e6 - 0.5e6 t,    Z_1 = 1e6 t,    Z_2 = 2e6 q + W (h2_0 - h2_1),    W = 1e6 / 1.5e38
# At t = 2, q = 0: Z = (3.5e6, 2e6, 0), orig = 0, pert_1 = 1.5e6 / 1.5e6 = 1 along u, pert_2 = 3.5e6 / 2.06e6 = 1.7: the step takes t to 3,
# where h2_0 = h2_1 = 4.5e38 overflows to +inf and Z_2 subtracts the two infinities.  The seeds' way back multiplies 6.7e-33 by
# 1.2e19 twice: every partial product is a normal float32 number.  The neighbours have q = 1.5: Z_2 = 3e6 is their nearest boundary,
# 0.24 away, and t moves by 0.06 only.
TAKEBACK_S = 1.2247449e19


def takeback_case():
    """(model, params float32, x [3, 4, 4, 1] float32): image 1 is the one whose first step overflows; images 0 and 2 are ordinary."""
    from defensegan_amd import network_builder as nb
    m = nb.MLP([nb.Flatten(), nb.Linear(3), nb.Linear(3), nb.Linear(3), nb.Softmax()], input_shape=(None, 4, 4, 1))
    u = np.full(16, 0.25)
    v = np.concatenate([np.full(8, 0.25), np.full(8, -0.25)])
    S = TAKEBACK_S
    W1 = np.stack([S * u, S * u, 1e3 * v], axis=1)
    W2 = np.diag([S, S, 1e3])
    w = 1e6 / 1.5e38
    W3 = np.array([[-0.25 * w, 0.5 * w, w], [-0.25 * w, 0.5 * w, -w], [0.0, 0.0, 2.0]])
    p = [(W1.astype(np.float32), np.zeros(3, np.float32)), (W2.astype(np.float32), np.zeros(3, np.float32)),
         (W3.astype(np.float32), np.array([4.5e6, 0.0, 0.0], np.float32))]
    rs = np.random.RandomState(8)
    x = np.empty((3, 16), np.float32)
    x[1] = 0.5 + rs.uniform(-0.02, 0.02, 16)
    for i in (0, 2):
        x[i] = np.concatenate([np.full(8, 0.875), np.full(8, 0.125)]) + rs.uniform(-0.02, 0.02, 16)
    return m, p, x.reshape(3, 4, 4, 1)
