"""CPU restatement of the Jacobian saliency-map attack ("Saliency map"), written from the definition and
independently of the device code (defensegan_amd/csrc/dg_jsma.hip, attacks.SaliencyMapMethod): torch on the CPU, float64 by default,
the two gradients from autograd.

    out = run(model, params, x, target, theta, max_iters, lo, hi, of_probs)          # the whole loop, float64
    out = run(..., shadow=torch.float32)                                             # with the margins' float32 yardstick
    p, q, best, second, S = pair_choice(a, b, dom, theta)                            # step 3 for one image

The definition, per image:  adv = x;  dom = x < hi (theta > 0) or x > lo (theta < 0);  active.  One iteration of an active image:
O = the logits at adv, or softmax(logits) with of_probs; inactive when the first arg-max of O (a NaN never a candidate) is the target,
when O holds a NaN or when fewer than 2 features are in dom;  a = grad O[t], b = grad sum_{j != t} O[j];  over the pairs p < q in dom,
A = a_p + a_q, Bs = b_p + b_q, admissible where A > 0 and Bs < 0 (theta < 0: A < 0 and Bs > 0), the admissible pair of the largest
-(A Bs) > 0 is taken, ties to the smallest p, then q; without one the image becomes inactive;  adv[p] = clip(adv[p] + theta), the same
for q; both leave dom.  x_adv = adv, final_class = the first arg-max of the logits at x_adv, n_changed = the elements with x_adv != x
(a NaN element of x is not counted).

``run`` records the DECISION MARGINS of its trajectory, per image and iteration: ``score_gap`` -- the best admissible score minus the
second best (0 where there is no second: the gap to taking no step) --, ``score_margin`` = score_gap / best, and ``out_gap`` -- the
gap between the two largest outputs, the margin of the activity arg-max --, plus ``final_gap`` (the two largest logits at x_adv).
With ``shadow=torch.float32`` every iteration is ALSO taken in float32 from the same float64 state and the float32-vs-float64
difference of each quantity compared is recorded beside its margin: ``score_err`` (the largest absolute difference over the whole
table of scores, an inadmissible pair scoring 0, so that a sign test that flips counts in full), ``out_err`` and ``final_err``.
``decidable(out)`` marks the images every margin of which exceeds 4 x that difference -- deepfool_reference.decidable's rule; the
factor leaves room for the device's different summation order."""
import numpy as np
import torch

from tests.support import bpda_reference as R
from tests.support.deepfool_reference import logits_fn


def pair_choice(a, b, dom, theta):
    """Step 3 for one image: a, b [F], dom [F] bool.  (p, q, best, second, S): the pair (-1, -1 without an admissible pair of score
    > 0), its score, the second largest admissible score (0 without one) and the [D, D] table of scores over the compacted domain
    (0 where inadmissible or not p < q; None when D < 2)."""
    idx = np.flatnonzero(dom)
    D = len(idx)
    if D < 2:
        return -1, -1, 0.0, 0.0, None
    with np.errstate(invalid="ignore", over="ignore"):
        A = a[idx][:, None] + a[idx][None, :]
        Bs = b[idx][:, None] + b[idx][None, :]
        adm = ((A > 0) & (Bs < 0)) if theta > 0 else ((A < 0) & (Bs > 0))
        S = np.where(adm & np.triu(np.ones((D, D), bool), 1), -(A * Bs), 0.0)
    S = np.where(np.isnan(S), 0.0, S)                              # a NaN score is never larger
    flat = int(np.argmax(S))                                       # the first maximum in row-major order: smallest p, then q
    best = float(S.flat[flat])
    if not best > 0:
        return -1, -1, 0.0, 0.0, S
    rest = S.copy()
    rest.flat[flat] = 0.0
    return int(idx[flat // D]), int(idx[flat % D]), best, float(rest.max()), S


def cleverhans_pair(a, b, dom, theta):
    """cleverhans' jsma_symbolic, literally, for one image: the [F, F] tables with the features outside the domain shifted by
    increase_coef * max|.| (increase_coef = +-2), the diagonal zeroed, the first arg-max of the flat index."""
    F = len(a)
    increase = theta > 0
    coef = (4 * int(increase) - 2) * (~dom).astype(a.dtype)
    ta = a - coef * np.abs(a).max()
    tb = b + coef * np.abs(b).max()
    A = ta[:, None] + ta[None, :]
    Bs = tb[:, None] + tb[None, :]
    mask = ((A > 0) & (Bs < 0)) if increase else ((A < 0) & (Bs > 0))
    scores = mask.astype(a.dtype) * (-A * Bs) * (1 - np.eye(F, dtype=a.dtype))
    best = int(np.argmax(scores.reshape(-1)))
    return best // F, best % F


def _top_gap(z):
    s = np.sort(np.where(np.isnan(z), -np.inf, z), axis=1)
    return s[:, -1] - s[:, -2]


def _first_argmax(z):
    return np.argmax(np.where(np.isnan(z), -np.inf, z), axis=1)


def _outputs(net, x, of_probs):
    z = net(x)
    return torch.softmax(z, dim=1) if of_probs else z


def start(x, theta, lo, hi):
    """The state at x [B,H,W,C] (tensor): x, adv, dom [B, F] bool, active [B]."""
    xf = x.reshape(x.shape[0], -1).numpy()
    with np.errstate(invalid="ignore"):
        dom = (xf < hi) if theta > 0 else (xf > lo)
    return {"x": x, "adv": x.clone(), "dom": dom, "active": np.ones(x.shape[0], bool)}


def gradients(net, adv, target, of_probs):
    """(O [B, n] NumPy, a, b [B, F] NumPy) at adv: a = grad O[t], b = grad sum_{j != t} O[j]."""
    adv = adv.clone().requires_grad_(True)
    O = _outputs(net, adv, of_probs)
    hot = torch.zeros_like(O)
    hot[torch.arange(O.shape[0]), torch.as_tensor(target, dtype=torch.long)] = 1
    ga = torch.autograd.grad((O * hot).sum(), adv, retain_graph=True)[0]
    gb = torch.autograd.grad((O * (1 - hot)).sum(), adv)[0]
    B = O.shape[0]
    return O.detach().numpy(), ga.reshape(B, -1).numpy(), gb.reshape(B, -1).numpy()


def step(net, state, target, theta, lo, hi, of_probs):
    """One iteration from ``state`` (not modified).  Returns (new state, info): pair [B, 2] (-1: no step), best, second [B], S (list
    of tables or None), O [B, n], entered [B] (active when the iteration began), out_gap [B] (+inf where not entered)."""
    B = state["x"].shape[0]
    O, a, b = gradients(net, state["adv"], target, of_probs)
    nan = np.isnan(O).any(axis=1)
    entered = state["active"].copy()
    act = entered & ~nan & (_first_argmax(O) != target) & (state["dom"].sum(axis=1) >= 2)
    adv = state["adv"].clone()
    flat = adv.reshape(B, -1)
    dom = state["dom"].copy()
    pair = np.full((B, 2), -1, np.int32)
    best, second, tables = np.zeros(B), np.zeros(B), [None] * B
    for i in np.flatnonzero(act):
        p, q, best[i], second[i], tables[i] = pair_choice(a[i], b[i], dom[i], theta)
        if p < 0:
            act[i] = False
            continue
        for f in (p, q):
            flat[i, f] = torch.clamp(flat[i, f] + theta, lo, hi)
            dom[i, f] = False
        pair[i] = (p, q)
    with np.errstate(invalid="ignore"):
        out_gap = np.where(entered & ~nan, _top_gap(O), np.inf)
    new = dict(state, adv=adv, dom=dom, active=act)
    return new, {"pair": pair, "best": best, "second": second, "S": tables, "O": O, "entered": entered, "searched": pair[:, 0] >= 0,
                 "out_gap": out_gap}


def run(model, params, x, target, theta=1.0, max_iters=None, lo=0.0, hi=1.0, of_probs=True, gamma=1.0, dtype=torch.float64, shadow=None):
    """The whole loop on x [B,H,W,C] (NumPy), target [B].  A dict of NumPy arrays: x_adv, iters, final_class, n_changed, choices
    [max_iters, B, 2] (-1: no step), score_gap, score_margin, out_gap [max_iters, B], final_gap [B]; with ``shadow`` score_err, out_err
    [max_iters, B] and final_err [B]."""
    net = logits_fn(model, params, dtype)
    net_s = logits_fn(model, params, shadow) if shadow is not None else None
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    B, F = int(xt.shape[0]), int(xt[0].numel())
    if max_iters is None:
        max_iters = int(np.floor(F * gamma / 2))
    target = np.asarray(target, np.int64)
    state = start(xt, theta, lo, hi)
    iters = np.zeros(B, np.int32)
    choices = np.full((max_iters, B, 2), -1, np.int32)
    score_gap, out_gap = np.full((max_iters, B), np.inf), np.full((max_iters, B), np.inf)
    score_margin = np.full((max_iters, B), np.inf)
    score_err, out_err = np.zeros((max_iters, B)), np.zeros((max_iters, B))
    for k in range(max_iters):
        if not state["active"].any():
            break
        new, info = step(net, state, target, theta, lo, hi, of_probs)
        ent = info["entered"]
        out_gap[k] = info["out_gap"]
        for i in np.flatnonzero(ent):
            if info["S"][i] is not None:                           # the image went through the pair search
                score_gap[k, i] = info["best"][i] - info["second"][i]
                score_margin[k, i] = score_gap[k, i] / info["best"][i] if info["best"][i] > 0 else np.inf
        if net_s is not None:
            st = dict(state, x=state["x"].to(shadow), adv=state["adv"].to(shadow))
            _, info_s = step(net_s, st, target, theta, lo, hi, of_probs)
            with np.errstate(invalid="ignore"):
                d = np.abs(info_s["O"].astype(np.float64) - info["O"])
            out_err[k] = np.where(ent, np.where(np.isnan(d), 0.0, d).max(axis=1), 0.0)
            for i in np.flatnonzero(ent):
                S, S32 = info["S"][i], info_s["S"][i]
                if S is not None and S32 is not None:
                    score_err[k, i] = float(np.abs(S32.astype(np.float64) - S).max())
                elif (S is None) != (S32 is None):                 # float32 searched where float64 did not, or the reverse
                    score_err[k, i] = np.inf
        iters += info["searched"].astype(np.int32)
        choices[k] = info["pair"]
        state = new
    x_adv = state["adv"]
    with torch.no_grad():
        zf = net(x_adv).numpy()
    xa, x0 = x_adv.numpy(), xt.numpy()
    with np.errstate(invalid="ignore"):
        n_changed = ((xa != x0) & ~np.isnan(x0)).reshape(B, -1).sum(axis=1).astype(np.int32)
    out = {"x_adv": xa, "iters": iters, "final_class": _first_argmax(zf).astype(np.int32), "n_changed": n_changed, "choices": choices,
           "score_gap": score_gap, "score_margin": score_margin, "out_gap": out_gap, "final_gap": np.where(np.isnan(zf).any(axis=1), 0.0, _top_gap(zf)),
           "target": target.astype(np.int32), "active": state["active"]}
    if net_s is not None:
        with torch.no_grad():
            d = np.abs(net_s(x_adv.to(shadow)).numpy().astype(np.float64) - zf)
        out.update(score_err=score_err, out_err=out_err, final_err=np.where(np.isnan(d), 0.0, d).max(axis=1))
    return out


def decidable(out):
    """[B] bool: every decision margin of the image's float64 trajectory exceeds 4 x the float32-vs-float64 difference of the quantity
    compared (``out`` from ``run(..., shadow=torch.float32)``).  A search that found no pair in either precision (gap 0, difference 0)
    is a decision both took."""
    sg, se = out["score_gap"], out["score_err"]
    return (((sg > 4.0 * se) | ((sg == 0) & (se == 0))).all(axis=0) & (out["out_gap"] > 4.0 * out["out_err"]).all(axis=0) &
            (out["final_gap"] > 4.0 * out["final_err"]))


# ---- the input sets the CPU and the GPU tests share (tests/test_jsma_cpu.py asserts that at least 75 % of each are decidable) ---------
def model_of(name, shape=(28, 28, 1)):
    """'mlpN': Flatten + Linear(32) + ReLU + Linear(N) + Softmax, the two-layer ReLU model; 'linN': Flatten + Linear(N) + Softmax;
    'F': model F's Conv2D stack, 10 classes."""
    from defensegan_amd import network_builder as nb
    inp = (None,) + tuple(shape)
    if name == "F":
        return nb.model_f(input_shape=inp)
    if name.startswith("mlp"):
        return nb.MLP([nb.Flatten(), nb.Linear(32), nb.ReLU(), nb.Linear(int(name[3:])), nb.Softmax()], input_shape=inp)
    if name.startswith("lin"):
        return nb.MLP([nb.Flatten(), nb.Linear(int(name[3:])), nb.Softmax()], input_shape=inp)
    raise KeyError(name)


def images(B, shape, seed):
    """[B, H, W, C] float32, x ~ 0.5 U[0, 1): every feature starts inside the search domain of either sign of theta (a zero aside)."""
    return (0.5 * np.random.RandomState(seed).uniform(0.0, 1.0, (B,) + tuple(shape))).astype(np.float32)


def targets(model, params, x, seed):
    """[B] int32: (the float64 first arg-max at x + 1 + r) % n, r drawn per image from RandomState(seed): never the image's own class."""
    with torch.no_grad():
        z = logits_fn(model, params)(torch.tensor(x, dtype=torch.float64)).numpy()
    n = z.shape[1]
    r = np.random.RandomState(seed).randint(0, n - 1, len(x))
    return ((_first_argmax(z) + 1 + r) % n).astype(np.int32)


def case_inputs(c):
    """(model, params, x, target) of a case dict (no device touched): bpda_reference.init_params' weights."""
    m = model_of(c["model"], c["shape"])
    p = R.init_params(m, c["clf_seed"])
    x = images(c["B"], c["shape"], c["x_seed"])
    return m, p, x, targets(m, p, x, c["x_seed"] + 1)


def _case(model, shape, B, theta=1.0, of_probs=1, gamma=1.0, clf_seed=17, x_seed=9, max_iters=None):
    return dict(model=model, shape=shape, B=B, theta=theta, of_probs=of_probs, gamma=gamma, clf_seed=clf_seed, x_seed=x_seed, max_iters=max_iters)


# the one-iteration cases: 4 x 4 (one float4 per thread, most threads idle), 5 x 5 (F % 4 != 0: the scalar path), 28 x 28 (the float4
# path), every B, 10 and 70 classes, both outputs, the three thetas, model F once
STEP_CASES = [_case("mlp10", s, B, max_iters=1) for s in ((4, 4, 1), (5, 5, 1), (28, 28, 1)) for B in (1, 3, 65)] + [
    _case("mlp70", (28, 28, 1), 3, of_probs=0, max_iters=1), _case("mlp70", (5, 5, 1), 3, max_iters=1),
    _case("mlp10", (4, 4, 1), 65, of_probs=0, max_iters=1), _case("mlp10", (28, 28, 1), 3, theta=-1.0, of_probs=0, max_iters=1),
    _case("mlp10", (5, 5, 1), 3, theta=-1.0, max_iters=1), _case("mlp10", (4, 4, 1), 3, theta=0.25, of_probs=0, max_iters=1),
    _case("mlp70", (28, 28, 1), 3, theta=0.25, max_iters=1), _case("F", (28, 28, 1), 3, of_probs=0, clf_seed=70, max_iters=1)]
# the whole runs: gamma 1.0 at F = 16 and 25, gamma 0.1 at F = 784; 'F28' is model F on its logits (the success figures)
RUN_CASES = {
    "r16": _case("mlp10", (4, 4, 1), 24, of_probs=0, clf_seed=3, x_seed=4),
    "r16p": _case("mlp10", (4, 4, 1), 24, theta=0.25, of_probs=1, clf_seed=3, x_seed=5),
    "r25": _case("mlp70", (5, 5, 1), 16, theta=-1.0, of_probs=0, clf_seed=5, x_seed=6),
    "r784": _case("mlp10", (28, 28, 1), 8, of_probs=0, gamma=0.1, clf_seed=7, x_seed=8),
    "r784p": _case("mlp10", (28, 28, 1), 8, of_probs=1, gamma=0.1, clf_seed=7, x_seed=8),
    "F28": _case("F", (28, 28, 1), 8, of_probs=0, gamma=0.1, clf_seed=70, x_seed=31),
}

_RUNS = {}


def case_run(c):
    """The float64 run of a case (a RUN_CASES name or a case dict) with its float32 shadow, computed once and shared (never modified)."""
    c = RUN_CASES[c] if isinstance(c, str) else c
    key = tuple(sorted((k, str(v)) for k, v in c.items()))
    if key not in _RUNS:
        m, p, x, t = case_inputs(c)
        _RUNS[key] = run(m, p, x, t, c["theta"], c["max_iters"], 0.0, 1.0, bool(c["of_probs"]), c["gamma"], shadow=torch.float32)
    return _RUNS[key]


def float32_run(c):
    """The same case run in float32 throughout: the trajectory a float32 implementation takes where nothing is close."""
    c = RUN_CASES[c] if isinstance(c, str) else c
    m, p, x, t = case_inputs(c)
    return run(m, p, x, t, c["theta"], c["max_iters"], 0.0, 1.0, bool(c["of_probs"]), c["gamma"], dtype=torch.float32)


# ---- the tiled case (the second trips of the image- and wave-strided loops): a linear model on 4 x 4, two iterations ---------------
IMAGE_CAP = 65536                    # jsma_image_grid: one workgroup per image (init, pair and final kernels)
WAVE_CAP = 4096 * 4                  # jsma_wave_grid: 4096 workgroups of 4 images (activity and class kernels)
CAP_SOURCES = (("dg_jsma.hip", "unsigned jsma_wave_grid(int B) { return (unsigned)((B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096); }"),
               ("dg_jsma.hip", "unsigned jsma_image_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }"),
               ("dg_jsma.hip", "for (long long b = blockIdx.x; b < B; b += gridDim.x) {"),
               ("dg_jsma.hip", "b += (long long)gridDim.x * 4"),
               ("dg_jsma.hip", "constexpr int JSMA_MAX_FEATURES = 5120;"))
TILE_B = IMAGE_CAP + 2
TILE_CASE = _case("lin5", (4, 4, 1), 67, of_probs=0, clf_seed=11, x_seed=2, max_iters=2)


# ---- the edge cases (tests/test_gpu_jsma_edges.py on the device, tests/test_jsma_edges_cpu.py for what each set was chosen for) ------
def sparse_images(B, shape, seed, lo=0.0, hi=1.0):
    """[B, H, W, C] float32, MNIST-like: per element, with u ~ U[0, 1) and then v ~ U[lo, hi) from RandomState(seed), lo where u < 0.45,
    hi where 0.45 <= u < 0.6, otherwise v.  theta > 0 finds about 85 % of the features in the search domain, theta < 0 about 55 %."""
    rs = np.random.RandomState(seed)
    u = rs.uniform(0.0, 1.0, (B,) + tuple(shape))
    v = rs.uniform(lo, hi, (B,) + tuple(shape))
    return np.where(u < 0.45, lo, np.where(u < 0.6, hi, v)).astype(np.float32)


def conv_model(shape):
    """Conv2D(8, 3 x 3, stride 1, SAME) + ReLU + Flatten + Linear(10) + Softmax: the model of the channel cases."""
    from defensegan_amd import network_builder as nb
    return nb.MLP([nb.Conv2D(8, (3, 3), (1, 1), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(10), nb.Softmax()], input_shape=(None,) + tuple(shape))


def pair_chunk(F):
    """The features per thread of jsma_pair_kernel's compaction when x is 16-byte aligned: ceil(F / 256) rounded up to the vector width."""
    V = 4 if F % 4 == 0 else 1
    return -(-(-(-F // 256)) // V) * V


TIE_BIAS = 1.0e5                     # class 0's bias in the linear tie models: no image reaches its target (the CPU test has the margin)
TIE_ITERS = 6
TIE_SHAPES = {16: (4, 4, 1), 25: (5, 5, 1), 784: (28, 28, 1), 1025: (25, 41, 1), 1300: (26, 50, 1), 3072: (32, 32, 3), 5120: (64, 80, 1)}
TIE_CHUNKS = {16: 4, 25: 1, 784: 4, 1025: 5, 1300: 8, 3072: 12, 5120: 20}
TIE_THETAS = (1.0, -0.5)
TIE_PATTERNS = ("full", "last_two", "first_and_last", "three", "every_third", "wave0_empty", "odd_threads", "thirteen")


def tie_domains(F):
    """The domain patterns of the all-ties family, in TIE_PATTERNS' order: sorted index arrays.  'wave0_empty' leaves out everything
    threads 0 .. 63 of the pair kernel own (nothing is left at F <= 64 chunk: that image takes no step), 'odd_threads' keeps the chunks
    of the odd threads."""
    c, idx = pair_chunk(F), np.arange(F)
    return [idx, idx[-2:], idx[[0, F - 1]], idx[[1, F // 2, F - 2]], idx[::3], idx[idx >= 64 * c], idx[(idx // c) % 2 == 1],
            np.unique(np.linspace(0, F - 1, 13).astype(np.int64))]


def tie_case(F, theta, lo=0.0, hi=1.0):
    """(model, params, x [8, H, W, C], target, doms) of the all-ties family: two classes, the target's column sign(theta) everywhere and
    the other column -sign(theta), so a = sign(theta), b = -sign(theta) and every pair in the domain is admissible at score 4.0; a
    feature in the domain starts a quarter of the range inside it, one outside at the bound that excludes it."""
    m = model_of("lin2", TIE_SHAPES[F])
    s = 1.0 if theta > 0 else -1.0
    W = np.stack([np.full(F, -s), np.full(F, s)], axis=1).astype(np.float32)
    doms = tie_domains(F)
    x = np.full((len(doms), F), hi if theta > 0 else lo, np.float32)
    for i, d in enumerate(doms):
        x[i, d] = lo + 0.25 * (hi - lo) if theta > 0 else hi - 0.25 * (hi - lo)
    return m, [(W, np.array([TIE_BIAS, 0.0], np.float32))], x.reshape((len(doms),) + TIE_SHAPES[F]), np.ones(len(doms), np.int32), doms


def tie_expected(x, doms, theta, max_iters, lo=0.0, hi=1.0):
    """What the all-ties family must give, from the patterns alone: step k of image i moves (d[2k], d[2k + 1]) of its sorted domain."""
    B = len(doms)
    xa = x.reshape(B, -1).copy()
    choices = np.full((max_iters, B, 2), -1, np.int32)
    iters = np.zeros(B, np.int32)
    for i, d in enumerate(doms):
        iters[i] = min(max_iters, len(d) // 2)
        for k in range(iters[i]):
            choices[k, i] = d[2 * k:2 * k + 2]
        moved = d[:2 * iters[i]]
        xa[i, moved] = np.clip(xa[i, moved] + np.float32(theta), np.float32(lo), np.float32(hi))
    return {"x_adv": xa.reshape(x.shape), "iters": iters, "n_changed": 2 * iters, "final_class": np.zeros(B, np.int32), "choices": choices}


# the dyadic family: weights k / 8, |k| <= DYADIC_K <= 16, so every sum and product of the pair rule is exact in float32 and float64
DYADIC_K = 2
DYADIC_SHAPES = {25: (5, 5, 1), 784: (28, 28, 1), 1300: (26, 50, 1)}
DYADIC_ITERS = 8
DYADIC_CASES = [(F, n, theta) for F in sorted(DYADIC_SHAPES) for n in (2, 3) for theta in (1.0, -1.0, 0.25)]


def dyadic_case(F, n, theta, B=6, lo=0.0, hi=1.0):
    """(model, params, x, target): a linear model of dyadic weights with class 0's bias TIE_BIAS, targets among the other classes, half
    of every image outside the search domain at random positions.  The weights are k / 8, k uniform in [-DYADIC_K, DYADIC_K].  At F = 25
    that draw leaves few ties among a dozen features, so there every row is one of three types, (a, b) = (2, 0), (0, -2) or (1, -1)
    eighths times sign(theta) for target 1: the best pairs, at score 4 / 64, are one of the first with one of the second type or two
    of the third -- no product set, so "the smallest p, then q" and "the smallest q, then p" name different pairs."""
    rs = np.random.RandomState(1000 * n + F + (7 if theta < 0 else 0))
    if F == 25:
        ab = np.array([(2, 0), (0, -2), (1, -1)])[rs.randint(0, 3, F)] * (1 if theta > 0 else -1)
        W = np.zeros((F, n))
        W[:, 1] = ab[:, 0]
        if n == 3:
            W[:, 2] = rs.randint(-1, 2, F)
        W[:, 0] = ab[:, 1] - W[:, 2:].sum(axis=1)
        W = (W / 8.0).astype(np.float32)
    else:
        W = (rs.randint(-DYADIC_K, DYADIC_K + 1, (F, n)) / 8.0).astype(np.float32)
    b = np.zeros(n, np.float32)
    b[0] = TIE_BIAS
    x = images(B, DYADIC_SHAPES[F], int(rs.randint(1 << 30))).reshape(B, F)
    x[rs.uniform(0.0, 1.0, (B, F)) < 0.5] = hi if theta > 0 else lo
    t = rs.randint(1, n, B).astype(np.int32)
    return model_of("lin%d" % n, DYADIC_SHAPES[F]), [(W, b)], x.reshape((B,) + DYADIC_SHAPES[F]), np.ones_like(t) if F == 25 else t


def dyadic_run(F, n, theta):
    """The float64 run of a dyadic case, computed once and shared (never modified).  No shadow: nothing in it rounds."""
    if ("dyadic", F, n, theta) not in _RUNS:
        m, p, x, t = dyadic_case(F, n, theta)
        _RUNS[("dyadic", F, n, theta)] = run(m, p, x, t, theta, DYADIC_ITERS, 0.0, 1.0, False)
    return _RUNS[("dyadic", F, n, theta)]


def linear_margins(params, x, target, choices, theta, lo=0.0, hi=1.0):
    """[iterations taken + 1, B] float64: logit 0 minus the largest other logit of a linear model at x and after every step of
    ``choices`` replayed in float64 (rows past the last step of an image repeat its last value)."""
    W, b = np.asarray(params[0][0], np.float64), np.asarray(params[0][1], np.float64)
    adv = np.asarray(x, np.float64).reshape(len(x), -1).copy()
    out = []
    for k in range(len(choices) + 1):
        z = adv @ W + b
        out.append(z[:, 0] - z[:, 1:].max(axis=1))
        if k < len(choices):
            for i in np.flatnonzero(choices[k][:, 0] >= 0):
                pq = choices[k][i]
                adv[i, pq] = np.clip(adv[i, pq] + theta, lo, hi)
    return np.array(out)


def replay(x, choices, theta, lo, hi):
    """x with the features of ``choices`` [iters, B, 2] moved in float32, one add and one clip each: what x_adv must be, bit for bit."""
    xa = np.array(x, np.float32).reshape(len(x), -1)
    for k in range(len(choices)):
        for i in np.flatnonzero(choices[k][:, 0] >= 0):
            pq = choices[k][i]
            xa[i, pq] = np.clip(xa[i, pq] + np.float32(theta), np.float32(lo), np.float32(hi))
    return xa.reshape(np.shape(x))


def _edge(model, shape, B, clf_seed, x_seed, t_seed, theta, max_iters, of_probs, lo=0.0, hi=1.0, sparse=True, outside=False):
    return dict(model=model, shape=shape, B=B, clf_seed=clf_seed, x_seed=x_seed, t_seed=t_seed, theta=theta, max_iters=max_iters,
                of_probs=of_probs, lo=lo, hi=hi, sparse=sparse, outside=outside)


INF = float("inf")
OUTSIDE_SEEDS = (29, 30)             # clf and x seed of the two images that start outside [0, 1]
EDGE_CASES = {}
for _th in (1.0, -1.0, 0.5):         # 2. sparse domains on the two-layer model, 28 x 28
    for _pr in (0, 1):
        EDGE_CASES["sparse_th%g_p%d" % (_th, _pr)] = _edge("mlp10", (28, 28, 1), 8, 7, 21, 22, _th, 20, _pr)
for _th in (0.5, -0.5):              # 3. clip ranges, 5 x 6
    EDGE_CASES["signed_th%g" % _th] = _edge("mlp10", (5, 6, 1), 16, 7, 23, 24, _th, 15, 0, -1.0, 1.0)
    EDGE_CASES["unbounded_th%g" % _th] = _edge("mlp10", (5, 6, 1), 16, 7, 23, 24, _th, 15, 0, -INF, INF)
    EDGE_CASES["point_th%g" % _th] = _edge("mlp10", (5, 6, 1), 16, 7, 23, 24, _th, 15, 0, 0.5, 0.5)
    EDGE_CASES["outside_th%g" % _th] = _edge("mlp10", (5, 6, 1), 2, OUTSIDE_SEEDS[0], OUTSIDE_SEEDS[1], 24, _th, 15, 0, 0.0, 1.0, outside=True)
for _sh in ((6, 5, 3), (4, 6, 3)):   # 4. channels and non-square images: gamma 0.5
    for _pr in (0, 1):
        EDGE_CASES["conv%dx%dx%d_p%d" % (_sh + (_pr,))] = _edge("conv8", _sh, 12, 9, 25, 26, 1.0, int(np.prod(_sh)) // 4, _pr, sparse=False)
for _pr in (0, 1):                   # 5. many classes: four trips of the 64 lanes
    EDGE_CASES["mlp200_p%d" % _pr] = _edge("mlp200", (5, 5, 1), 6, 5, 27, 28, 1.0, 6, _pr, sparse=False)
SPARSE_CASES = sorted(k for k in EDGE_CASES if k.startswith("sparse"))
RANGE_CASES = sorted(k for k in EDGE_CASES if k[:5] in ("signe", "unbou", "point", "outsi"))
CONV_CASES = sorted(k for k in EDGE_CASES if k.startswith("conv"))
MANY_CLASS_CASES = sorted(k for k in EDGE_CASES if k.startswith("mlp200"))


def edge_inputs(name):
    """(model, params, x, target) of an EDGE_CASES entry (no device touched).  The images that start outside the range: elements 3,
    11 and 20 of image 0 and 5, 17 and 26 of image 1 are 1.5, -0.5, 1.5."""
    c = EDGE_CASES[name]
    m = conv_model(c["shape"]) if c["model"] == "conv8" else model_of(c["model"], c["shape"])
    p = R.init_params(m, c["clf_seed"])
    finite = [v if np.isfinite(v) else s for v, s in ((c["lo"], -1.0), (c["hi"], 1.0))]
    if c["lo"] == c["hi"]:
        finite = [-1.0, 1.0]                                        # the images of the signed range around the single point
    x = sparse_images(c["B"], c["shape"], c["x_seed"], *finite) if c["sparse"] else images(c["B"], c["shape"], c["x_seed"])
    if c["outside"]:
        for i, at in enumerate(((3, 11, 20), (5, 17, 26))):
            x[i].reshape(-1)[list(at)] = (1.5, -0.5, 1.5)
    return m, p, x, targets(m, p, x, c["t_seed"])


def edge_run(name):
    """The float64 run of an EDGE_CASES entry with its float32 shadow, computed once and shared (never modified)."""
    if ("edge", name) not in _RUNS:
        c = EDGE_CASES[name]
        m, p, x, t = edge_inputs(name)
        _RUNS[("edge", name)] = run(m, p, x, t, c["theta"], c["max_iters"], c["lo"], c["hi"], bool(c["of_probs"]), shadow=torch.float32)
    return _RUNS[("edge", name)]


# 6. an infinite pixel: three classes on 4 x 4, dyadic weights none of which is zero (0 x inf would be a NaN logit), no bias.  Feature 5's
# row is (1, -2, 3) / 8, so +inf there makes the logits (inf, -inf, inf) -- the first arg-max is class 0, the target 2 ties with it and
# does not count -- and -inf makes them (-inf, inf, -inf).  theta has the pixel's sign, so the pixel is outside the domain, the logits
# stay infinite for the whole run and the dyadic pair rule is an exact oracle for that image.
INF_PIXEL = (1, 5)                   # image, feature
INF_ITERS = 4


def inf_case(sign):
    """(model, params, x with the pixel at sign * inf, x without, target, theta)."""
    rs = np.random.RandomState(41)
    k = rs.randint(1, 4, (16, 3)) * rs.choice([-1, 1], (16, 3))
    k[INF_PIXEL[1]] = (1, -2, 3)
    x = images(4, (4, 4, 1), 42)
    bad = x.copy()
    bad[INF_PIXEL[0]].reshape(-1)[INF_PIXEL[1]] = sign * INF
    return (model_of("lin3", (4, 4, 1)), [((k / 8.0).astype(np.float32), np.zeros(3, np.float32))], bad, x, np.full(4, 2, np.int32),
            float(sign))


# 8. the early exit: a linear model on 4 x 4 over 64 images; the batches are the images the float64 run finishes in exactly 1 and 2 steps
EXIT_CASE = _case("lin5", (4, 4, 1), 64, of_probs=0, clf_seed=11, x_seed=2, max_iters=5)


def exit_batches():
    """(model, params, x, target, ref, {1: indices, 2: indices}): the decidable images of EXIT_CASE that reach their target after
    exactly 1 and exactly 2 steps."""
    m, p, x, t = case_inputs(EXIT_CASE)
    ref = case_run(EXIT_CASE)
    dec = decidable(ref)
    done = ref["final_class"] == ref["target"]
    return m, p, x, t, ref, {k: np.flatnonzero(dec & done & (ref["iters"] == k)) for k in (1, 2)}
